// The operators of the Real-ESRGAN second-order degradation (opt['degradation'], mrefsr_amd/degradation.py), forward only
// (the chain runs under no_grad), fp32 NCHW.  Each kernel restates one operator of the reference:
//   filter2d   basicsr/utils/img_process_util.py:7-31 (filter2D: reflect padding + per-sample k x k correlation)
//   usm        basicsr/utils/img_process_util.py:63-83 (USMSharp.forward), the Gaussian as a row and a column pass
//   resize     F.interpolate(mode = area | bilinear | bicubic, align_corners=False) as realesrgan_model.py:95, 126, 151, 164 call it
//   noise      basicsr/data/degradations.py:461-514 (Gaussian) and :610-684 (Poisson), on random tensors drawn by the caller
//   levels     the len(torch.unique(...)) loops of degradations.py:630-648, without a readback
//   jpeg       basicsr/utils/diffjpeg.py:449-491, DiffJPEG(differentiable=False)
//
// filter2d: block (tx, ty, plane) owns 16 x 64 pixels of one channel plane.  It stages the (16 + 2p) x (64 + 2p) pixels under its
// windows (p = k / 2 <= 10) into LDS, the reflect padding resolved by index arithmetic on load (there is no padded copy; positions
// further than p outside the image are read by no pixel inside it and are staged as 0), and the sample's k x k taps next to them.
// Thread t has column t % 64 and the rows t / 64 + 4 j, j < 4: a wave reads 64 consecutive floats of a staged row (no bank conflict)
// and a tap it loads once (a broadcast) serves four pixels.  The taps of a kernel row are added in order, then the k row sums.
//
// usm: two launches over 32 x 32 tiles of a plane, both the same separable blur: stage (32 + 2p)^2 pixels (p = 25 for radius 51:
// 82 x 82 floats = 26.3 KiB), blur the rows into a (32 + 2p) x 32 array (10.3 KiB), then the columns.  Launch 1 stages the image and
// writes the residual r = img - blur; launch 2 stages the hard mask [|r| 255 > threshold] computed from r on load, blurs it to the
// soft mask and writes soft clip(img + weight r, 0, 1) + (1 - soft) img.  Per pixel 2 (2p + 1) LDS taps instead of (2p + 1)^2.
//
// resize: one thread per output pixel of a plane; the coordinate scales come from the caller (1 / scale_factor or in / out: torch
// uses the former when it is called with scale_factor, the latter with size).  bilinear and bicubic in torch's operation order,
// area by adaptive_avg_pool2d's window rule floor(i in / out) ... ceil((i + 1) in / out).
//
// noise: one thread per pixel, the three channels together (they share the gray draw), every operation in the reference's order
// (this file is built with -ffp-contract=off).  levels: block (x, b) ORs the levels round(clamp(img 255)) of its pixels' channels and
// of their gray value into two 256-bit sets in LDS, then into the sample's sets in device memory; the sample's last block (a ticket
// per sample) counts the bits, writes 2^ceil(log2(count)) and leaves sets and ticket zero for the next launch.
//
// jpeg: one block per 16 x 16 macroblock, one thread per pixel, everything between the load and the store in LDS: x 255 -> YCbCr
// -> 2 x 2 chroma mean -> six 8 x 8 blocks (4 Y, Cb, Cr) - 128 -> DCT as a pass over columns and a pass over rows -> / (table
// factor) -> round half to even -> x (table factor) -> inverse DCT the same way + 128 -> chroma replicated -> RGB -> clamp -> / 255.
// Pixels outside the image are zeros on load (the reference's zero padding to multiples of 16) and are not stored (its crop).
#include <math.h>

#include "common.h"

namespace {

constexpr int THREADS = 256;

// index i in [-p, n + p) of the reflect-padded axis -> [0, n) (p < n: one reflection is enough)
__device__ __forceinline__ int reflect(const int i, const int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__device__ __forceinline__ float clamp01(const float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// ---------------------------------------------------------------------------------------------------------------- filter2d
constexpr int F_TH = 16, F_TW = 64, F_MAXK = 21, F_ROWS = 4;          // F_TH / F_ROWS rows of threads, F_ROWS pixels each
constexpr int F_SH = F_TH + F_MAXK - 1, F_SW = F_TW + F_MAXK - 1;     // 36 x 84 staged floats at most

__global__ __launch_bounds__(THREADS) void filter2d_kernel(const float *__restrict__ img, const float *__restrict__ kern, const int kern_stride,
                                                           const int C, const int H, const int W, const int k, float *__restrict__ out)
{
    __shared__ float s[F_SH * F_SW];
    __shared__ float wk[F_MAXK * F_MAXK];
    const int tid = threadIdx.x, pad = k / 2;
    const int y0 = blockIdx.y * F_TH, x0 = blockIdx.x * F_TW;
    const long plane = blockIdx.z, hw = (long)H * W;
    const float *src = img + plane * hw;
    const float *taps = kern + (plane / C) * (long)kern_stride;
    const int sh = F_TH + 2 * pad, sw = F_TW + 2 * pad;

    for (int idx = tid; idx < k * k; idx += THREADS) wk[idx] = taps[idx];
    for (int idx = tid; idx < sh * sw; idx += THREADS) {
        const int r = idx / sw, c = idx % sw;
        const int py = y0 - pad + r, px = x0 - pad + c;   // padded coordinates, >= -pad
        float v = 0.f;
        if (py < H + pad && px < W + pad) v = src[(long)reflect(py, H) * W + reflect(px, W)];
        s[r * F_SW + c] = v;
    }
    __syncthreads();

    const int cx = tid % F_TW, r0 = tid / F_TW;
    float acc[F_ROWS] = {0.f, 0.f, 0.f, 0.f};
    for (int dy = 0; dy < k; ++dy) {   // k sums of k taps, then their sum: the rounding error grows with 2 sqrt(k), not k
        float row[F_ROWS] = {0.f, 0.f, 0.f, 0.f};
        for (int dx = 0; dx < k; ++dx) {
            const float wv = wk[dy * k + dx];
#pragma unroll
            for (int j = 0; j < F_ROWS; ++j) row[j] += wv * s[(r0 + 4 * j + dy) * F_SW + cx + dx];
        }
#pragma unroll
        for (int j = 0; j < F_ROWS; ++j) acc[j] += row[j];
    }
    const int gx = x0 + cx;
    if (gx >= W) return;
#pragma unroll
    for (int j = 0; j < F_ROWS; ++j) {
        const int gy = y0 + r0 + 4 * j;
        if (gy < H) out[plane * hw + (long)gy * W + gx] = acc[j];
    }
}

// ---------------------------------------------------------------------------------------------------------------- usm
constexpr int U_T = 32, U_MAXK = 51, U_S = U_T + U_MAXK - 1;          // 32 x 32 tile, 82 x 82 staged floats at most
constexpr int U_PER_THREAD = U_T * U_T / THREADS;                     // 4

struct UsmTaps { float g[U_MAXK]; };

// FINAL = false: out = img - blur(img).  FINAL = true: `res` is that residual; out = soft clip(img + weight res) + (1 - soft) img
// with soft = blur([|res| 255 > threshold]).
template <bool FINAL>
__global__ __launch_bounds__(THREADS) void usm_kernel(const float *__restrict__ img, const float *__restrict__ res, const UsmTaps taps,
                                                      const int H, const int W, const int k, const float weight, const float threshold,
                                                      float *__restrict__ out)
{
    __shared__ float s[U_S * U_S];      // the image (or the hard mask) under the tile's windows
    __shared__ float hrow[U_S * U_T];   // its rows blurred
    __shared__ float g[U_MAXK];
    const int tid = threadIdx.x, pad = k / 2, side = U_T + 2 * pad;
    const int y0 = blockIdx.y * U_T, x0 = blockIdx.x * U_T;
    const long plane = blockIdx.z, hw = (long)H * W;
    const float *src = (FINAL ? res : img) + plane * hw;

    if (tid < k) g[tid] = taps.g[tid];
    for (int idx = tid; idx < side * side; idx += THREADS) {
        const int r = idx / side, c = idx % side;
        const int py = y0 - pad + r, px = x0 - pad + c;
        float v = 0.f;
        if (py < H + pad && px < W + pad) {
            v = src[(long)reflect(py, H) * W + reflect(px, W)];
            if constexpr (FINAL) v = fabsf(v) * 255.f > threshold ? 1.f : 0.f;
        }
        s[r * U_S + c] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < side * U_T; idx += THREADS) {
        const int r = idx / U_T, c = idx % U_T;
        float a = 0.f;
        for (int t = 0; t < k; ++t) a += g[t] * s[r * U_S + c + t];
        hrow[idx] = a;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < U_PER_THREAD; ++j) {
        const int idx = j * THREADS + tid, r = idx / U_T, c = idx % U_T;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        float a = 0.f;
        for (int t = 0; t < k; ++t) a += g[t] * hrow[(r + t) * U_T + c];
        const long off = plane * hw + (long)gy * W + gx;
        if constexpr (FINAL) {
            const float v = img[off];
            const float sharp = clamp01(v + weight * res[off]);
            out[off] = a * sharp + (1.f - a) * v;
        } else {
            out[off] = s[(r + pad) * U_S + c + pad] - a;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- resize
enum { MODE_AREA = 0, MODE_BILINEAR = 1, MODE_BICUBIC = 2 };

// torch's cubic convolution coefficients (UpSample.h: A = -0.75)
__device__ __forceinline__ void cubic_coeffs(float c[4], const float t)
{
    constexpr float A = -0.75f;
    const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = x2 + 1.f;
    c[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    c[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
    c[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    c[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void resize_kernel(const float *__restrict__ in, const int H, const int W, const int OH, const int OW,
                                                         const float scale_h, const float scale_w, float *__restrict__ out)
{
    const long plane = blockIdx.y, i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (long)OH * OW) return;
    const int oy = (int)(i / OW), ox = (int)(i % OW);
    const float *src = in + plane * (long)H * W;
    float v;
    if constexpr (MODE == MODE_AREA) {
        const int ys = (int)(((long)oy * H) / OH), ye = (int)((((long)oy + 1) * H + OH - 1) / OH);
        const int xs = (int)(((long)ox * W) / OW), xe = (int)((((long)ox + 1) * W + OW - 1) / OW);
        float sum = 0.f;
        for (int y = ys; y < ye; ++y)
            for (int x = xs; x < xe; ++x) sum += src[(long)y * W + x];
        v = sum / (float)((ye - ys) * (xe - xs));
    } else if constexpr (MODE == MODE_BILINEAR) {
        const float sy = fmaxf(scale_h * ((float)oy + 0.5f) - 0.5f, 0.f), sx = fmaxf(scale_w * ((float)ox + 0.5f) - 0.5f, 0.f);
        const int iy = min((int)sy, H - 1), ix = min((int)sx, W - 1);
        const int iy1 = iy + (iy < H - 1 ? 1 : 0), ix1 = ix + (ix < W - 1 ? 1 : 0);
        const float ly1 = fminf(fmaxf(sy - (float)iy, 0.f), 1.f), lx1 = fminf(fmaxf(sx - (float)ix, 0.f), 1.f);
        const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
        v = ly0 * (lx0 * src[(long)iy * W + ix] + lx1 * src[(long)iy * W + ix1]) +
            ly1 * (lx0 * src[(long)iy1 * W + ix] + lx1 * src[(long)iy1 * W + ix1]);
    } else {
        const float sy = scale_h * ((float)oy + 0.5f) - 0.5f, sx = scale_w * ((float)ox + 0.5f) - 0.5f;
        const float fy = floorf(sy), fx = floorf(sx);
        // (the taps are clamped into the image below; clamping the base first keeps the int conversion defined for any scale)
        const int iy = (int)fminf(fmaxf(fy, -2.f), (float)H + 1.f), ix = (int)fminf(fmaxf(fx, -2.f), (float)W + 1.f);
        float cy[4], cx[4];
        cubic_coeffs(cy, sy - fy);
        cubic_coeffs(cx, sx - fx);
        float rows[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long yo = (long)min(max(iy - 1 + a, 0), H - 1) * W;
            float p[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) p[b] = src[yo + min(max(ix - 1 + b, 0), W - 1)];
            rows[a] = p[0] * cx[0] + p[1] * cx[1] + p[2] * cx[2] + p[3] * cx[3];
        }
        v = rows[0] * cy[0] + rows[1] * cy[1] + rows[2] * cy[2] + rows[3] * cy[3];
    }
    out[plane * (long)OH * OW + i] = v;
}

// ---------------------------------------------------------------------------------------------------------------- noise
enum { NOISE_GAUSSIAN = 0, NOISE_POISSON = 1 };
// `x / 255.` of the reference: torch on the GPU divides a tensor by a host scalar as x * (1 / 255) with the reciprocal in fp32
constexpr float INV255 = 1.f / 255.f;

// round(x 255) clamped to 0 ... 255 (torch.round: half to even), as a float
__device__ __forceinline__ float level255(const float x) { return fminf(fmaxf(rintf(x * 255.f), 0.f), 255.f); }

__device__ __forceinline__ float gray_of(const float r, const float g, const float b) { return (0.2989f * r + 0.587f * g) + 0.114f * b; }

template <int MODE>
__global__ __launch_bounds__(THREADS) void noise_kernel(const float *__restrict__ img, const float *__restrict__ a, const float *__restrict__ ag,
                                                        const float *__restrict__ param, const float *__restrict__ gray,
                                                        const float *__restrict__ vals, const long hw, float *__restrict__ out)
{
    const long b = blockIdx.y, i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= hw) return;
    const float p = param[b], gf = gray[b], cf = 1.f - gf;
    const float *x = img + 3 * b * hw + i, *n = a + 3 * b * hw + i;
    float *o = out + 3 * b * hw + i;
    const float ngv = ag[b * hw + i];
    if constexpr (MODE == NOISE_GAUSSIAN) {
        const float ng = ngv * p * INV255;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float nc = n[c * hw] * p * INV255;
            o[c * hw] = clamp01(x[c * hw] + (nc * cf + ng * gf));
        }
    } else {
        const float v0 = vals[2 * b], v1 = vals[2 * b + 1];
        const float r = x[0], g = x[hw], bl = x[2 * hw];
        const float ng = ngv / v1 - level255(gray_of(r, g, bl)) * INV255;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float xc = x[c * hw];
            const float nc = n[c * hw] / v0 - level255(xc) * INV255;
            o[c * hw] = clamp01(xc + (nc * cf + ng * gf) * p);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- levels
constexpr int L_PIX = 2048;   // pixels per block

// sets: [B][16] words (8 of the colour levels, 8 of the gray levels) then [B] tickets; all zero on entry and on exit
__global__ __launch_bounds__(THREADS) void levels_kernel(const float *__restrict__ img, const long hw, unsigned int *sets, const int B,
                                                         float *__restrict__ vals)
{
    __shared__ unsigned int bits[16];
    __shared__ int last;
    const int tid = threadIdx.x;
    const long b = blockIdx.y;
    if (tid < 16) bits[tid] = 0u;
    __syncthreads();
    const float *x = img + 3 * b * hw;
    const long end = min(hw, ((long)blockIdx.x + 1) * L_PIX);
    for (long i = (long)blockIdx.x * L_PIX + tid; i < end; i += THREADS) {
        const float r = x[i], g = x[hw + i], bl = x[2 * hw + i];
        const int lr = (int)level255(r), lg = (int)level255(g), lb = (int)level255(bl), ly = (int)level255(gray_of(r, g, bl));
        atomicOr(&bits[lr >> 5], 1u << (lr & 31));
        atomicOr(&bits[lg >> 5], 1u << (lg & 31));
        atomicOr(&bits[lb >> 5], 1u << (lb & 31));
        atomicOr(&bits[8 + (ly >> 5)], 1u << (ly & 31));
    }
    __syncthreads();
    unsigned int *mine = sets + 16 * b;
    if (tid < 16 && bits[tid]) __hip_atomic_fetch_or(mine + tid, bits[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!mrefsr::last_block_by_ticket(sets + 16 * (long)B + b, gridDim.x, &last)) return;
    if (tid < 16) {
        bits[tid] = __popc(__hip_atomic_load(mine + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        __hip_atomic_store(mine + tid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (tid < 2) {
        unsigned int count = 0;
        for (int q = 0; q < 8; ++q) count += bits[8 * tid + q];
        unsigned int v = 1;   // 2^ceil(log2(count)), count >= 1
        while (v < count) v <<= 1;
        vals[2 * b + tid] = (float)v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- jpeg
// cos(j pi / 16), j < 32, rounded from double
__constant__ float COS16[32] = {
    1.000000000e+00f, 9.807852507e-01f, 9.238795042e-01f, 8.314695954e-01f, 7.071067691e-01f, 5.555702448e-01f, 3.826834261e-01f, 1.950903237e-01f,
    6.123234263e-17f, -1.950903237e-01f, -3.826834261e-01f, -5.555702448e-01f, -7.071067691e-01f, -8.314695954e-01f, -9.238795042e-01f, -9.807852507e-01f,
    -1.000000000e+00f, -9.807852507e-01f, -9.238795042e-01f, -8.314695954e-01f, -7.071067691e-01f, -5.555702448e-01f, -3.826834261e-01f, -1.950903237e-01f,
    -1.836970147e-16f, 1.950903237e-01f, 3.826834261e-01f, 5.555702448e-01f, 7.071067691e-01f, 8.314695954e-01f, 9.238795042e-01f, 9.807852507e-01f};
// The quantisation tables as diffjpeg.py:14-23 holds them, i.e. TRANSPOSED from the JPEG standard's row-major listing: entry [u][v]
// divides the coefficient of vertical frequency u and horizontal frequency v.
__constant__ float Y_TABLE[64] = {16, 12, 14, 14, 18, 24, 49, 72,  11, 12, 13, 17, 22, 35, 64, 92,  10, 14, 16, 22, 37, 55, 78, 95,
                                  16, 19, 24, 29, 56, 64, 87, 98,  24, 26, 40, 51, 68, 81, 103, 112,  40, 58, 57, 87, 109, 104, 121, 100,
                                  51, 60, 69, 80, 103, 113, 120, 103,  61, 55, 56, 62, 77, 92, 101, 99};
__constant__ float C_TABLE[64] = {17, 18, 24, 47, 99, 99, 99, 99,  18, 21, 26, 66, 99, 99, 99, 99,  24, 26, 56, 99, 99, 99, 99, 99,
                                  47, 66, 99, 99, 99, 99, 99, 99,  99, 99, 99, 99, 99, 99, 99, 99,  99, 99, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99,  99, 99, 99, 99, 99, 99, 99, 99};
constexpr int J_LD = 9;         // row stride of an 8 x 8 block in LDS
constexpr int J_ITEMS = 6 * 64; // coefficients of a macroblock: 4 Y blocks, Cb, Cr
constexpr float INV_SQRT2 = 0.70710678118654752440f;

__global__ __launch_bounds__(THREADS) void jpeg_kernel(const float *__restrict__ img, const float *__restrict__ quality, const int H, const int W,
                                                       float *__restrict__ out)
{
    __shared__ float full[3][16][17];       // Y, Cb, Cr of the macroblock's pixels
    __shared__ float blk[6][8][J_LD];
    __shared__ float tmp[6][8][J_LD];
    __shared__ float cs[8][8];              // cs[k][n] = cos((2 n + 1) k pi / 16)
    const int tid = threadIdx.x, py = tid / 16, px = tid % 16;
    const int gy = blockIdx.y * 16 + py, gx = blockIdx.x * 16 + px;
    const long b = blockIdx.z, hw = (long)H * W;
    const bool inside = gy < H && gx < W;
    const long off = 3 * b * hw + (long)gy * W + gx;

    // quality -> factor (diffjpeg.py:32-45), in fp32 as the reference's tensor arithmetic
    const float q = quality[b];
    const float factor = (q < 50.f ? 5000.f / q : 200.f - q * 2.f) / 100.f;

    if (tid < 64) cs[tid / 8][tid % 8] = COS16[((2 * (tid % 8) + 1) * (tid / 8)) & 31];
    {
        const float r = inside ? img[off] * 255.f : 0.f, g = inside ? img[off + hw] * 255.f : 0.f, bl = inside ? img[off + 2 * hw] * 255.f : 0.f;
        full[0][py][px] = (0.299f * r + 0.587f * g) + 0.114f * bl;
        full[1][py][px] = ((-0.168736f * r + -0.331264f * g) + 0.5f * bl) + 128.f;
        full[2][py][px] = ((0.5f * r + -0.418688f * g) + -0.081312f * bl) + 128.f;
    }
    __syncthreads();
    for (int i = tid; i < J_ITEMS; i += THREADS) {
        const int m = i / 64, x = (i / 8) % 8, y = i % 8;
        float v;
        if (m < 4) {
            v = full[0][(m / 2) * 8 + x][(m % 2) * 8 + y];
        } else {
            const float(*c)[17] = full[m - 3];
            v = (((c[2 * x][2 * y] + c[2 * x][2 * y + 1]) + c[2 * x + 1][2 * y]) + c[2 * x + 1][2 * y + 1]) * 0.25f;
        }
        blk[m][x][y] = v - 128.f;
    }
    __syncthreads();
    // DCT: tmp[x][v] = sum_y blk[x][y] cos((2 y + 1) v pi / 16); coefficient [u][v] = scale sum_x tmp[x][v] cos((2 x + 1) u pi / 16)
    for (int i = tid; i < J_ITEMS; i += THREADS) {
        const int m = i / 64, x = (i / 8) % 8, v = i % 8;
        float a = 0.f;
#pragma unroll
        for (int y = 0; y < 8; ++y) a += blk[m][x][y] * cs[v][y];
        tmp[m][x][v] = a;
    }
    __syncthreads();
    for (int i = tid; i < J_ITEMS; i += THREADS) {
        const int m = i / 64, u = (i / 8) % 8, v = i % 8;
        float a = 0.f;
#pragma unroll
        for (int x = 0; x < 8; ++x) a += tmp[m][x][v] * cs[u][x];
        const float au = u == 0 ? INV_SQRT2 : 1.f, av = v == 0 ? INV_SQRT2 : 1.f;
        const float coef = (au * av * 0.25f) * a;
        const float table = (m < 4 ? Y_TABLE : C_TABLE)[u * 8 + v] * factor;
        // quantise, dequantise, and the inverse transform's alpha on the way
        blk[m][u][v] = (rintf(coef / table) * table) * (au * av);
    }
    __syncthreads();
    // inverse: tmp[x][v] = sum_y blk[x][y] cos((2 v + 1) y pi / 16); pixel [u][v] = 0.25 sum_x tmp[x][v] cos((2 u + 1) x pi / 16) + 128
    for (int i = tid; i < J_ITEMS; i += THREADS) {
        const int m = i / 64, x = (i / 8) % 8, v = i % 8;
        float a = 0.f;
#pragma unroll
        for (int y = 0; y < 8; ++y) a += blk[m][x][y] * cs[y][v];
        tmp[m][x][v] = a;
    }
    __syncthreads();
    for (int i = tid; i < J_ITEMS; i += THREADS) {
        const int m = i / 64, u = (i / 8) % 8, v = i % 8;
        float a = 0.f;
#pragma unroll
        for (int x = 0; x < 8; ++x) a += tmp[m][x][v] * cs[x][u];
        blk[m][u][v] = 0.25f * a + 128.f;
    }
    __syncthreads();
    if (!inside) return;
    const float yv = blk[(py / 8) * 2 + px / 8][py % 8][px % 8];
    const float cb = blk[4][py / 2][px / 2] - 128.f, cr = blk[5][py / 2][px / 2] - 128.f;
    const float r = yv + 1.402f * cr;   // (0 cb left out: the reference adds an exact zero)
    const float g = (yv + -0.344136f * cb) + -0.714136f * cr;
    const float bl = yv + 1.772f * cb;
    out[off] = fminf(fmaxf(r, 0.f), 255.f) / 255.f;
    out[off + hw] = fminf(fmaxf(g, 0.f), 255.f) / 255.f;
    out[off + 2 * hw] = fminf(fmaxf(bl, 0.f), 255.f) / 255.f;
}

// batch and planes within the grid's 65535, a plane's pixel count in 31 bits
bool image_ok(const int batch, const int c, const int h, const int w)
{
    return batch > 0 && c > 0 && (int64_t)batch * c <= 65535 && h > 0 && w > 0 && h <= (1 << 19) && w <= (1 << 19) && (int64_t)h * w <= ((int64_t)1 << 30);
}

}  // namespace

MREFSR_EXPORT int mrefsr_degrade_filter2d_f32(const float *img, const float *kernels, int batch, int c, int h, int w, int k, int shared,
                                              float *out, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(image_ok(batch, c, h, w), "degrade_filter2d: batch=%d c=%d (batch*c <= 65535) h=%d w=%d (<= 2^19, h*w <= 2^30)", batch, c, h, w);
    MREFSR_REQUIRE(k >= 3 && k <= F_MAXK && k % 2 == 1, "degrade_filter2d: k=%d must be odd, 3..%d", k, F_MAXK);
    MREFSR_REQUIRE(h > k / 2 && w > k / 2, "degrade_filter2d: h=%d w=%d must exceed k/2=%d (reflect padding)", h, w, k / 2);
    MREFSR_REQUIRE(mrefsr::cdiv(h, F_TH) <= 65535, "degrade_filter2d: h=%d too large", h);
    MREFSR_REQUIRE(img && kernels && out && img != out, "degrade_filter2d: null pointer or in-place call");
    const dim3 grid(mrefsr::cdiv(w, F_TW), mrefsr::cdiv(h, F_TH), batch * c);
    hipLaunchKernelGGL(filter2d_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, img, kernels, shared ? 0 : k * k, c, h, w, k, out);
    return mrefsr::check_launch("degrade_filter2d");
}

MREFSR_EXPORT int mrefsr_degrade_usm_f32(const float *img, const float *taps, int batch, int c, int h, int w, int k, float weight,
                                         float threshold, float *residual, float *out, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(image_ok(batch, c, h, w), "degrade_usm: batch=%d c=%d (batch*c <= 65535) h=%d w=%d (<= 2^19, h*w <= 2^30)", batch, c, h, w);
    MREFSR_REQUIRE(k >= 3 && k <= U_MAXK && k % 2 == 1, "degrade_usm: k=%d must be odd, 3..%d", k, U_MAXK);
    MREFSR_REQUIRE(h > k / 2 && w > k / 2, "degrade_usm: h=%d w=%d must exceed k/2=%d (reflect padding)", h, w, k / 2);
    MREFSR_REQUIRE(mrefsr::cdiv(h, U_T) <= 65535, "degrade_usm: h=%d too large", h);
    MREFSR_REQUIRE(img && taps && residual && out && img != out && img != residual && residual != out, "degrade_usm: null pointer or aliased buffers");
    UsmTaps t;
    for (int i = 0; i < U_MAXK; ++i) t.g[i] = i < k ? taps[i] : 0.f;
    const dim3 grid(mrefsr::cdiv(w, U_T), mrefsr::cdiv(h, U_T), batch * c);
    hipLaunchKernelGGL(usm_kernel<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, img, (const float *)nullptr, t, h, w, k, weight, threshold,
                       residual);
    hipLaunchKernelGGL(usm_kernel<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, img, (const float *)residual, t, h, w, k, weight, threshold,
                       out);
    return mrefsr::check_launch("degrade_usm");
}

MREFSR_EXPORT int mrefsr_degrade_resize_f32(const float *in, int batch, int c, int h, int w, int oh, int ow, int mode, float scale_h,
                                            float scale_w, float *out, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(image_ok(batch, c, h, w) && image_ok(batch, c, oh, ow),
                   "degrade_resize: batch=%d c=%d (batch*c <= 65535) %dx%d -> %dx%d (sides 1..2^19, pixels <= 2^30)", batch, c, h, w, oh, ow);
    MREFSR_REQUIRE(mode >= MODE_AREA && mode <= MODE_BICUBIC, "degrade_resize: mode=%d (0 area, 1 bilinear, 2 bicubic)", mode);
    MREFSR_REQUIRE(mode == MODE_AREA || (scale_h > 0.f && scale_w > 0.f && isfinite(scale_h) && isfinite(scale_w)),
                   "degrade_resize: coordinate scales %g, %g must be positive and finite", (double)scale_h, (double)scale_w);
    MREFSR_REQUIRE(in && out && in != out, "degrade_resize: null pointer or in-place call");
    const dim3 grid(mrefsr::cdiv((long)oh * ow, THREADS), batch * c);
    auto kernel = mode == MODE_AREA ? resize_kernel<MODE_AREA> : mode == MODE_BILINEAR ? resize_kernel<MODE_BILINEAR> : resize_kernel<MODE_BICUBIC>;
    hipLaunchKernelGGL(kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, in, h, w, oh, ow, scale_h, scale_w, out);
    return mrefsr::check_launch("degrade_resize");
}

MREFSR_EXPORT int mrefsr_degrade_noise_f32(const float *img, const float *noise, const float *noise_gray, const float *param, const float *gray,
                                           const float *vals, int batch, int h, int w, int mode, float *out, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(image_ok(batch, 3, h, w), "degrade_noise: batch=%d (3*batch <= 65535) h=%d w=%d (<= 2^19, h*w <= 2^30)", batch, h, w);
    MREFSR_REQUIRE(mode == NOISE_GAUSSIAN || mode == NOISE_POISSON, "degrade_noise: mode=%d (0 Gaussian, 1 Poisson)", mode);
    MREFSR_REQUIRE(img && noise && noise_gray && param && gray && out, "degrade_noise: null pointer");
    MREFSR_REQUIRE(mode == NOISE_GAUSSIAN || vals, "degrade_noise: the Poisson model needs vals (mrefsr_degrade_levels_f32)");
    const long hw = (long)h * w;
    const dim3 grid(mrefsr::cdiv(hw, THREADS), batch);
    auto kernel = mode == NOISE_GAUSSIAN ? noise_kernel<NOISE_GAUSSIAN> : noise_kernel<NOISE_POISSON>;
    hipLaunchKernelGGL(kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, img, noise, noise_gray, param, gray, vals, hw, out);
    return mrefsr::check_launch("degrade_noise");
}

MREFSR_EXPORT int64_t mrefsr_degrade_levels_workspace_words(int batch) { return batch > 0 ? 17 * (int64_t)batch : -1; }

MREFSR_EXPORT int mrefsr_degrade_levels_f32(const float *img, int batch, int h, int w, uint32_t *sets, float *vals, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(image_ok(batch, 3, h, w), "degrade_levels: batch=%d (3*batch <= 65535) h=%d w=%d (<= 2^19, h*w <= 2^30)", batch, h, w);
    MREFSR_REQUIRE(img && sets && vals, "degrade_levels: null pointer");
    const long hw = (long)h * w;
    const dim3 grid(mrefsr::cdiv(hw, L_PIX), batch);
    hipLaunchKernelGGL(levels_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, img, hw, sets, batch, vals);
    return mrefsr::check_launch("degrade_levels");
}

MREFSR_EXPORT int mrefsr_degrade_jpeg_f32(const float *img, const float *quality, int batch, int h, int w, float *out, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(image_ok(batch, 3, h, w) && batch <= 65535, "degrade_jpeg: batch=%d (3*batch <= 65535) h=%d w=%d (<= 2^19, h*w <= 2^30)", batch, h, w);
    MREFSR_REQUIRE(mrefsr::cdiv(h, 16) <= 65535, "degrade_jpeg: h=%d too large", h);
    MREFSR_REQUIRE(img && quality && out, "degrade_jpeg: null pointer");
    const dim3 grid(mrefsr::cdiv(w, 16), mrefsr::cdiv(h, 16), batch);
    hipLaunchKernelGGL(jpeg_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, img, quality, h, w, out);
    return mrefsr::check_launch("degrade_jpeg");
}
