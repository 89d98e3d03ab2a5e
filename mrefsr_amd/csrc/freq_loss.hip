// The frequency-domain losses of the training step (train.freq_opt; losses.FFTLoss, losses.FocalFrequencyLoss) and
// their gradient towards pred: a dense 2-D DFT of the residual X = pred - target of every [H][W] plane as two small GEMMs on
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation, k-ordered), no FFT library.
//
//   D[ky][kx] = sum_h sum_x X[h][x] e^(-2 pi i (ky h / H + kx x / W)),   kx = 0 .. W/2 (Wh = W/2 + 1 columns: X is real, the other
//   columns are the conjugates D[-ky][-kx]; their share of a sum over the full spectrum is the multiplicity mult = 1 for kx = 0 and
//   for kx = W/2 with W even, 2 otherwise).
//
// Twiddles: tab_n[r] = (cos, sin)(2 pi r / n), r = 0 .. n-1, the fp32 rounding of the float64 values, built by the caller once per
// (device, n); a block copies the table of its pass into LDS (8 KiB at n = 1024) and indexes it by (j k) mod n.  The index is
// carried in integers: one `%` per lane at the start, then an add and a conditional subtract per step; j k is never formed in
// floating point.
//
// Launches (block = 4 waves, tile 32 x 32 outputs, one 16 x 16 MFMA tile per wave; lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15]
// and D[4 (l >> 4) + r][l & 15]):
//   row_fwd     T = X F_W (real x complex): rows of ALL planes as one [planes H][W] matrix, X formed on load; a lane reads the four
//               x = k0 + 4 (l >> 4) + e of a 16-wide k step and feeds element e to the e-th MFMA pair.  T [planes][H][Wh][2] -> scratch.
//   col<FFT>    D = F_H T (complex x complex) per plane, epilogue: sum mult (|Re D| + |Im D|), G = sign(D) mult gs.
//   col<FOCAL>  the same product, epilogue: D gs_d -> the map, per-block maximum of w = sqrt(m)^alpha, m = Re D^2 + Im D^2.
//   focal_fin   per plane: the maximum of its blocks' maxima, w / max (NaN -> 0, clamped to [0, 1]), sum mult w m,
//               G = 2 w D mult gs in place.
//   col<ADJ>    U = F_H^H G (backward, first launch) -> scratch.
//   row_bwd     grad = f Re(U F_W^H), f = loss_weight grad_loss[0] read on the device; every element of grad_pred written once.
// FFTLoss: 2 forward launches; FocalFrequencyLoss: 3; backward: 2.  The imaginary part of a self-conjugate bin (ky in {0, H/2},
// kx in {0, W/2}) is structurally zero and is set to zero.
//
// Sums: a thread adds its four values r = 0..3, the 256 threads by an LDS tree, one fp32 partial per block (write-through); the
// block that draws the last ticket (reduce.h) adds the partials in ascending block order in double and writes the loss.  No float
// atomics, no readback, the same bits from call to call.  The maximum is order-free.
#include <math.h>

#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 32;         // output rows / columns per block
constexpr int THREADS = 256;
constexpr int MAXN = 1024;       // largest H or W: the twiddle table of a pass fits LDS
constexpr int FIN = 4;           // elements per thread of focal_fin

enum { MODE_FFT = 0, MODE_FOCAL = 1, MODE_ADJ = 2 };

__device__ __forceinline__ void load_table(float2 *__restrict__ tab, const float2 *__restrict__ src, const int n)
{
    for (int i = threadIdx.x; i < n; i += THREADS) tab[i] = src[i];
    __syncthreads();
}

__device__ __forceinline__ int wrap(const int idx, const int n) { return idx >= n ? idx - n : idx; }

__device__ __forceinline__ float mult_of(const int kx, const int W) { return (kx == 0 || 2 * kx == W) ? 1.f : 2.f; }

__device__ __forceinline__ float sign_of(const float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// m = Re^2 + Im^2 and w = sqrt(m)^alpha with the roundings spelt out: col<FOCAL> and focal_fin must give the same bits
__device__ __forceinline__ float power_of(const float re, const float im) { return __fmaf_rn(re, re, __fmul_rn(im, im)); }

__device__ __forceinline__ float weight_of(const float m, const float alpha)
{
    const float a = __fsqrt_rn(m);
    return alpha == 1.f ? a : powf(a, alpha);   // (powf(0, 0) = 1, as torch)
}

// T[row][kx] = sum_x (pred - target)[row][x] (cos, -sin)(2 pi kx x / W); rows = planes H.  grid (row tiles, column tiles)
__global__ __launch_bounds__(THREADS) void row_fwd_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                          const float2 *__restrict__ tabw, const long rows, const int W, const int Wh,
                                                          float2 *__restrict__ T)
{
    __shared__ float2 tab[MAXN];
    load_table(tab, tabw, W);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kl = lane >> 4, cl = lane & 15;
    const long row0 = (long)blockIdx.x * TILE + 16 * (wave >> 1);
    const int kx0 = blockIdx.y * TILE + 16 * (wave & 1);
    const long row = row0 + cl;
    const bool rok = row < rows;
    const float *pr = pred + (rok ? row : 0) * W, *tg = target + (rok ? row : 0) * W;
    const int kxc = kx0 + cl < Wh ? kx0 + cl : 0;
    int idx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) idx[e] = (kxc * (4 * kl + e)) % W;
    const int step = (16 * kxc) % W;
    f32x4 re = {0.f, 0.f, 0.f, 0.f}, im = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < W; k0 += 16) {
        float a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int x = k0 + 4 * kl + e;
            a[e] = (rok && x < W) ? pr[x] - tg[x] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float2 cs = tab[idx[e]];
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], cs.x, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], cs.y, im, 0, 0, 0);
            idx[e] = wrap(idx[e] + step, W);
        }
    }
    const int kx = kx0 + cl;
    if (kx >= Wh) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long orow = row0 + 4 * kl + r;
        if (orow < rows) T[orow * Wh + kx] = make_float2(re[r], -im[r]);
    }
}

// the column pass of one plane: out[i][kx] = sum_k e^(-+ 2 pi i (i k) / H) src[k][kx] (ADJ: the + sign), i, k = 0 .. H-1, and the
// epilogue of its mode.  grid (column tiles, row tiles, planes)
template <int MODE>
__global__ __launch_bounds__(THREADS) void col_kernel(const float2 *__restrict__ src, const float2 *__restrict__ tabh, const int H,
                                                      const int W, const int Wh, const float gs, const float alpha,
                                                      float2 *__restrict__ out, const int write_out, float *partial,
                                                      unsigned int *ticket, const double factor, float *__restrict__ loss)
{
    __shared__ float2 tab[MAXN];
    __shared__ float red[THREADS];
    __shared__ int last;
    load_table(tab, tabh, H);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kl = lane >> 4, cl = lane & 15;
    const int i0 = blockIdx.y * TILE + 16 * (wave >> 1), kx0 = blockIdx.x * TILE + 16 * (wave & 1);
    const long plane = (long)blockIdx.z * H * Wh;
    const int ic = i0 + cl < H ? i0 + cl : 0;
    const int kx = kx0 + cl;
    const bool kok = kx < Wh;
    const float2 *sp = src + plane + (kok ? kx : 0);
    int idx = (ic * kl) % H;
    const int step = (4 * ic) % H;
    f32x4 re = {0.f, 0.f, 0.f, 0.f}, im = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < H; k += 4) {
        const int h = k + kl;
        const float2 b = (kok && h < H) ? sp[(long)h * Wh] : make_float2(0.f, 0.f);
        const float2 cs = tab[idx];
        const float s = MODE == MODE_ADJ ? -cs.y : cs.y;
        // (c - i s)(b.x + i b.y) = (c b.x + s b.y) + i (c b.y - s b.x)
        re = __builtin_amdgcn_mfma_f32_16x16x4f32(cs.x, b.x, re, 0, 0, 0);
        re = __builtin_amdgcn_mfma_f32_16x16x4f32(s, b.y, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_16x16x4f32(cs.x, b.y, im, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_16x16x4f32(-s, b.x, im, 0, 0, 0);
        idx = wrap(idx + step, H);
    }
    if constexpr (MODE == MODE_ADJ) {
        if (!kok) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * kl + r;
            if (i < H) out[plane + (long)i * Wh + kx] = make_float2(re[r], im[r]);
        }
    } else {
        const float mult = mult_of(kx, W);
        const bool xself = kx == 0 || 2 * kx == W;
        float v = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ky = i0 + 4 * kl + r;
            if (!kok || ky >= H) continue;
            float dre = re[r], dim = (xself && (ky == 0 || 2 * ky == H)) ? 0.f : im[r];
            if constexpr (MODE == MODE_FFT) {
                v += mult * (fabsf(dre) + fabsf(dim));
                if (write_out) out[plane + (long)ky * Wh + kx] = make_float2(sign_of(dre) * (mult * gs), sign_of(dim) * (mult * gs));
            } else {
                dre *= gs, dim *= gs;
                out[plane + (long)ky * Wh + kx] = make_float2(dre, dim);
                v = fmaxf(v, weight_of(power_of(dre, dim), alpha));
            }
        }
        const unsigned int nblocks = gridDim.x * gridDim.y * gridDim.z;
        const unsigned int bid = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        const int tid = threadIdx.x;
        if constexpr (MODE == MODE_FFT) {
            // the block's tree sum written through; the block that arrives last adds the partials in block order: fl32(factor total)
            const float bsum = mrefsr::block_sum<THREADS>(red, v);
            if (tid == 0) mrefsr::store_partial(partial + bid, bsum);
            if (!mrefsr::last_block_by_ticket(ticket, nblocks, &last)) return;
            const double total = mrefsr::sum_partials_in_order(partial, nblocks, red);
            if (tid == 0) loss[0] = (float)(factor * total);
        } else {
            const float bmax = mrefsr::block_max<THREADS>(red, v);
            if (tid == 0) partial[bid] = bmax;
        }
    }
}

// grid (chunks of 1024 coefficients, planes): the plane's maximum from the `per_plane` block maxima of col<FOCAL>, the weights, the
// loss and -- with write_g -- the gradient map over D in place
__global__ __launch_bounds__(THREADS) void focal_fin_kernel(float2 *__restrict__ d, const float *__restrict__ wmax, const int per_plane,
                                                            const int H, const int W, const int Wh, const float alpha, const float gs,
                                                            const int write_g, float *partial, unsigned int *ticket, const double factor,
                                                            float *__restrict__ loss)
{
    __shared__ float red[THREADS];
    __shared__ int last;
    const int tid = threadIdx.x;
    float mx = 0.f;
    for (int i = tid; i < per_plane; i += THREADS) mx = fmaxf(mx, wmax[(long)blockIdx.y * per_plane + i]);
    mx = mrefsr::block_max<THREADS>(red, mx);
    const int n = H * Wh;
    float2 *dp = d + (long)blockIdx.y * n;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < FIN; ++k) {
        const int e = (blockIdx.x * FIN + k) * THREADS + tid;
        if (e >= n) continue;
        const float2 c = dp[e];
        const float m = power_of(c.x, c.y);
        float w = weight_of(m, alpha) / mx;
        w = w != w ? 0.f : fminf(fmaxf(w, 0.f), 1.f);
        const float mult = mult_of(e % Wh, W);
        v += mult * (w * m);
        if (write_g) {
            const float f = 2.f * mult * gs * w;
            dp[e] = make_float2(f * c.x, f * c.y);
        }
    }
    // as col<FFT>: tree sum, partial written through, the last block's ordered total in double
    const unsigned int nblocks = gridDim.x * gridDim.y;
    const float bsum = mrefsr::block_sum<THREADS>(red, v);
    if (tid == 0) mrefsr::store_partial(partial + blockIdx.y * gridDim.x + blockIdx.x, bsum);
    if (!mrefsr::last_block_by_ticket(ticket, nblocks, &last)) return;
    const double total = mrefsr::sum_partials_in_order(partial, nblocks, red);
    if (tid == 0) loss[0] = (float)(factor * total);
}

// grad[row][x] = f sum_kx (Re U[row][kx] cos(2 pi kx x / W) - Im U[row][kx] sin(2 pi kx x / W)); grid (row tiles, column tiles)
__global__ __launch_bounds__(THREADS) void row_bwd_kernel(const float2 *__restrict__ U, const float2 *__restrict__ tabw,
                                                          const float *__restrict__ gup, const float loss_weight, const long rows,
                                                          const int W, const int Wh, float *__restrict__ grad)
{
    __shared__ float2 tab[MAXN];
    load_table(tab, tabw, W);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kl = lane >> 4, cl = lane & 15;
    const long row0 = (long)blockIdx.x * TILE + 16 * (wave >> 1);
    const int x0 = blockIdx.y * TILE + 16 * (wave & 1);
    const long row = row0 + cl;
    const bool rok = row < rows;
    const float2 *up = U + (rok ? row : 0) * Wh;
    const int xc = x0 + cl < W ? x0 + cl : 0;
    int idx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) idx[e] = (xc * (4 * kl + e)) % W;
    const int step = (16 * xc) % W;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Wh; k0 += 16) {
        float2 u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int kx = k0 + 4 * kl + e;
            u[e] = (rok && kx < Wh) ? up[kx] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float2 cs = tab[idx[e]];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(u[e].x, cs.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(u[e].y, -cs.y, acc, 0, 0, 0);
            idx[e] = wrap(idx[e] + step, W);
        }
    }
    const int x = x0 + cl;
    if (x >= W) return;
    const float f = __fmul_rn(loss_weight, gup[0]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long orow = row0 + 4 * kl + r;
        if (orow < rows) grad[orow * W + x] = f * acc[r];
    }
}

bool shape_ok(const int planes, const int h, const int w)
{
    // (planes in the grid's z; every element offset in 31 bits)
    return planes > 0 && planes <= 65535 && h >= 1 && h <= MAXN && w >= 1 && w <= MAXN && (int64_t)planes * h * w <= ((int64_t)1 << 30);
}

}  // namespace

MREFSR_EXPORT int mrefsr_freq_loss_blocks(int planes, int h, int w)
{
    if (!shape_ok(planes, h, w)) return -1;
    return planes * mrefsr::cdiv(h, TILE) * mrefsr::cdiv(w / 2 + 1, TILE);
}

MREFSR_EXPORT int mrefsr_freq_loss_fwd_f32(const float *pred, const float *target, int planes, int h, int w, int focal, int ortho, float alpha,
                                           float loss_weight, const float *tab_h, const float *tab_w, float *t, float *g, int write_g,
                                           float *partial, uint32_t *ticket, float *loss, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(shape_ok(planes, h, w), "freq_loss_fwd: planes=%d (1..65535) h=%d w=%d (1..1024, planes*h*w <= 2^30)", planes, h, w);
    MREFSR_REQUIRE(pred && target && tab_h && tab_w && t && partial && ticket && loss, "freq_loss_fwd: null pointer");
    MREFSR_REQUIRE(g || (!focal && !write_g), "freq_loss_fwd: the map g is needed with write_g and by the focal form");
    MREFSR_REQUIRE(!focal || (alpha >= 0.f && alpha <= 3.0e38f), "freq_loss_fwd: alpha=%g is not a finite value >= 0", (double)alpha);
    const int wh = w / 2 + 1;
    const long rows = (long)planes * h;
    const double count = (double)planes * h * w, root = sqrt((double)h * w);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(row_fwd_kernel, dim3(mrefsr::cdiv(rows, TILE), mrefsr::cdiv(wh, TILE)), dim3(THREADS), 0, st, pred, target,
                       (const float2 *)tab_w, rows, w, wh, (float2 *)t);
    const dim3 grid(mrefsr::cdiv(wh, TILE), mrefsr::cdiv(h, TILE), planes);
    if (!focal) {
        // loss = loss_weight s sum mult (|Re| + |Im|) / (2 count), s the norm's scale; G = sign mult s / (2 count)
        const double s = (ortho ? 1.0 / root : 1.0) / (2.0 * count);
        hipLaunchKernelGGL(col_kernel<MODE_FFT>, grid, dim3(THREADS), 0, st, (const float2 *)t, (const float2 *)tab_h, h, w, wh, (float)s, 0.f,
                           (float2 *)g, write_g, partial, ticket, (double)loss_weight * s, loss);
        return mrefsr::check_launch("freq_loss_fwd");
    }
    // D = the ortho spectrum; loss = loss_weight sum mult w m / count; G = 2 w D mult / (count sqrt(h w)) towards the raw transform
    const int per_plane = grid.x * grid.y;
    float *wmax = partial, *part = partial + (long)planes * per_plane;
    hipLaunchKernelGGL(col_kernel<MODE_FOCAL>, grid, dim3(THREADS), 0, st, (const float2 *)t, (const float2 *)tab_h, h, w, wh,
                       (float)(1.0 / root), alpha, (float2 *)g, 1, wmax, ticket, 0.0, loss);
    hipLaunchKernelGGL(focal_fin_kernel, dim3(mrefsr::cdiv((long)h * wh, FIN * THREADS), planes), dim3(THREADS), 0, st, (float2 *)g, wmax,
                       per_plane, h, w, wh, alpha, (float)(1.0 / (count * root)), write_g, part, ticket, (double)loss_weight / count, loss);
    return mrefsr::check_launch("freq_loss_fwd");
}

MREFSR_EXPORT int mrefsr_freq_loss_bwd_f32(const float *g, const float *grad_loss, int planes, int h, int w, float loss_weight,
                                           const float *tab_h, const float *tab_w, float *u, float *grad_pred, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(shape_ok(planes, h, w), "freq_loss_bwd: planes=%d (1..65535) h=%d w=%d (1..1024, planes*h*w <= 2^30)", planes, h, w);
    MREFSR_REQUIRE(g && grad_loss && tab_h && tab_w && u && grad_pred, "freq_loss_bwd: null pointer");
    const int wh = w / 2 + 1;
    const long rows = (long)planes * h;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(col_kernel<MODE_ADJ>, dim3(mrefsr::cdiv(wh, TILE), mrefsr::cdiv(h, TILE), planes), dim3(THREADS), 0, st,
                       (const float2 *)g, (const float2 *)tab_h, h, w, wh, 0.f, 0.f, (float2 *)u, 1, (float *)nullptr,
                       (unsigned int *)nullptr, 0.0, (float *)nullptr);
    hipLaunchKernelGGL(row_bwd_kernel, dim3(mrefsr::cdiv(rows, TILE), mrefsr::cdiv(w, TILE)), dim3(THREADS), 0, st, (const float2 *)u,
                       (const float2 *)tab_w, grad_loss, loss_weight, rows, w, wh, grad_pred);
    return mrefsr::check_launch("freq_loss_bwd");
}
