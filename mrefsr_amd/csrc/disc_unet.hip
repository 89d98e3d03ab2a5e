// UNetDiscriminatorSN of the adversarial training step (basicsr/archs/discriminator_arch.py:127-200, Real-ESRGAN's U-Net
// discriminator with spectral normalisation): the kernels of mrefsr_amd/archs/nhwc_unetdisc.py that csrc/disc_vgg.hip does not have.
// conv0 .. conv8 run on disc_vgg.hip's convolutions (conv1 .. conv8 with the weights W_orig / sigma that sn_scale writes).
//   sn_*          spectral norm of up to 8 layers at once (torch.nn.utils.spectral_norm, n_power_iterations 1, dim 0):
//                   sn_wtu        partial t = W^T u over 32-row chunks (one launch for every layer)
//                   sn_v          per layer: t = sum of the chunks in order, v = t / max(|t|, eps)
//                   sn_wv         per (layer, row): s = W v, a fixed tree
//                   sn_u          per layer: u = s / max(|s|, eps) (training) or the stored u (eval); sigma = u . s
//                   sn_scale      W = W_orig / sigma for every layer
//                   sn_dot        per 16 K-element chunk of a layer: a partial <G, W_orig>
//                   sn_bwd        dW_orig = G / sigma - (<G, W_orig> / sigma^2) u v^T, the chunks' dot summed in order per block
//   up2 / up2_adj bilinear x2 (align_corners False) on NHWC maps, forward (optionally up(y + skip)) and its adjoint as a gather
//   add           out = a + b (the x6 + x0 skip)
//   conv9_*       nn.Conv2d(C, 1, 3, 1, 1): forward (+ bias), input gradient, weight gradient as a fixed-order split over pixels
// No float atomics anywhere: two runs give the same bits.
#include "disc_common.h"

namespace {

constexpr int SN_MAX = 8;     // layers per call
constexpr int SN_RC = 32;     // rows per chunk of W^T u
constexpr int SN_CH = 16384;  // elements per chunk of <G, W_orig>

struct SnTab {
    const float *w[SN_MAX];   // W_orig [rows][cols] (torch's [Cout][Cin][kh][kw] read as a matrix)
    float *u[SN_MAX];         // live buffers (updated in place in training mode)
    float *v[SN_MAX];
    const float *g[SN_MAX];   // sn_dot / sn_bwd: the gradient G of W
    float *o[SN_MAX];         // sn_scale: W; sn_bwd: dW_orig
    int rows[SN_MAX], cols[SN_MAX];
    long uoff[SN_MAX], voff[SN_MAX];   // offsets in the snapshots (and of s in the workspace: uoff)
    long poff[SN_MAX];                 // offset of the layer's W^T u partials in the workspace
    int bstart[SN_MAX + 1];            // first block of each layer (sn_wtu, sn_wv, sn_dot / sn_bwd: per launch)
    int L;
};

__device__ inline int layer_of(const SnTab &t, int b)
{
    int l = 0;
    while (l + 1 < t.L && b >= t.bstart[l + 1]) ++l;
    return l;
}

// block b of layer l = (row chunk rc, column block cb): part[rc][k] = sum over the chunk's rows of W[r][k] u[r]
__global__ __launch_bounds__(256) void sn_wtu_kernel(const SnTab t, float *__restrict__ part)
{
    const int l = layer_of(t, blockIdx.x), b = blockIdx.x - t.bstart[l];
    const int R = t.rows[l], K = t.cols[l];
    const int ncb = (K + 255) / 256;
    const int rc = b / ncb, k = (b % ncb) * 256 + threadIdx.x;
    if (k >= K) return;
    const float *w = t.w[l], *u = t.u[l];
    const int r0 = rc * SN_RC, r1 = min(r0 + SN_RC, R);
    float acc = 0.f;
    for (int r = r0; r < r1; ++r) acc += w[(long)r * K + k] * u[r];
    part[t.poff[l] + (long)rc * K + k] = acc;
}

// one block per layer: t[k] = sum_rc part[rc][k] in order; v = t / max(|t|, eps) -> live v and snap_v
__global__ __launch_bounds__(256) void sn_v_kernel(const SnTab t, const float *__restrict__ part, float *__restrict__ snap_v, float eps)
{
    __shared__ float red[256];
    const int l = blockIdx.x;
    const int R = t.rows[l], K = t.cols[l], nrc = (R + SN_RC - 1) / SN_RC;
    const float *p = part + t.poff[l];
    float ss = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
        float tk = 0.f;
        for (int rc = 0; rc < nrc; ++rc) tk += p[(long)rc * K + k];
        ss += tk * tk;
    }
    const float inv = 1.f / fmaxf(sqrtf(mrefsr::block_sum<256>(red, ss)), eps);
    float *v = t.v[l], *sv = snap_v + t.voff[l];
    for (int k = threadIdx.x; k < K; k += 256) {
        float tk = 0.f;
        for (int rc = 0; rc < nrc; ++rc) tk += p[(long)rc * K + k];
        const float vk = tk * inv;
        v[k] = vk;
        sv[k] = vk;
    }
}

// one block per (layer, row): s[r] = sum_k W[r][k] v[k] (v = snap_v in training mode, the live v in eval mode)
__global__ __launch_bounds__(256) void sn_wv_kernel(const SnTab t, const float *__restrict__ snap_v, int use_snap, float *__restrict__ s)
{
    __shared__ float red[256];
    const int l = layer_of(t, blockIdx.x), r = blockIdx.x - t.bstart[l];
    const int K = t.cols[l];
    const float *w = t.w[l] + (long)r * K, *v = use_snap ? snap_v + t.voff[l] : t.v[l];
    float acc = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) acc += w[k] * v[k];
    const float sr = mrefsr::block_sum<256>(red, acc);
    if (threadIdx.x == 0) s[t.uoff[l] + r] = sr;
}

// one block per layer: update: u = s / max(|s|, eps) -> live u and snap_u; else snap_u = u, snap_v = v.  sigma = snap_u . s
__global__ __launch_bounds__(256) void sn_u_kernel(const SnTab t, const float *__restrict__ s, float *__restrict__ snap_u, float *__restrict__ snap_v,
                                                   float *__restrict__ sigma, int update, float eps)
{
    __shared__ float red[256];
    const int l = blockIdx.x;
    const int R = t.rows[l], K = t.cols[l];
    const float *sl = s + t.uoff[l];
    float *su = snap_u + t.uoff[l];
    if (update) {
        float ss = 0.f;
        for (int r = threadIdx.x; r < R; r += 256) ss += sl[r] * sl[r];
        const float inv = 1.f / fmaxf(sqrtf(mrefsr::block_sum<256>(red, ss)), eps);
        for (int r = threadIdx.x; r < R; r += 256) {
            const float ur = sl[r] * inv;
            t.u[l][r] = ur;
            su[r] = ur;
        }
    } else {
        for (int r = threadIdx.x; r < R; r += 256) su[r] = t.u[l][r];
        for (int k = threadIdx.x; k < K; k += 256) snap_v[t.voff[l] + k] = t.v[l][k];
    }
    float d = 0.f;
    for (int r = threadIdx.x; r < R; r += 256) d += su[r] * sl[r];   // (each thread reads back its own writes)
    const float sg = mrefsr::block_sum<256>(red, d);
    if (threadIdx.x == 0) sigma[l] = sg;
}

// W[l][i] = W_orig[l][i] / sigma[l]; blocks of 256 elements, numbered per layer
__global__ __launch_bounds__(256) void sn_scale_kernel(const SnTab t, const float *__restrict__ sigma)
{
    const int l = layer_of(t, blockIdx.x);
    const long i = (long)(blockIdx.x - t.bstart[l]) * 256 + threadIdx.x;
    if (i < (long)t.rows[l] * t.cols[l]) t.o[l][i] = t.w[l][i] / sigma[l];
}

// partial <G, W_orig> of chunk c of layer l (SN_CH elements, a fixed tree)
__global__ __launch_bounds__(256) void sn_dot_kernel(const SnTab t, float *__restrict__ part)
{
    __shared__ float red[256];
    const int l = layer_of(t, blockIdx.x), c = blockIdx.x - t.bstart[l];
    const long n = (long)t.rows[l] * t.cols[l];
    const long i0 = (long)c * SN_CH, i1 = i0 + SN_CH < n ? i0 + SN_CH : n;
    const float *w = t.w[l], *gl = t.g[l];
    float acc = 0.f;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) acc += gl[i] * w[i];
    const float sc = mrefsr::block_sum<256>(red, acc);
    if (threadIdx.x == 0) part[blockIdx.x] = sc;
}

// dW_orig = G / sigma + c u v^T with c = -<G, W_orig> / sigma^2; each block sums its layer's chunk dots in order (thread 0)
__global__ __launch_bounds__(256) void sn_bwd_kernel(const SnTab t, const float *__restrict__ part, const float *__restrict__ snap_u,
                                                     const float *__restrict__ snap_v, const float *__restrict__ sigma)
{
    __shared__ float coef;
    const int l = layer_of(t, blockIdx.x), c = blockIdx.x - t.bstart[l];
    const long n = (long)t.rows[l] * t.cols[l];
    const int nch = t.bstart[l + 1] - t.bstart[l];
    const float sg = sigma[l];
    if (threadIdx.x == 0) {
        float d = 0.f;
        for (int j = 0; j < nch; ++j) d += part[t.bstart[l] + j];
        coef = -d / (sg * sg);
    }
    __syncthreads();
    const int K = t.cols[l];
    const float *gl = t.g[l], *u = snap_u + t.uoff[l], *v = snap_v + t.voff[l];
    float *dw = t.o[l];
    const long i0 = (long)c * SN_CH, i1 = i0 + SN_CH < n ? i0 + SN_CH : n;
    const float cf = coef;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) {
        const long r = i / K, k = i - r * K;
        dw[i] = gl[i] / sg + cf * u[r] * v[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// bilinear x2, align_corners False (torch's upsample_bilinear2d): output row o of an n-row input reads rows (i0, i1) with weights
// (1 - l, l):  o = 0: (0, min(1, n - 1), l 0);  o = 2k, k >= 1: (k - 1, k, l 0.75);  o = 2k + 1: (k, min(k + 1, n - 1), l 0.25).
// Adjoint: input row i is read by o = 2i - 1 (0.25, i >= 1), 2i (0.75; 1 for i = 0), 2i + 1 (0.75; 1 for i = n - 1), 2i + 2 (0.25,
// i <= n - 2); the 2-D weights are products of the row and column ones.
// ---------------------------------------------------------------------------------------------------------------
__device__ inline void up_src(int o, int n, int &i0, int &i1, float &l)
{
    const int k = o >> 1;
    if (o & 1) i0 = k, i1 = k < n - 1 ? k + 1 : k, l = 0.25f;
    else if (k == 0) i0 = 0, i1 = n > 1 ? 1 : 0, l = 0.f;
    else i0 = k - 1, i1 = k, l = 0.75f;
}

__device__ inline int up_adj_taps(int i, int n, int *o, float *wt)
{
    int m = 0;
    if (i >= 1) o[m] = 2 * i - 1, wt[m++] = 0.25f;
    o[m] = 2 * i, wt[m++] = i == 0 ? 1.f : 0.75f;
    o[m] = 2 * i + 1, wt[m++] = i == n - 1 ? 1.f : 0.75f;
    if (i <= n - 2) o[m] = 2 * i + 2, wt[m++] = 0.25f;
    return m;
}

__device__ inline float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ inline float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline float4 lerp4(float4 a, float4 b, float w0, float w1)
{
    return make_float4(w0 * a.x + w1 * b.x, w0 * a.y + w1 * b.y, w0 * a.z + w1 * b.z, w0 * a.w + w1 * b.w);
}

// one thread per output float4: out [N][2h][2w][C] = up(y + skip) (skip may be NULL)
__global__ __launch_bounds__(256) void up2_kernel(const float *__restrict__ y, const float *__restrict__ skip, float *__restrict__ out, int N, int h,
                                                  int w, int C)
{
    const int C4 = C >> 2, H2 = 2 * h, W2 = 2 * w;
    const long total = (long)N * H2 * W2 * C4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        long r = i / C4;
        const int ox = (int)(r % W2);
        r /= W2;
        const int oy = (int)(r % H2);
        const int n = (int)(r / H2);
        int y0, y1, x0, x1;
        float ly, lx;
        up_src(oy, h, y0, y1, ly);
        up_src(ox, w, x0, x1, lx);
        const long base = (long)n * h * w * C, c = 4L * c4;
        const long o00 = base + ((long)y0 * w + x0) * C + c, o01 = base + ((long)y0 * w + x1) * C + c;
        const long o10 = base + ((long)y1 * w + x0) * C + c, o11 = base + ((long)y1 * w + x1) * C + c;
        float4 v00 = ld4(y + o00), v01 = ld4(y + o01), v10 = ld4(y + o10), v11 = ld4(y + o11);
        if (skip) v00 = add4(v00, ld4(skip + o00)), v01 = add4(v01, ld4(skip + o01)), v10 = add4(v10, ld4(skip + o10)), v11 = add4(v11, ld4(skip + o11));
        const float4 a = lerp4(v00, v01, 1.f - lx, lx), b = lerp4(v10, v11, 1.f - lx, lx);
        *reinterpret_cast<float4 *>(out + i * 4) = lerp4(a, b, 1.f - ly, ly);
    }
}

// one thread per input float4: out [N][h][w][C] = the adjoint of up2 applied to g [N][2h][2w][C] (a gather over <= 4 x 4 taps)
__global__ __launch_bounds__(256) void up2_adj_kernel(const float *__restrict__ g, float *__restrict__ out, int N, int h, int w, int C)
{
    const int C4 = C >> 2, H2 = 2 * h, W2 = 2 * w;
    const long total = (long)N * h * w * C4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        long r = i / C4;
        const int ix = (int)(r % w);
        r /= w;
        const int iy = (int)(r % h);
        const int n = (int)(r / h);
        int oy[4], ox[4];
        float wy[4], wx[4];
        const int my = up_adj_taps(iy, h, oy, wy), mx = up_adj_taps(ix, w, ox, wx);
        const float *gb = g + (long)n * H2 * W2 * C + 4L * c4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int a = 0; a < my; ++a) {
            float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int b = 0; b < mx; ++b) {
                const float4 v = ld4(gb + ((long)oy[a] * W2 + ox[b]) * C);
                row = make_float4(row.x + wx[b] * v.x, row.y + wx[b] * v.y, row.z + wx[b] * v.z, row.w + wx[b] * v.w);
            }
            acc = make_float4(acc.x + wy[a] * row.x, acc.y + wy[a] * row.y, acc.z + wy[a] * row.z, acc.w + wy[a] * row.w);
        }
        *reinterpret_cast<float4 *>(out + i * 4) = acc;
    }
}

__global__ __launch_bounds__(256) void add_kernel(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ out, long n)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = a[i] + b[i];
}

// ---------------------------------------------------------------------------------------------------------------
// conv9: nn.Conv2d(C, 1, 3, 1, 1) on x [N][H][W][C]; w in torch's [1][C][3][3] layout, staged in LDS as ws[tap][C].
// Forward: a 16-lane group per output pixel, lane j over the channel quads j, j + 16, ..; the 16 partial sums are added by a fixed
// xor butterfly.  Input gradient: one thread per (pixel, quad), 9 taps.  Weight gradient: a block per (pixel chunk, 16 quads): 16
// pixel slots x 16 lanes, each lane 9 x 4 sums over its slot's pixels, the slots added in order through LDS; the chunks in order by
// conv9_wgrad_finish.
// ---------------------------------------------------------------------------------------------------------------
constexpr int C9_MAXC = 512;
constexpr int C9_PIX = 256;   // pixels per wgrad chunk (at least)

__device__ inline void stage_w9(const float *__restrict__ w, float *ws, int C)
{
    for (int i = threadIdx.x; i < 9 * C; i += blockDim.x) {
        const int c = i % C, tap = i / C;
        ws[i] = w[c * 9 + tap];
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void conv9_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                                                        float *__restrict__ y, int N, int H, int W, int C)
{
    __shared__ __attribute__((aligned(16))) float ws[9 * C9_MAXC];
    stage_w9(w, ws, C);
    const int C4 = C >> 2, j = threadIdx.x & 15;
    const long P = (long)N * H * W;
    const long groups = (long)gridDim.x * 16;
    // (the 16 lanes of a group share p: the butterfly below stays inside lanes that run the same iterations)
    for (long p = blockIdx.x * 16L + (threadIdx.x >> 4); p < P; p += groups) {
        float acc = 0.f;
        {
            const int px = (int)(p % W);
            const long r = p / W;
            const int py = (int)(r % H);
            const long nb = (r / H) * H;
            for (int ky = 0; ky < 3; ++ky) {
                const int sy = py + ky - 1;
                if (sy < 0 || sy >= H) continue;
                for (int kx = 0; kx < 3; ++kx) {
                    const int sx = px + kx - 1;
                    if (sx < 0 || sx >= W) continue;
                    const float *xs = x + ((nb + sy) * W + sx) * C;
                    const float *wt = ws + (ky * 3 + kx) * C;
                    for (int q = j; q < C4; q += 16) {
                        const float4 a = ld4(xs + 4 * q), b = *reinterpret_cast<const float4 *>(wt + 4 * q);
                        acc += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
                    }
                }
            }
        }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 16);
        if (j == 0) y[p] = bias ? acc + bias[0] : acc;
    }
}

// dx[q][c] = sum over (ky, kx) of w[c][ky][kx] gy[q - (ky - 1, kx - 1)]
__global__ __launch_bounds__(256) void conv9_dgrad_kernel(const float *__restrict__ gy, const float *__restrict__ w, float *__restrict__ dx, int N,
                                                          int H, int W, int C)
{
    __shared__ __attribute__((aligned(16))) float ws[9 * C9_MAXC];
    stage_w9(w, ws, C);
    const int C4 = C >> 2;
    const long total = (long)N * H * W * C4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int q = (int)(i % C4);
        const long p = i / C4;
        const int px = (int)(p % W);
        const long r = p / W;
        const int py = (int)(r % H);
        const long nb = (r / H) * H;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int ky = 0; ky < 3; ++ky) {
            const int sy = py - ky + 1;
            if (sy < 0 || sy >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int sx = px - kx + 1;
                if (sx < 0 || sx >= W) continue;
                const float g = gy[(nb + sy) * W + sx];
                const float4 b = *reinterpret_cast<const float4 *>(ws + (ky * 3 + kx) * C + 4 * q);
                acc = make_float4(acc.x + b.x * g, acc.y + b.y * g, acc.z + b.z * g, acc.w + b.w * g);
            }
        }
        *reinterpret_cast<float4 *>(dx + i * 4) = acc;
    }
}

// block (chunk, qg): pixels [chunk PB, (chunk + 1) PB), quads 16 qg + lane; part[chunk][tap][C]
__global__ __launch_bounds__(256) void conv9_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ gy, float *__restrict__ part, int N,
                                                          int H, int W, int C, int PB)
{
    __shared__ float red[16][16][37];   // [slot][lane][9 x 4] (pitch 37: spread banks)
    const int slot = threadIdx.x >> 4, j = threadIdx.x & 15;
    const int q = blockIdx.y * 16 + j;
    const int C4 = C >> 2;
    const long P = (long)N * H * W;
    const long p0 = (long)blockIdx.x * PB, p1 = p0 + PB < P ? p0 + PB : P;
    float acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t][0] = acc[t][1] = acc[t][2] = acc[t][3] = 0.f;
    if (q < C4) {
        for (long p = p0 + slot; p < p1; p += 16) {
            const float g = gy[p];
            const int px = (int)(p % W);
            const long r = p / W;
            const int py = (int)(r % H);
            const long nb = (r / H) * H;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int sy = py + ky - 1;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int sx = px + kx - 1;
                    if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
                        const float4 a = ld4(x + ((nb + sy) * W + sx) * C + 4 * q);
                        acc[ky * 3 + kx][0] += a.x * g, acc[ky * 3 + kx][1] += a.y * g;
                        acc[ky * 3 + kx][2] += a.z * g, acc[ky * 3 + kx][3] += a.w * g;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[slot][j][t * 4 + e] = acc[t][e];
    __syncthreads();
    // 16 lanes x 36 sums, each over the 16 slots in order
    for (int o = threadIdx.x; o < 16 * 36; o += 256) {
        const int lj = o / 36, te = o % 36;
        const int qq = blockIdx.y * 16 + lj;
        if (qq >= C4) continue;
        float s = 0.f;
        for (int sl = 0; sl < 16; ++sl) s += red[sl][lj][te];
        const int tap = te >> 2, c = 4 * qq + (te & 3);
        part[((long)blockIdx.x * 9 + tap) * C + c] = s;
    }
}

// dw[c][tap] = sum over the chunks in order of part[chunk][tap][c]
__global__ __launch_bounds__(256) void conv9_wgrad_finish_kernel(const float *__restrict__ part, float *__restrict__ dw, int C, int nch)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 9 * C) return;
    const int c = i / 9, tap = i % 9;
    float s = 0.f;
    for (int k = 0; k < nch; ++k) s += part[((long)k * 9 + tap) * C + c];
    dw[i] = s;
}

// ------------------------------------------------------------------------------------------------- host side
int sn_table(SnTab &t, const float *const *w, float *const *u, float *const *v, const int *rows, const int *cols, int L)
{
    if (L < 1 || L > SN_MAX) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "disc_sn: %d layers (1 .. %d)", L, SN_MAX);
    t = SnTab{};
    t.L = L;
    long uo = 0, vo = 0, po = 0;
    for (int l = 0; l < L; ++l) {
        if (!w[l] || (u && !u[l]) || (v && !v[l])) return mrefsr::fail(MREFSR_E_INVALID, "disc_sn: null pointer of layer %d", l);
        if (rows[l] <= 0 || cols[l] <= 0) return mrefsr::fail(MREFSR_E_INVALID, "disc_sn: layer %d is %d x %d", l, rows[l], cols[l]);
        if ((long)rows[l] * cols[l] > (1L << 30)) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "disc_sn: layer %d too large", l);
        t.w[l] = w[l], t.u[l] = u ? u[l] : nullptr, t.v[l] = v ? v[l] : nullptr;
        t.rows[l] = rows[l], t.cols[l] = cols[l];
        t.uoff[l] = uo, t.voff[l] = vo, t.poff[l] = po;
        uo += rows[l], vo += cols[l];
        po += (long)((rows[l] + SN_RC - 1) / SN_RC) * cols[l];
    }
    return MREFSR_OK;
}

long sn_part_floats(const SnTab &t)
{
    const int l = t.L - 1;
    return t.poff[l] + (long)((t.rows[l] + SN_RC - 1) / SN_RC) * t.cols[l];
}

long sn_rows_total(const SnTab &t) { return t.uoff[t.L - 1] + t.rows[t.L - 1]; }

// bstart for blocks of `per(l)` each; returns the total
template <class F>
int sn_blocks(SnTab &t, F per)
{
    int b = 0;
    for (int l = 0; l < t.L; ++l) t.bstart[l] = b, b += per(l);
    t.bstart[t.L] = b;
    return b;
}

int check_c9(const char *what, int N, int H, int W, int C)
{
    if (N <= 0 || H <= 0 || W <= 0) return mrefsr::fail(MREFSR_E_INVALID, "%s: N=%d H=%d W=%d", what, N, H, W);
    if (C <= 0 || C % 4 || C > C9_MAXC) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: C=%d (a multiple of 4, at most %d)", what, C, C9_MAXC);
    return MREFSR_OK;
}

int c9_chunk(long P, int &nch)
{
    long pb = (P + 511) / 512;
    if (pb < C9_PIX) pb = C9_PIX;
    pb = (pb + 15) / 16 * 16;
    nch = (int)((P + pb - 1) / pb);
    return (int)pb;
}

}  // namespace

MREFSR_EXPORT int64_t mrefsr_disc_sn_workspace_bytes(const int *rows, const int *cols, int L)
{
    if (!rows || !cols || L < 1 || L > SN_MAX) return -1;
    const float *w[SN_MAX];
    for (int l = 0; l < L; ++l) w[l] = (const float *)1;   // (only the geometry is read)
    SnTab t;
    if (sn_table(t, w, nullptr, nullptr, rows, cols, L)) return -1;
    return (int64_t)(sn_part_floats(t) + sn_rows_total(t)) * 4;
}

MREFSR_EXPORT int mrefsr_disc_sn_power_f32(const float *const *w, float *const *u, float *const *v, const int *rows, const int *cols, int L, int update,
                                           float eps, float *snap_u, float *snap_v, float *sigma, void *workspace, int64_t workspace_bytes,
                                           mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(w && u && v && rows && cols && snap_u && snap_v && sigma && workspace, "disc_sn_power: null pointer");
    SnTab t;
    int rc = sn_table(t, w, u, v, rows, cols, L);
    if (rc) return rc;
    const int64_t need = mrefsr_disc_sn_workspace_bytes(rows, cols, L);
    MREFSR_REQUIRE(workspace_bytes >= need, "disc_sn_power: workspace of %ld bytes < %ld", (long)workspace_bytes, (long)need);
    hipStream_t st = (hipStream_t)stream;
    float *part = (float *)workspace, *s = part + sn_part_floats(t);
    if (update) {
        const int nb = sn_blocks(t, [&](int l) { return ((t.rows[l] + SN_RC - 1) / SN_RC) * ((t.cols[l] + 255) / 256); });
        hipLaunchKernelGGL(sn_wtu_kernel, dim3(nb), dim3(256), 0, st, t, part);
        hipLaunchKernelGGL(sn_v_kernel, dim3(L), dim3(256), 0, st, t, (const float *)part, snap_v, eps);
    }
    const int nb = sn_blocks(t, [&](int l) { return t.rows[l]; });
    hipLaunchKernelGGL(sn_wv_kernel, dim3(nb), dim3(256), 0, st, t, (const float *)snap_v, update ? 1 : 0, s);
    hipLaunchKernelGGL(sn_u_kernel, dim3(L), dim3(256), 0, st, t, (const float *)s, snap_u, snap_v, sigma, update ? 1 : 0, eps);
    return mrefsr::check_launch("disc_sn_power");
}

MREFSR_EXPORT int mrefsr_disc_sn_scale_f32(const float *const *w_orig, float *const *w, const int *rows, const int *cols, int L, const float *sigma,
                                           mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(w_orig && w && rows && cols && sigma, "disc_sn_scale: null pointer");
    SnTab t;
    int rc = sn_table(t, w_orig, nullptr, nullptr, rows, cols, L);
    if (rc) return rc;
    for (int l = 0; l < L; ++l) {
        MREFSR_REQUIRE(w[l], "disc_sn_scale: null output of layer %d", l);
        t.o[l] = w[l];
    }
    const int nb = sn_blocks(t, [&](int l) { return (int)(((long)t.rows[l] * t.cols[l] + 255) / 256); });
    hipLaunchKernelGGL(sn_scale_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, t, sigma);
    return mrefsr::check_launch("disc_sn_scale");
}

MREFSR_EXPORT int64_t mrefsr_disc_sn_bwd_workspace_bytes(const int *rows, const int *cols, int L)
{
    if (!rows || !cols || L < 1 || L > SN_MAX) return -1;
    long n = 0;
    for (int l = 0; l < L; ++l) {
        if (rows[l] <= 0 || cols[l] <= 0) return -1;
        n += ((long)rows[l] * cols[l] + SN_CH - 1) / SN_CH;
    }
    return (int64_t)n * 4;
}

MREFSR_EXPORT int mrefsr_disc_sn_bwd_f32(const float *const *g, const float *const *w_orig, float *const *dw, const int *rows, const int *cols, int L,
                                         const float *snap_u, const float *snap_v, const float *sigma, void *workspace, int64_t workspace_bytes,
                                         mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(g && w_orig && dw && rows && cols && snap_u && snap_v && sigma && workspace, "disc_sn_bwd: null pointer");
    SnTab t;
    int rc = sn_table(t, w_orig, nullptr, nullptr, rows, cols, L);
    if (rc) return rc;
    for (int l = 0; l < L; ++l) {
        MREFSR_REQUIRE(g[l] && dw[l], "disc_sn_bwd: null gradient of layer %d", l);
        t.g[l] = g[l], t.o[l] = dw[l];
    }
    const int64_t need = mrefsr_disc_sn_bwd_workspace_bytes(rows, cols, L);
    MREFSR_REQUIRE(workspace_bytes >= need, "disc_sn_bwd: workspace of %ld bytes < %ld", (long)workspace_bytes, (long)need);
    const int nb = sn_blocks(t, [&](int l) { return (int)(((long)t.rows[l] * t.cols[l] + SN_CH - 1) / SN_CH); });
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sn_dot_kernel, dim3(nb), dim3(256), 0, st, t, (float *)workspace);
    hipLaunchKernelGGL(sn_bwd_kernel, dim3(nb), dim3(256), 0, st, t, (const float *)workspace, snap_u, snap_v, sigma);
    return mrefsr::check_launch("disc_sn_bwd");
}

MREFSR_EXPORT int mrefsr_disc_up2_f32(const float *y, const float *skip, float *out, int N, int h, int w, int C, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(y && out, "disc_up2: null pointer");
    MREFSR_REQUIRE(N > 0 && h > 0 && w > 0 && C > 0 && C % 4 == 0, "disc_up2: N=%d h=%d w=%d C=%d (C a multiple of 4)", N, h, w, C);
    const long total = (long)N * 4 * h * w * (C / 4);
    hipLaunchKernelGGL(up2_kernel, dim3(grid_of((total + 255) / 256, 16384)), dim3(256), 0, (hipStream_t)stream, y, skip, out, N, h, w, C);
    return mrefsr::check_launch("disc_up2");
}

MREFSR_EXPORT int mrefsr_disc_up2_adj_f32(const float *g, float *out, int N, int h, int w, int C, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(g && out, "disc_up2_adj: null pointer");
    MREFSR_REQUIRE(N > 0 && h > 0 && w > 0 && C > 0 && C % 4 == 0, "disc_up2_adj: N=%d h=%d w=%d C=%d (C a multiple of 4)", N, h, w, C);
    const long total = (long)N * h * w * (C / 4);
    hipLaunchKernelGGL(up2_adj_kernel, dim3(grid_of((total + 255) / 256, 16384)), dim3(256), 0, (hipStream_t)stream, g, out, N, h, w, C);
    return mrefsr::check_launch("disc_up2_adj");
}

MREFSR_EXPORT int mrefsr_disc_add_f32(const float *a, const float *b, float *out, int64_t n, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(a && b && out && n > 0, "disc_add: null pointer or n=%ld", (long)n);
    hipLaunchKernelGGL(add_kernel, dim3(grid_of((n + 255) / 256, 16384)), dim3(256), 0, (hipStream_t)stream, a, b, out, (long)n);
    return mrefsr::check_launch("disc_add");
}

MREFSR_EXPORT int mrefsr_disc_conv9_f32(const float *x, const float *w, const float *bias, float *y, int N, int H, int W, int C, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && w && y, "disc_conv9: null pointer");
    int rc = check_c9("disc_conv9", N, H, W, C);
    if (rc) return rc;
    const long P = (long)N * H * W;
    hipLaunchKernelGGL(conv9_fwd_kernel, dim3(grid_of((P + 15) / 16, 8192)), dim3(256), 0, (hipStream_t)stream, x, w, bias, y, N, H, W, C);
    return mrefsr::check_launch("disc_conv9");
}

MREFSR_EXPORT int mrefsr_disc_conv9_dgrad_f32(const float *gy, const float *w, float *dx, int N, int H, int W, int C, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(gy && w && dx, "disc_conv9_dgrad: null pointer");
    int rc = check_c9("disc_conv9_dgrad", N, H, W, C);
    if (rc) return rc;
    const long total = (long)N * H * W * (C / 4);
    hipLaunchKernelGGL(conv9_dgrad_kernel, dim3(grid_of((total + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)stream, gy, w, dx, N, H, W, C);
    return mrefsr::check_launch("disc_conv9_dgrad");
}

MREFSR_EXPORT int64_t mrefsr_disc_conv9_wgrad_workspace_bytes(int N, int H, int W, int C)
{
    if (check_c9("disc_conv9_wgrad_workspace_bytes", N, H, W, C)) return -1;
    int nch;
    c9_chunk((long)N * H * W, nch);
    return (int64_t)nch * 9 * C * 4;
}

MREFSR_EXPORT int mrefsr_disc_conv9_wgrad_f32(const float *x, const float *gy, float *dw, int N, int H, int W, int C, void *workspace,
                                              int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && gy && dw && workspace, "disc_conv9_wgrad: null pointer");
    int rc = check_c9("disc_conv9_wgrad", N, H, W, C);
    if (rc) return rc;
    const int64_t need = mrefsr_disc_conv9_wgrad_workspace_bytes(N, H, W, C);
    MREFSR_REQUIRE(workspace_bytes >= need, "disc_conv9_wgrad: workspace of %ld bytes < %ld", (long)workspace_bytes, (long)need);
    int nch;
    const int pb = c9_chunk((long)N * H * W, nch);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(conv9_wgrad_kernel, dim3(nch, (C / 4 + 15) / 16), dim3(256), 0, st, x, gy, (float *)workspace, N, H, W, C, pb);
    hipLaunchKernelGGL(conv9_wgrad_finish_kernel, dim3((9 * C + 255) / 256), dim3(256), 0, st, (const float *)workspace, dw, C, nch);
    return mrefsr::check_launch("disc_conv9_wgrad");
}
