// The multi-scale SSIM loss of the training step (train.msssim_opt, losses.MSSSIMLoss) and the MS-SSIM of validation (val.msssim):
// Wang, Simoncelli, Bovik, "Multi-scale structural similarity for image quality assessment" (Asilomar 2003), with the window and the
// constants of the validation metric at every level (11 taps, sigma 1.5, valid region, C1 = (0.01 255)^2, C2 = (0.03 255)^2), in fp32
// on the unquantised, unclamped images, and its gradient towards pred.  losses.msssim_loss_torch spells the definition out.
//
// Planes as in ssim_loss.hip: 'y' mode, one per image, X = 65.481 R + 128.553 G + 24.966 B + 16; 'rgb' mode, three per image,
// X = 255 x.  Level 1 is the plane, level j + 1 the 2 x 2 mean of level j with stride 2 (a trailing odd row or column is dropped):
// H_j = H >> (j - 1), and H_M, W_M >= 11.  Per plane p: F_{p,j} = mean cs over level j's (H_j - 10) x (W_j - 10) map for j < M,
// F_{p,M} = mean l cs; v_p = prod_j F_{p,j}^{w_j} when every F_{p,j} > 0, otherwise v_p = 0 WITH GRADIENT 0 (the zero rule);
// loss = loss_weight (1 - mean_p v_p).
//
// Memory.  A pyramid holds the levels one behind the other, level j as [planes][H_j][W_j]; `pyramid` is pred's, then target's.  A
// map set holds level j as [planes][H_j - 10][W_j - 10]; `maps` is the sets a, b, c.  Both survive the forward for the backward.
//
// Forward, three launches.
//   1. pyramid: block (tx, ty, plane) owns the 32 x 32 level-1 pixels from (32 ty, 32 tx) of pred and of target and every pooled
//      pixel under them (level j: (32 >> (j - 1))^2 of them; 32 is a multiple of 2^4, so a pooled pixel never straddles two blocks).
//      Pooling: 0.25 ((p00 + p01) + (p10 + p11)) in fp32.
//   2. statistics, all levels in one grid: block (level, plane, ty, tx) owns 16 x 32 map positions and runs the forward tile body
//      of ssim_window.h (moments_tile) on the level's planes: the window moments from pixels staged MINUS a per-tile reference
//      value, so that sigma^2 does not cancel at 255 scale -- the coarse levels are smooth.  Per position cs = A2 / B2 (levels
//      j < M) or l cs (level M), and, when a gradient is wanted, the coefficients at fixed RAW second moments
//          j < M:  a = d cs/d mu_x = 2 (mu_x cs - mu_y) / B2,  b = d cs/d E[x^2] = -cs / B2,  c = d cs/d E[xy] = 2 / B2
//          j = M:  the a, b, c of ssim_window.h's ssim_terms (m = l cs)
//      with A2 = 2 sigma_xy + C2, B2 = sigma_x^2 + sigma_y^2 + C2.  Sum: per thread position k = 0 then 1, the 256 threads by the
//      LDS tree of reduce.h, one fp32 partial per block.
//   3. combine, one block: the partials of each (plane, level), which are adjacent, in double: lane l of a wave adds partials
//      l, l + 64, .. in ascending order, then wave_sum; F = sum / count_j.  Per plane v_p = exp(sum_j w_j log F_{p,j}) or the zero
//      rule, the multipliers mult[p][j] = w_j v_p / F_{p,j} / count_j (0 under the zero rule) in double, rounded to fp32; the mean of
//      v: thread t adds planes t, t + 256, .. in ascending order, then the tree; loss = fl32(loss_weight (1 - sum / planes)).
//   No float atomics, no ticket, no readback: the same bits from call to call.
//
// Backward, two launches (one when M = 1).  Level j's own term is g_j = mult[p][j] (G^T a + 2 X_j G^T b + Y_j G^T c), G^T the same
// window over the maps zero-extended by 10 (adjoint_tile; exactly 0 where mult is 0, whatever the maps hold); level j's plane gradient is
// d_j = g_j + d_{j+1}(y >> 1, x >> 1) / 4 inside the pooled region.  Because H_{j+1} = H_j >> 1, a level-1 pixel lies in level j's
// pooled region exactly when (y >> (j - 1)) < H_j and (x >> (j - 1)) < W_j, and then in every finer one, so the recursion needs no
// intermediate planes:
//   1. own terms of the levels 2 .. M in one grid (16 x 32 pixels per block) into the workspace;
//   2. level 1: its own term plus the coarse levels by the recursion's own order, t = g_M; t = g_j + t / 4 for j = M - 1 .. 2;
//      d_1 = g_1 + t / 4; times (-loss_weight / planes) grad_loss[0] (read from the device), mapped back to R, G, B: every element of
//      grad_pred is written exactly once.
#include "common.h"
#include "ssim_window.h"

namespace {

using namespace mrefsr::ssim;

constexpr int PT = 32;                          // level-1 pixels per side of a pyramid block
constexpr int MAXL = MREFSR_MSSSIM_MAX_LEVELS;

// the geometry of one call, passed to every kernel by value (level index j = 0 .. levels - 1 is the text's level j + 1)
struct Pyr {
    int levels, planes;
    int h[MAXL], w[MAXL];
    long pix[MAXL + 1];    // floats in front of level j in a pyramid; pix[levels] = one pyramid
    long map[MAXL + 1];    // floats in front of level j in a map set; map[levels] = one set
    int ftx[MAXL], fty[MAXL];   // forward tiles of a plane's map
    long fblk[MAXL + 1];   // forward blocks in front of level j (plane-major inside a level); fblk[levels] = the grid
    int btx[MAXL], bty[MAXL];   // backward tiles of a plane
    long bblk[MAXL + 1];   // backward blocks of the levels 1 .. levels - 1 in front of level j (bblk[0] = bblk[1] = 0)
    double w8[MAXL];       // the weights
};

bool shape_ok(const int batch, const int h, const int w, const int levels)
{
    // (3 batch and the tiles of a plane within the grid's 65535; a plane's pixel count in 31 bits; every level at least the window)
    return levels >= 1 && levels <= MAXL && batch > 0 && batch <= 21845 && h <= (1 << 19) && w <= (1 << 19) &&
           (int64_t)h * w <= ((int64_t)1 << 30) && (h >> (levels - 1)) >= TAPS && (w >> (levels - 1)) >= TAPS;
}

// false for a shape outside the limits (then `g` is not to be used)
bool geometry(const int batch, const int h, const int w, const int rgb, const int levels, Pyr &g)
{
    if (!shape_ok(batch, h, w, levels)) return false;
    g = Pyr{};
    g.levels = levels, g.planes = (rgb ? 3 : 1) * batch;
    for (int j = 0; j < levels; ++j) {
        g.h[j] = h >> j, g.w[j] = w >> j;
        g.ftx[j] = mrefsr::cdiv(g.w[j] - HALO, TW), g.fty[j] = mrefsr::cdiv(g.h[j] - HALO, TH);
        g.btx[j] = mrefsr::cdiv(g.w[j], TW), g.bty[j] = mrefsr::cdiv(g.h[j], TH);
        g.pix[j + 1] = g.pix[j] + (long)g.planes * g.h[j] * g.w[j];
        g.map[j + 1] = g.map[j] + (long)g.planes * (g.h[j] - HALO) * (g.w[j] - HALO);
        g.fblk[j + 1] = g.fblk[j] + (long)g.planes * g.ftx[j] * g.fty[j];
        g.bblk[j + 1] = g.bblk[j] + (j == 0 ? 0 : (long)g.planes * g.btx[j] * g.bty[j]);
    }
    return g.fblk[levels] <= ((long)1 << 30) && g.bblk[levels] <= ((long)1 << 30);
}

// forward workspace: the partials (one float per forward block), then planes x levels doubles F
int64_t fwd_partial_bytes(const Pyr &g) { return (g.fblk[g.levels] * 4 + 255) / 256 * 256; }
int64_t fwd_workspace_bytes(const Pyr &g) { return fwd_partial_bytes(g) + (int64_t)g.planes * g.levels * 8; }
// backward workspace: the own terms of the levels 2 .. M
int64_t bwd_workspace_bytes(const Pyr &g) { return (g.pix[g.levels] - g.pix[1]) * 4; }

// ---- forward 1: the planes and their pooled levels ---------------------------------------------------------------
template <bool RGB>
__global__ __launch_bounds__(THREADS) void msssim_pyramid_kernel(const float *__restrict__ pred, const float *__restrict__ target, const Pyr g,
                                                                 float *__restrict__ pyramid)
{
    __shared__ float buf[2][PT * PT];
    const int tid = threadIdx.x;
    const int H = g.h[0], W = g.w[0];
    const int y0 = blockIdx.y * PT, x0 = blockIdx.x * PT;
    const long p = blockIdx.z, hw = (long)H * W;
    for (int which = 0; which < 2; ++which) {
        const float *img = which ? target : pred;
        float *pyr = pyramid + which * g.pix[g.levels];
        __syncthreads();   // (the previous image's last level has been read)
        for (int idx = tid; idx < PT * PT; idx += THREADS) {
            const int gy = y0 + idx / PT, gx = x0 + idx % PT;
            float val = 0.f;
            if (gy < H && gx < W) {
                const long off = (long)gy * W + gx;
                val = plane_value<RGB>(img, p, hw, off);
                pyr[p * hw + off] = val;
            }
            buf[0][idx] = val;
        }
        // a pooled pixel inside level j has its four parents inside level j - 1: the zeros outside never reach a stored value
        for (int j = 1; j < g.levels; ++j) {
            __syncthreads();
            const int n = PT >> j;
            const float *src = buf[(j - 1) & 1];
            float *dst = buf[j & 1];
            for (int idx = tid; idx < n * n; idx += THREADS) {
                const int r = idx / n, c = idx % n;
                const float *q = src + (2 * r) * (2 * n) + 2 * c;
                const float val = 0.25f * ((q[0] + q[1]) + (q[2 * n] + q[2 * n + 1]));
                dst[idx] = val;
                const int gy = (y0 >> j) + r, gx = (x0 >> j) + c;
                if (gy < g.h[j] && gx < g.w[j]) pyr[g.pix[j] + (p * g.h[j] + gy) * g.w[j] + gx] = val;
            }
        }
    }
}

// ---- forward 2: the window statistics of every level ------------------------------------------------------------
template <bool WANT_GRAD>
__global__ __launch_bounds__(THREADS) void msssim_stats_kernel(const float *__restrict__ pyramid, const Pyr g, const Taps taps,
                                                               float *__restrict__ maps, float *__restrict__ partial)
{
    __shared__ float s[2 * SH * SW];        // pred | target, minus the tile's reference values
    __shared__ float v[5 * TH * SW];        // column-filtered x, y, xx, yy, xy; then the reduction tree
    const int tid = threadIdx.x;
    const long bid = blockIdx.x;
    int j = 0;
    while (j + 1 < g.levels && bid >= g.fblk[j + 1]) ++j;
    const bool last = j == g.levels - 1;
    const int H = g.h[j], W = g.w[j], MH = H - HALO, MW = W - HALO;
    const long local = bid - g.fblk[j], tiles = (long)g.ftx[j] * g.fty[j];
    const long p = local / tiles;
    const int t = (int)(local % tiles);
    const int y0 = (t / g.ftx[j]) * TH, x0 = (t % g.ftx[j]) * TW;
    const float *X = pyramid + g.pix[j] + p * H * W, *Y = X + g.pix[g.levels];

    float fsum = 0.f;
    moments_tile(
        s, v, taps, H, W, y0, x0, [&](const long off, float &xv, float &yv) { xv = X[off], yv = Y[off]; },
        [&](const int my, const int mx, const Moments &q) {
            // (in front of the test and the branches: there the compiler shares A2 and 1 / B2 with ssim_terms, one division per position
            // for either kind of level; behind them it emits the division a second time)
            const float a2 = 2.f * q.sxy + C2, b2 = q.sxx + q.syy + C2, ib2 = 1.f / b2;
            if (my >= MH || mx >= MW) return;
            const long o = g.map[j] + (p * MH + my) * MW + mx;
            if (last) {
                const Terms t = ssim_terms(q);
                fsum += t.m;
                if constexpr (WANT_GRAD) maps[o] = t.a, maps[g.map[g.levels] + o] = t.b, maps[2 * g.map[g.levels] + o] = t.c;
            } else {
                const float cs = a2 * ib2;
                fsum += cs;
                if constexpr (WANT_GRAD) {
                    maps[o] = 2.f * (q.mux * cs - q.muy) * ib2;
                    maps[g.map[g.levels] + o] = -cs * ib2;
                    maps[2 * g.map[g.levels] + o] = 2.f * ib2;
                }
            }
        });
    const float bsum = mrefsr::block_sum<THREADS>(v, fsum);   // (meets first: every thread has read v, it becomes the tree)
    if (tid == 0) partial[bid] = bsum;
}

// ---- forward 3: F, v, the loss and the multipliers ---------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void msssim_combine_kernel(const float *__restrict__ partial, const Pyr g, const double loss_weight,
                                                                 double *F, float *__restrict__ mult, double *__restrict__ values,
                                                                 float *__restrict__ loss)
{
    __shared__ double red[THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long pairs = (long)g.planes * g.levels;
    for (long q = wave; q < pairs; q += THREADS / 64) {
        const long p = q / g.levels;
        const int j = (int)(q % g.levels);
        const int tiles = g.ftx[j] * g.fty[j];
        const float *part = partial + g.fblk[j] + p * tiles;
        double sum = 0.0;
        for (int i = lane; i < tiles; i += 64) sum += (double)part[i];
        sum = mrefsr::wave_sum(sum);
        if (lane == 0) F[q] = sum / ((double)(g.h[j] - HALO) * (double)(g.w[j] - HALO));
    }
    __syncthreads();   // (F is this block's own: its writes are visible to the block behind the barrier)

    double vsum = 0.0;
    for (long p = tid; p < g.planes; p += THREADS) {
        bool positive = true;
        double lg = 0.0;
        for (int j = 0; j < g.levels; ++j) {
            const double f = F[p * g.levels + j];
            positive = positive && f > 0.0;       // (false for a NaN as well)
            if (positive) lg += g.w8[j] * log(f);
        }
        const double val = positive ? exp(lg) : 0.0;
        vsum += val;
        if (values) values[p] = val;
        if (mult)
            for (int j = 0; j < g.levels; ++j)
                mult[p * g.levels + j] =
                    positive ? (float)(g.w8[j] * val / F[p * g.levels + j] / ((double)(g.h[j] - HALO) * (double)(g.w[j] - HALO))) : 0.f;
    }
    const double total = mrefsr::block_sum<THREADS>(red, vsum);
    if (tid == 0) loss[0] = (float)(loss_weight * (1.0 - total / (double)g.planes));
}

// ---- backward ----------------------------------------------------------------------------------------------------
// level j's own term mult (G^T a + 2 X G^T b + Y G^T c) of plane p at the block's 16 x 32 pixels from (y0, x0), by adjoint_tile of
// ssim_window.h: emit(off, value) for the thread's pixels inside the level, off = y W + x.  s: 3 SH SW floats of LDS, v: 3 TH SW.
template <class E>
__device__ __forceinline__ void own_term(const Pyr &g, const int j, const long p, const int y0, const int x0, const float *__restrict__ pyramid,
                                         const float *__restrict__ maps, const float *__restrict__ mult, const Taps &taps, float *s, float *v,
                                         const E &emit)
{
    const int H = g.h[j], W = g.w[j], MH = H - HALO, MW = W - HALO;
    const float m = mult[p * g.levels + j];
    const float *A = maps + g.map[j] + p * MH * MW, *B = A + g.map[g.levels], *C = B + g.map[g.levels];
    const float *X = pyramid + g.pix[j] + p * H * W, *Y = X + g.pix[g.levels];
    // (the zero rule: a plane whose multiplier is 0 gets exactly 0, whatever its maps hold -- they are not even read)
    adjoint_tile(
        s, v, taps, H, W, y0, x0,
        [&](const int my, const int mx, float &av, float &bv, float &cv) {
            const long o = (long)my * MW + mx;
            if (m != 0.f) av = A[o], bv = B[o], cv = C[o];
        },
        [&](const int gy, const int gx, const float (&t)[3]) {
            const long off = (long)gy * W + gx;
            emit(off, m != 0.f ? m * (t[0] + 2.f * X[off] * t[1] + Y[off] * t[2]) : 0.f);
        });
}

__global__ __launch_bounds__(THREADS) void msssim_bwd_levels_kernel(const float *__restrict__ pyramid, const float *__restrict__ maps,
                                                                    const float *__restrict__ mult, const Pyr g, const Taps taps,
                                                                    float *__restrict__ own)
{
    __shared__ float s[3 * SH * SW];
    __shared__ float v[3 * TH * SW];
    const long bid = blockIdx.x;
    int j = 1;
    while (j + 1 < g.levels && bid >= g.bblk[j + 1]) ++j;
    const long local = bid - g.bblk[j], tiles = (long)g.btx[j] * g.bty[j];
    const long p = local / tiles;
    const int t = (int)(local % tiles);
    float *out = own + (g.pix[j] - g.pix[1]) + p * g.h[j] * g.w[j];
    own_term(g, j, p, (t / g.btx[j]) * TH, (t % g.btx[j]) * TW, pyramid, maps, mult, taps, s, v,
             [&](const long off, const float val) { out[off] = val; });
}

template <bool RGB>
__global__ __launch_bounds__(THREADS) void msssim_bwd_finish_kernel(const float *__restrict__ pyramid, const float *__restrict__ maps,
                                                                    const float *__restrict__ mult, const float *__restrict__ own,
                                                                    const float *__restrict__ gup, const Pyr g, const Taps taps,
                                                                    const float scale, float *__restrict__ grad)
{
    __shared__ float s[3 * SH * SW];
    __shared__ float v[3 * TH * SW];
    const int W = g.w[0];
    const long p = blockIdx.z, hw = (long)g.h[0] * W;
    const float f = scale * gup[0];
    own_term(g, 0, p, blockIdx.y * TH, blockIdx.x * TW, pyramid, maps, mult, taps, s, v, [&](const long off, const float g1) {
        const int y = (int)(off / W), x = (int)(off % W);
        float t = 0.f;
        for (int j = g.levels - 1; j >= 1; --j) {
            const int yy = y >> j, xx = x >> j;
            // (outside level j's pooled region the pixel is outside every coarser one: t is still 0)
            t = yy < g.h[j] && xx < g.w[j] ? own[(g.pix[j] - g.pix[1]) + (p * g.h[j] + yy) * g.w[j] + xx] + 0.25f * t : 0.f;
        }
        store_plane_grad<RGB>(grad, p, hw, off, f * (g1 + 0.25f * t));
    });
}

}  // namespace

#define MSSSIM_LIMITS "batch=%d (1..21845) h=%d w=%d (<= 2^19, h*w <= 2^30) levels=%d (1..5, min(h, w) >> (levels - 1) >= 11)"

MREFSR_EXPORT int64_t mrefsr_msssim_pyramid_floats(int batch, int h, int w, int rgb, int levels)
{
    Pyr g;
    return geometry(batch, h, w, rgb, levels, g) ? 2 * g.pix[levels] : -1;
}

MREFSR_EXPORT int64_t mrefsr_msssim_map_floats(int batch, int h, int w, int rgb, int levels)
{
    Pyr g;
    return geometry(batch, h, w, rgb, levels, g) ? 3 * g.map[levels] : -1;
}

MREFSR_EXPORT int64_t mrefsr_msssim_workspace_bytes(int batch, int h, int w, int rgb, int levels, int backward)
{
    Pyr g;
    if (!geometry(batch, h, w, rgb, levels, g)) return -1;
    return backward ? bwd_workspace_bytes(g) : fwd_workspace_bytes(g);
}

MREFSR_EXPORT int mrefsr_msssim_loss_fwd_f32(const float *pred, const float *target, int batch, int h, int w, int rgb, int levels,
                                             const double *weights, float loss_weight, float *pyramid, float *maps, float *mult,
                                             double *values, void *workspace, int64_t workspace_bytes, float *loss, mrefsr_stream_t stream)
{
    Pyr g;
    MREFSR_REQUIRE(geometry(batch, h, w, rgb, levels, g), "msssim_loss_fwd: " MSSSIM_LIMITS, batch, h, w, levels);
    MREFSR_REQUIRE(pred && target && weights && pyramid && workspace && loss, "msssim_loss_fwd: null pointer");
    MREFSR_REQUIRE((maps && mult) || (!maps && !mult), "msssim_loss_fwd: the coefficient maps and the multipliers come together or not at all");
    MREFSR_REQUIRE(workspace_bytes >= fwd_workspace_bytes(g), "msssim_loss_fwd: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                   (long long)fwd_workspace_bytes(g));
    for (int j = 0; j < levels; ++j) {
        MREFSR_REQUIRE(isfinite(weights[j]) && weights[j] > 0.0, "msssim_loss_fwd: weights[%d] = %g; finite and > 0", j, weights[j]);
        g.w8[j] = weights[j];
    }
    float *partial = (float *)workspace;
    double *F = (double *)((char *)workspace + fwd_partial_bytes(g));
    const Taps taps = gaussian_taps();
    const hipStream_t st = (hipStream_t)stream;
    const dim3 pgrid(mrefsr::cdiv(w, PT), mrefsr::cdiv(h, PT), g.planes);
    if (rgb)
        hipLaunchKernelGGL(msssim_pyramid_kernel<true>, pgrid, dim3(THREADS), 0, st, pred, target, g, pyramid);
    else
        hipLaunchKernelGGL(msssim_pyramid_kernel<false>, pgrid, dim3(THREADS), 0, st, pred, target, g, pyramid);
    hipLaunchKernelGGL(maps ? msssim_stats_kernel<true> : msssim_stats_kernel<false>, dim3((unsigned)g.fblk[levels]), dim3(THREADS), 0, st,
                       (const float *)pyramid, g, taps, maps, partial);
    hipLaunchKernelGGL(msssim_combine_kernel, dim3(1), dim3(THREADS), 0, st, (const float *)partial, g, (double)loss_weight, F, mult, values,
                       loss);
    return mrefsr::check_launch("msssim_loss_fwd");
}

MREFSR_EXPORT int mrefsr_msssim_loss_bwd_f32(const float *pyramid, const float *maps, const float *mult, const float *grad_loss, int batch,
                                             int h, int w, int rgb, int levels, float loss_weight, void *workspace, int64_t workspace_bytes,
                                             float *grad_pred, mrefsr_stream_t stream)
{
    Pyr g;
    MREFSR_REQUIRE(geometry(batch, h, w, rgb, levels, g), "msssim_loss_bwd: " MSSSIM_LIMITS, batch, h, w, levels);
    MREFSR_REQUIRE(pyramid && maps && mult && grad_loss && grad_pred && (workspace || levels == 1), "msssim_loss_bwd: null pointer");
    MREFSR_REQUIRE(workspace_bytes >= bwd_workspace_bytes(g), "msssim_loss_bwd: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                   (long long)bwd_workspace_bytes(g));
    const Taps taps = gaussian_taps();
    const hipStream_t st = (hipStream_t)stream;
    float *own = (float *)workspace;
    if (levels > 1)
        hipLaunchKernelGGL(msssim_bwd_levels_kernel, dim3((unsigned)g.bblk[levels]), dim3(THREADS), 0, st, pyramid, maps, mult, g, taps, own);
    const dim3 grid(g.btx[0], g.bty[0], g.planes);
    const float scale = (float)(-(double)loss_weight / (double)g.planes);
    if (rgb)
        hipLaunchKernelGGL(msssim_bwd_finish_kernel<true>, grid, dim3(THREADS), 0, st, pyramid, maps, mult, (const float *)own, grad_loss, g, taps,
                           scale, grad_pred);
    else
        hipLaunchKernelGGL(msssim_bwd_finish_kernel<false>, grid, dim3(THREADS), 0, st, pyramid, maps, mult, (const float *)own, grad_loss, g, taps,
                           scale, grad_pred);
    return mrefsr::check_launch("msssim_loss_bwd");
}
