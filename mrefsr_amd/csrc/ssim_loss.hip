// The SSIM loss of the training step (train.ssim_opt, losses.SSIMLoss): loss_weight (1 - mean m) over the structural-similarity
// map of Wang et al. ("Image quality assessment: from error visibility to structural similarity", IEEE TIP 2004) with the window
// of the validation metric (mrefsr_amd/metrics.py: 11 taps, sigma 1.5, "valid" region, C1 = (0.01 255)^2, C2 = (0.03 255)^2), in
// fp32 on the unquantised, unclamped images, and its gradient towards pred.
//
// Planes: 'y' mode, one per image, X = 65.481 R + 128.553 G + 24.966 B + 16; 'rgb' mode, three per image, X = 255 x.  The map of
// an H x W plane is MH x MW = (H - 10) x (W - 10).
//
// Forward, one launch: block (tx, ty, plane) owns the TH x TW = 16 x 32 map positions from (16 ty, 32 tx).  It stages the
// 26 x 42 pixels under them of pred and target into LDS as fp32 (the map applied on load, pixels outside the image as 0) MINUS a
// reference value per tile and image, rx / ry = the plane's value at the tile's centre pixel (clamped into the image): the filtered
// moments u = E[x - rx], v = E[y - ry], E[(x - rx)^2], E[(y - ry)^2], E[(x - rx)(y - ry)] give the variances and the covariance
// without the cancellation of E[x^2] - mu^2 at 255 scale (sigma_x^2 = E[(x - rx)^2] - u^2 exactly, whatever rx is); mu_x = u + rx.
// The 11 taps run down the columns into LDS (five planes of 16 x 42), then along the rows in registers.  Each thread forms m at
// its two positions (k = 0, 1: position 256 k + tid of the tile, row-major) and, when a gradient is wanted, stores
//     a = dm/d mu_x   = 2 mu_y (A2 - A1) D + 2 mu_x m (1/B2 - 1/B1)
//     b = dm/d E[x^2] = -m / B2
//     c = dm/d E[xy]  = 2 A1 D
// (derivatives at fixed RAW second moments; A1 = 2 mu_x mu_y + C1, A2 = 2 sigma_xy + C2, B1 = mu_x^2 + mu_y^2 + C1,
// B2 = sigma_x^2 + sigma_y^2 + C2, D = 1 / (B1 B2), m = A1 A2 D) into three [planes, MH, MW] maps.  Sum of m: per thread k = 0 then
// k = 1 (a position outside the map counts 0), the 256 threads by an LDS tree (128, 64, ... 1), one fp32 partial per block written
// through to `partial`; the block that draws the last ticket (reduce.h) adds the partials in ascending block order
// ((plane, ty, tx) row-major) in double and writes loss = fl32(loss_weight (1 - sum / count)).  No float atomics, no readback.
//
// Backward, one launch over 16 x 32 tiles of the INPUT: d(sum m)/dX(p) = (G^T a)(p) + 2 X(p) (G^T b)(p) + Y(p) (G^T c)(p), G^T the
// adjoint of the valid filter = the same 11 x 11 window (it is symmetric) over the maps zero-extended by 10 on every side.  The
// block stages the 26 x 42 map values of a, b, c around its tile (zeros outside the map), filters them as the forward does,
// recomputes X and Y from the images, scales by -loss_weight / count and the upstream gradient (read from the device) and maps the
// result back to R, G, B with the plane's coefficients: every element of grad_pred is written exactly once.
#include <math.h>

#include "common.h"

namespace {

constexpr int TH = 16, TW = 32, HALO = 10, TAPS = 11;
constexpr int SH = TH + HALO, SW = TW + HALO;   // staged rows / columns: 26 x 42
constexpr int THREADS = 256;
constexpr int PER_THREAD = TH * TW / THREADS;   // 2
constexpr float C1 = 6.5025f, C2 = 58.5225f;    // (0.01 * 255)^2, (0.03 * 255)^2
constexpr float YR = 65.481f, YG = 128.553f, YB = 24.966f, Y0 = 16.f;

struct Taps { float g[TAPS]; };

// the taps of metrics._gaussian_window(11, 1.5): exp(-(i - 5)^2 / 4.5) normalised in double, rounded to fp32
const Taps &gaussian_taps()
{
    static const Taps taps = [] {
        double k[TAPS], s = 0.0;
        for (int i = 0; i < TAPS; ++i) s += k[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        Taps t;
        for (int i = 0; i < TAPS; ++i) t.g[i] = (float)(k[i] / s);
        return t;
    }();
    return taps;
}

// plane value at pixel offset `off` of image plane `p`: p indexes images in y mode, (image, channel) pairs in rgb mode
template <bool RGB>
__device__ __forceinline__ float plane_value(const float *__restrict__ img, const long p, const long hw, const long off)
{
    if constexpr (RGB) {
        return 255.f * img[p * hw + off];
    } else {
        const float *px = img + 3 * p * hw + off;
        return YR * px[0] + YG * px[hw] + YB * px[2 * hw] + Y0;
    }
}

// N planes of TH x SW in `v`: the taps down the columns of N planes of SH x SW in `s`; prod(s, i, q) gives plane q's value at index i
template <int N, class F>
__device__ __forceinline__ void filter_columns(float *__restrict__ v, const Taps &taps, const F &prod)
{
    for (int idx = threadIdx.x; idx < TH * SW; idx += THREADS) {
        float acc[N];
#pragma unroll
        for (int q = 0; q < N; ++q) acc[q] = 0.f;
#pragma unroll
        for (int i = 0; i < TAPS; ++i) {
            float val[N];
            prod(idx + i * SW, val);
#pragma unroll
            for (int q = 0; q < N; ++q) acc[q] += taps.g[i] * val[q];
        }
#pragma unroll
        for (int q = 0; q < N; ++q) v[q * TH * SW + idx] = acc[q];
    }
}

// the taps along row r of the N planes in `v`, at column c
template <int N>
__device__ __forceinline__ void filter_row(const float *__restrict__ v, const Taps &taps, const int r, const int c, float (&out)[N])
{
#pragma unroll
    for (int q = 0; q < N; ++q) out[q] = 0.f;
#pragma unroll
    for (int j = 0; j < TAPS; ++j)
#pragma unroll
        for (int q = 0; q < N; ++q) out[q] += taps.g[j] * v[q * TH * SW + r * SW + c + j];
}

template <bool RGB, bool WANT_GRAD>
__global__ __launch_bounds__(THREADS) void ssim_loss_fwd_kernel(const float *__restrict__ pred, const float *__restrict__ target, const int H,
                                                                const int W, const Taps taps, float *__restrict__ ga, float *__restrict__ gb,
                                                                float *__restrict__ gc, float *partial, unsigned int *ticket,
                                                                const double inv_count, const float loss_weight, float *__restrict__ loss)
{
    __shared__ float s[2 * SH * SW];        // pred | target, minus the tile's reference values
    __shared__ float v[5 * TH * SW];        // column-filtered x, y, xx, yy, xy; then the reduction tree
    __shared__ int last;
    const int tid = threadIdx.x;
    const int MH = H - HALO, MW = W - HALO;
    const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
    const long p = blockIdx.z, hw = (long)H * W;
    const int cy = min(y0 + SH / 2, H - 1), cx = min(x0 + SW / 2, W - 1);
    const float rx = plane_value<RGB>(pred, p, hw, (long)cy * W + cx), ry = plane_value<RGB>(target, p, hw, (long)cy * W + cx);

    for (int idx = tid; idx < SH * SW; idx += THREADS) {
        const int gy = y0 + idx / SW, gx = x0 + idx % SW;
        float xv = 0.f, yv = 0.f;
        if (gy < H && gx < W) {
            const long off = (long)gy * W + gx;
            xv = plane_value<RGB>(pred, p, hw, off) - rx;
            yv = plane_value<RGB>(target, p, hw, off) - ry;
        }
        s[idx] = xv;
        s[SH * SW + idx] = yv;
    }
    __syncthreads();
    filter_columns<5>(v, taps, [&](const int i, float (&val)[5]) {
        const float xv = s[i], yv = s[SH * SW + i];
        val[0] = xv, val[1] = yv, val[2] = xv * xv, val[3] = yv * yv, val[4] = xv * yv;
    });
    __syncthreads();

    float msum = 0.f;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int idx = k * THREADS + tid, r = idx / TW, c = idx % TW;
        const int my = y0 + r, mx = x0 + c;
        float f[5];
        filter_row<5>(v, taps, r, c, f);
        const float u = f[0], w = f[1];
        const float mux = u + rx, muy = w + ry;
        const float sxx = f[2] - u * u, syy = f[3] - w * w, sxy = f[4] - u * w;
        const float a1 = 2.f * mux * muy + C1, a2 = 2.f * sxy + C2;
        const float b1 = mux * mux + muy * muy + C1, b2 = sxx + syy + C2;
        const float ib1 = 1.f / b1, ib2 = 1.f / b2, d = ib1 * ib2;
        const float m = a1 * a2 * d;
        if (my < MH && mx < MW) {
            msum += m;
            if constexpr (WANT_GRAD) {
                const long o = (p * MH + my) * MW + mx;
                ga[o] = 2.f * muy * (a2 - a1) * d + 2.f * mux * m * (ib2 - ib1);
                gb[o] = -m * ib2;
                gc[o] = 2.f * a1 * d;
            }
        }
    }
    const float bsum = mrefsr::block_sum<THREADS>(v, msum);   // (meets first: every thread has read v, it becomes the tree)
    const unsigned int nblocks = gridDim.x * gridDim.y * gridDim.z;
    const unsigned int bid = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (tid == 0) mrefsr::store_partial(partial + bid, bsum);
    if (!mrefsr::last_block_by_ticket(ticket, nblocks, &last)) return;
    const double total = mrefsr::sum_partials_in_order(partial, nblocks, v);
    if (tid == 0) loss[0] = (float)((double)loss_weight * (1.0 - total * inv_count));
}

template <bool RGB>
__global__ __launch_bounds__(THREADS) void ssim_loss_bwd_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                                const float *__restrict__ ga, const float *__restrict__ gb,
                                                                const float *__restrict__ gc, const float *__restrict__ gup, const int H,
                                                                const int W, const Taps taps, const float scale, float *__restrict__ grad)
{
    __shared__ float s[3 * SH * SW];        // a | b | c around the tile, zero outside the map
    __shared__ float v[3 * TH * SW];
    const int tid = threadIdx.x;
    const int MH = H - HALO, MW = W - HALO;
    const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
    const long p = blockIdx.z, hw = (long)H * W;

    for (int idx = tid; idx < SH * SW; idx += THREADS) {
        const int my = y0 - HALO + idx / SW, mx = x0 - HALO + idx % SW;
        float av = 0.f, bv = 0.f, cv = 0.f;
        if (my >= 0 && my < MH && mx >= 0 && mx < MW) {
            const long o = (p * MH + my) * MW + mx;
            av = ga[o], bv = gb[o], cv = gc[o];
        }
        s[idx] = av;
        s[SH * SW + idx] = bv;
        s[2 * SH * SW + idx] = cv;
    }
    __syncthreads();
    filter_columns<3>(v, taps, [&](const int i, float (&val)[3]) { val[0] = s[i], val[1] = s[SH * SW + i], val[2] = s[2 * SH * SW + i]; });
    __syncthreads();

    const float f = scale * gup[0];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int idx = k * THREADS + tid, r = idx / TW, c = idx % TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        float t[3];
        filter_row<3>(v, taps, r, c, t);
        const long off = (long)gy * W + gx;
        const float xv = plane_value<RGB>(pred, p, hw, off), yv = plane_value<RGB>(target, p, hw, off);
        const float gx_ = f * (t[0] + 2.f * xv * t[1] + yv * t[2]);
        if constexpr (RGB) {
            grad[p * hw + off] = 255.f * gx_;
        } else {
            float *out = grad + 3 * p * hw + off;
            out[0] = YR * gx_, out[hw] = YG * gx_, out[2 * hw] = YB * gx_;
        }
    }
}

bool shape_ok(const int batch, const int h, const int w)
{
    // (3 batch and the tile rows / columns of a plane within the grid's 65535; a plane's pixel count in 31 bits)
    return batch > 0 && batch <= 21845 && h >= TAPS && w >= TAPS && h <= (1 << 19) && w <= (1 << 19) && (int64_t)h * w <= ((int64_t)1 << 30);
}

int64_t fwd_blocks(const int batch, const int h, const int w, const int rgb)
{
    return (int64_t)(rgb ? 3 : 1) * batch * mrefsr::cdiv(h - HALO, TH) * mrefsr::cdiv(w - HALO, TW);
}

}  // namespace

MREFSR_EXPORT int mrefsr_ssim_loss_blocks(int batch, int h, int w, int rgb)
{
    if (!shape_ok(batch, h, w)) return -1;
    const int64_t n = fwd_blocks(batch, h, w, rgb);
    return n > ((int64_t)1 << 30) ? -1 : (int)n;
}

MREFSR_EXPORT int mrefsr_ssim_loss_fwd_f32(const float *pred, const float *target, int batch, int h, int w, int rgb, float loss_weight,
                                           float *a, float *b, float *c, float *partial, uint32_t *ticket, float *loss,
                                           mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(shape_ok(batch, h, w) && mrefsr_ssim_loss_blocks(batch, h, w, rgb) > 0,
                   "ssim_loss_fwd: batch=%d (1..21845) h=%d w=%d (11..2^19, h*w <= 2^30, at most 2^30 tiles)", batch, h, w);
    MREFSR_REQUIRE(pred && target && partial && ticket && loss, "ssim_loss_fwd: null pointer");
    MREFSR_REQUIRE((a && b && c) || (!a && !b && !c), "ssim_loss_fwd: the coefficient maps a, b, c come all three or not at all");
    const int planes = (rgb ? 3 : 1) * batch;
    const dim3 grid(mrefsr::cdiv(w - HALO, TW), mrefsr::cdiv(h - HALO, TH), planes);
    const double inv_count = 1.0 / ((double)planes * (h - HALO) * (w - HALO));
    const Taps taps = gaussian_taps();
    auto kernel = rgb ? (a ? ssim_loss_fwd_kernel<true, true> : ssim_loss_fwd_kernel<true, false>)
                      : (a ? ssim_loss_fwd_kernel<false, true> : ssim_loss_fwd_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, pred, target, h, w, taps, a, b, c, partial, ticket, inv_count,
                       loss_weight, loss);
    return mrefsr::check_launch("ssim_loss_fwd");
}

MREFSR_EXPORT int mrefsr_ssim_loss_bwd_f32(const float *pred, const float *target, const float *a, const float *b, const float *c,
                                           const float *grad_loss, int batch, int h, int w, int rgb, float loss_weight, float *grad_pred,
                                           mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(shape_ok(batch, h, w), "ssim_loss_bwd: batch=%d (1..21845) h=%d w=%d (11..2^19, h*w <= 2^30)", batch, h, w);
    MREFSR_REQUIRE(pred && target && a && b && c && grad_loss && grad_pred, "ssim_loss_bwd: null pointer");
    const int planes = (rgb ? 3 : 1) * batch;
    const dim3 grid(mrefsr::cdiv(w, TW), mrefsr::cdiv(h, TH), planes);
    const float scale = (float)(-(double)loss_weight / ((double)planes * (h - HALO) * (w - HALO)));
    const Taps taps = gaussian_taps();
    if (rgb)
        hipLaunchKernelGGL(ssim_loss_bwd_kernel<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, pred, target, a, b, c, grad_loss, h, w, taps,
                           scale, grad_pred);
    else
        hipLaunchKernelGGL(ssim_loss_bwd_kernel<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, pred, target, a, b, c, grad_loss, h, w,
                           taps, scale, grad_pred);
    return mrefsr::check_launch("ssim_loss_bwd");
}
