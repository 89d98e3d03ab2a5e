// The SSIM loss of the training step (train.ssim_opt, losses.SSIMLoss): loss_weight (1 - mean m) over the structural-similarity
// map of Wang et al. ("Image quality assessment: from error visibility to structural similarity", IEEE TIP 2004) with the window
// of the validation metric (mrefsr_amd/metrics.py: 11 taps, sigma 1.5, "valid" region, C1 = (0.01 255)^2, C2 = (0.03 255)^2), in
// fp32 on the unquantised, unclamped images, and its gradient towards pred.
//
// Planes: 'y' mode, one per image, X = 65.481 R + 128.553 G + 24.966 B + 16; 'rgb' mode, three per image, X = 255 x.  The map of
// an H x W plane is MH x MW = (H - 10) x (W - 10).
//
// Forward, one launch: block (tx, ty, plane) owns the TH x TW = 16 x 32 map positions from (16 ty, 32 tx) and runs the forward
// tile body of ssim_window.h (moments_tile) on pred and target, the plane's map applied on load: the window moments from pixels
// staged MINUS a per-tile reference value, so that the variances do not cancel at 255 scale.  Each thread forms m at its two
// positions and, when a gradient is wanted, stores the coefficients a = dm/d mu_x, b = dm/d E[x^2], c = dm/d E[xy] (derivatives at
// fixed RAW second moments: ssim_terms) into three [planes, MH, MW] maps.  Sum of m: per thread k = 0 then k = 1 (a position
// outside the map counts 0), the 256 threads by an LDS tree (128, 64, ... 1), one fp32 partial per block written
// through to `partial`; the block that draws the last ticket (reduce.h) adds the partials in ascending block order
// ((plane, ty, tx) row-major) in double and writes loss = fl32(loss_weight (1 - sum / count)).  No float atomics, no readback.
//
// Backward, one launch over 16 x 32 tiles of the INPUT: d(sum m)/dX(p) = (G^T a)(p) + 2 X(p) (G^T b)(p) + Y(p) (G^T c)(p), G^T the
// adjoint of the valid filter over the maps zero-extended by 10 (adjoint_tile of ssim_window.h).  The block recomputes X and Y
// from the images, scales by -loss_weight / count and the upstream gradient (read from the device) and maps the result back to
// R, G, B with the plane's coefficients: every element of grad_pred is written exactly once.
#include "common.h"
#include "ssim_window.h"

namespace {

using namespace mrefsr::ssim;

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
    const long p = blockIdx.z, hw = (long)H * W;

    float msum = 0.f;
    moments_tile(
        s, v, taps, H, W, blockIdx.y * TH, blockIdx.x * TW,
        [&](const long off, float &xv, float &yv) { xv = plane_value<RGB>(pred, p, hw, off), yv = plane_value<RGB>(target, p, hw, off); },
        [&](const int my, const int mx, const Moments &q) {
            const Terms t = ssim_terms(q);
            if (my >= MH || mx >= MW) return;
            msum += t.m;
            if constexpr (WANT_GRAD) {
                const long o = (p * MH + my) * MW + mx;
                ga[o] = t.a, gb[o] = t.b, gc[o] = t.c;
            }
        });
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
    const int MH = H - HALO, MW = W - HALO;
    const long p = blockIdx.z, hw = (long)H * W;
    const float f = scale * gup[0];
    adjoint_tile(
        s, v, taps, H, W, blockIdx.y * TH, blockIdx.x * TW,
        [&](const int my, const int mx, float &av, float &bv, float &cv) {
            const long o = (p * MH + my) * MW + mx;
            av = ga[o], bv = gb[o], cv = gc[o];
        },
        [&](const int gy, const int gx, const float (&t)[3]) {
            const long off = (long)gy * W + gx;
            const float xv = plane_value<RGB>(pred, p, hw, off), yv = plane_value<RGB>(target, p, hw, off);
            store_plane_grad<RGB>(grad, p, hw, off, f * (t[0] + 2.f * xv * t[1] + yv * t[2]));
        });
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
