// The artifact loss of LDL (train.ldl_opt, losses.LDLLoss; Liang et al., "Details or Artifacts: A Locally Discriminative Learning
// Approach to Realistic Image Super-Resolution", CVPR 2022; basicsr/losses/loss_util.py:99-145 as used by
// basicsr/models/realesrgan_model.py:211-226), in fp32, and its gradient towards pred THROUGH the weight map.
//
// pred, target, ema [B][3][H][W], H, W >= 4.  r = sum_c |target - pred|, r_e = sum_c |target - ema| (channels added 0, 1, 2),
//     g_b = Var(r_b)^(1/5)             unbiased over the H W pixels of sample b (0 for a variance of exactly 0)
//     v_p = unbiased variance of r over the 7 x 7 window at p of the image reflect-padded by 3 (n = 49)
//     m_p = [r_p >= r_e,p]
//     loss = loss_weight / (3 B H W) sum_b g_b S_b,   S_b = sum_p v_p m_p r_p.
//
// Forward, one launch: block (tx, ty, b) owns the TH x TW = 16 x 32 pixels from (16 ty, 32 tx) of sample b.  It stages r of the
// 22 x 38 pixels under their windows into LDS, the reflect padding resolved by index arithmetic on load (positions further than 3
// outside the image are never read by a pixel inside it and are staged as 0).  Each thread has two pixels (k = 0, 1: position
// 256 k + tid of the tile, row-major).  Per pixel TWO passes over the 49 taps in LDS: the window mean as mu = r_p + sum (tap - r_p)
// / 49 (the sum of the small deviations from the centre tap, not of the taps: the backward's r_p - mu_q is first order in mu's
// error), then the squares about it -- no E[r^2] - mu^2, so a residual of mean 0.9 and local deviation 0.01 keeps its digits.
// Both sums run row by row (seven sums of seven, then their sum).  With maps wanted it stores
// m r, mu and v m.  Block sums by an LDS tree (128, 64, ... 1) in fp32: sum r -> the block's mean, sum (r - mean)^2 -> its M2 (two
// passes again), sum v m r; with the block's pixel count the three go to its row of `partial`.  The block that draws the last
// ticket (reduce.h) finalises: thread t takes samples t, t + 256, ...; per sample it merges the blocks' (count, mean, M2) in double,
// in ascending block order and again in two passes -- mean = sum count_b mean_b / (H W), M2 = sum M2_b + count_b (mean_b - mean)^2:
// one dependent fp64 add per block, where the pairwise update of (count, mean, M2) has two divisions in its chain -- adds their
// sum v m r in the same order, and writes stats[b] = (g_b, mean_b, k_b, S_b), k_b = S_b (1/5) Var_b^(-4/5) 2 / (H W - 1), or 0 for
// a variance of 0; thread 0 then adds the threads' g_b S_b in ascending order in double: loss = fl32(loss_weight / (3 B H W) sum).
// No float atomics, no readback, the same bits from call to call.
//
// Backward, one launch over the same tiles: with s = loss_weight / (3 B H W) times the upstream gradient (read from the device),
//     dL/dr_p = s [ g v_p m_p + (2 / 48) g sum_q mult(q, p) m_q r_q (r_p - mu_q) + k_b (r_p - mean_b) ]
// and grad_pred_c(p) = sign(pred_c - target_c) dL/dr_p.  q runs over the image pixels within 3 of p; mult(q, p) = my(qy, py)
// mx(qx, px) is the number of positions of q's padded window that reflect onto p:
//     m1(q, p) = 1 + [p + q <= 3 and p >= 1] + [(n - 1 - p) + (n - 1 - q) <= 3 and p <= n - 2]          (n = H or W)
// (the position itself, its mirror image about the first pixel, about the last one; for n < 7 both mirrors can hit).  The block
// stages m r and mu of its 22 x 38 neighbourhood (0 outside the image) and sums the 49 products (r_p - mu_q) directly: the
// difference is formed per tap, not as r_p A_p - C_p.  Every element of grad_pred is written exactly once.
//
// ldl_scale_map: w = g_b (v m), the artifact map on request (losses.LDLLoss.artifact_map), one launch.
#include <math.h>

#include "common.h"

namespace {

constexpr int TH = 16, TW = 32, PAD = 3, KS = 7;
constexpr int SH = TH + 2 * PAD, SW = TW + 2 * PAD;   // staged rows / columns: 22 x 38
constexpr int THREADS = 256;
constexpr int PER_THREAD = TH * TW / THREADS;         // 2
constexpr float INV_N = 1.f / 49.f, INV_N1 = 1.f / 48.f;
constexpr int INFLIGHT = 16;                          // block rows of `partial` a finalising thread loads before it merges them

// index i in [-3, n + 3) of the reflect-padded axis -> [0, n) (n >= 4: one reflection is enough)
__device__ __forceinline__ int reflect(const int i, const int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// sum_c |a_c - b_c| at pixel offset off of an image (channels hw apart), added in the order 0, 1, 2
__device__ __forceinline__ float residual(const float *__restrict__ a, const float *__restrict__ b, const long hw, const long off)
{
    return (fabsf(a[off] - b[off]) + fabsf(a[off + hw] - b[off + hw])) + fabsf(a[off + 2 * hw] - b[off + 2 * hw]);
}

__device__ __forceinline__ int tile_count(const int t, const int n, const int size) { return min(size, n - t * size); }

template <bool WANT_MAPS>
__global__ __launch_bounds__(THREADS) void ldl_loss_fwd_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                               const float *__restrict__ ema, const int B, const int H, const int W,
                                                               float *__restrict__ mr, float *__restrict__ mu, float *__restrict__ vm,
                                                               float *partial, unsigned int *ticket, float *__restrict__ stats,
                                                               const double scale, float *__restrict__ loss)
{
    __shared__ float s[SH * SW];        // r under the tile's windows
    __shared__ float red[THREADS];
    __shared__ double acc[THREADS];
    __shared__ int last;
    const int tid = threadIdx.x;
    const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
    const long b = blockIdx.z, hw = (long)H * W;
    const float *p3 = pred + 3 * b * hw, *t3 = target + 3 * b * hw, *e3 = ema + 3 * b * hw;

    for (int idx = tid; idx < SH * SW; idx += THREADS) {
        const int py = y0 - PAD + idx / SW, px = x0 - PAD + idx % SW;   // padded coordinates, >= -3
        float rv = 0.f;
        if (py < H + PAD && px < W + PAD) rv = residual(t3, p3, hw, (long)reflect(py, H) * W + reflect(px, W));
        s[idx] = rv;
    }
    __syncthreads();

    float rp[PER_THREAD], svr = 0.f, rsum = 0.f;
    bool inside[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int idx = k * THREADS + tid, r = idx / TW, c = idx % TW;
        const int gy = y0 + r, gx = x0 + c;
        inside[k] = gy < H && gx < W;
        rp[k] = 0.f;
        if (!inside[k]) continue;
        const float *win = s + r * SW + c;
        const float rv = win[PAD * SW + PAD];
        float sum = 0.f;
#pragma unroll
        for (int dy = 0; dy < KS; ++dy) {
            float row = 0.f;
#pragma unroll
            for (int dx = 0; dx < KS; ++dx) row += win[dy * SW + dx] - rv;
            sum += row;
        }
        const float mean = rv + sum * INV_N;
        float ssq = 0.f;
#pragma unroll
        for (int dy = 0; dy < KS; ++dy) {
            float row = 0.f;
#pragma unroll
            for (int dx = 0; dx < KS; ++dx) {
                const float d = win[dy * SW + dx] - mean;
                row += d * d;
            }
            ssq += row;
        }
        const long off = (long)gy * W + gx;
        const bool keep = rv >= residual(t3, e3, hw, off);
        const float vmask = keep ? ssq * INV_N1 : 0.f;
        rp[k] = rv;
        rsum += rv;
        svr += vmask * rv;
        if constexpr (WANT_MAPS) {
            if (mr) mr[b * hw + off] = keep ? rv : 0.f, mu[b * hw + off] = mean;
            if (vm) vm[b * hw + off] = vmask;
        }
    }
    const int count = tile_count(blockIdx.y, H, TH) * tile_count(blockIdx.x, W, TW);
    const float bmean = mrefsr::block_sum<THREADS>(red, rsum) / (float)count;
    float dev = 0.f;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k)
        if (inside[k]) dev += (rp[k] - bmean) * (rp[k] - bmean);
    const float bm2 = mrefsr::block_sum<THREADS>(red, dev);
    const float bsvr = mrefsr::block_sum<THREADS>(red, svr);
    const unsigned int per_sample = gridDim.x * gridDim.y, nblocks = per_sample * gridDim.z;
    const unsigned int bid = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (tid == 0) {
        mrefsr::store_partial(partial + 4 * bid, (float)count);
        mrefsr::store_partial(partial + 4 * bid + 1, bmean);
        mrefsr::store_partial(partial + 4 * bid + 2, bm2);
        mrefsr::store_partial(partial + 4 * bid + 3, bsvr);
    }
    if (!mrefsr::last_block_by_ticket(ticket, nblocks, &last)) return;

    double mine = 0.0;
    for (int sb = tid; sb < B; sb += THREADS) {
        double mean = 0.0, m2 = 0.0, sv = 0.0;
        // two passes over the sample's block rows, INFLIGHT rows loaded at a time and added in ascending block order: the mean
        // from the blocks' (count, mean), then M2 = sum M2_b + count_b (mean_b - mean)^2 -- one dependent fp64 add per block
        const float *rows = partial + 4 * (long)sb * per_sample;
        for (unsigned int j0 = 0; j0 < per_sample; j0 += INFLIGHT) {
            float cnt[INFLIGHT], mb[INFLIGHT], sb3[INFLIGHT];
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                const bool in = j0 + u < per_sample;
                cnt[u] = in ? __hip_atomic_load(rows + 4 * (j0 + u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
                mb[u] = in ? __hip_atomic_load(rows + 4 * (j0 + u) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
                sb3[u] = in ? __hip_atomic_load(rows + 4 * (j0 + u) + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                mean += (double)cnt[u] * (double)mb[u];
                sv += (double)sb3[u];
            }
        }
        mean /= (double)hw;
        for (unsigned int j0 = 0; j0 < per_sample; j0 += INFLIGHT) {
            float cnt[INFLIGHT], mb[INFLIGHT], qb[INFLIGHT];
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                const bool in = j0 + u < per_sample;
                cnt[u] = in ? __hip_atomic_load(rows + 4 * (j0 + u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
                mb[u] = in ? __hip_atomic_load(rows + 4 * (j0 + u) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
                qb[u] = in ? __hip_atomic_load(rows + 4 * (j0 + u) + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                const double delta = (double)mb[u] - mean;
                m2 += (double)qb[u] + (double)cnt[u] * (delta * delta);
            }
        }
        const double var = m2 / ((double)hw - 1.0);
        const bool positive = var > 0.0;
        const double g = positive ? pow(var, 0.2) : 0.0;
        const double kb = positive ? sv * 0.2 * pow(var, -0.8) * 2.0 / ((double)hw - 1.0) : 0.0;
        stats[4 * sb] = (float)g;
        stats[4 * sb + 1] = (float)mean;
        stats[4 * sb + 2] = (float)kb;
        stats[4 * sb + 3] = (float)sv;
        mine += g * sv;   // (samples t, t + 256, ... in ascending order)
    }
    acc[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        const int n = min(B, THREADS);
        for (int q = 0; q < n; ++q) total += acc[q];
        loss[0] = (float)(scale * total);
    }
}

// multiplicity along one axis of n pixels: positions of q's padded 7-window that reflect onto p (|q - p| <= 3, both in [0, n))
__device__ __forceinline__ float mult1(const int q, const int p, const int n)
{
    return 1.f + (p >= 1 && p + q <= PAD ? 1.f : 0.f) + (p <= n - 2 && (n - 1 - p) + (n - 1 - q) <= PAD ? 1.f : 0.f);
}

__global__ __launch_bounds__(THREADS) void ldl_loss_bwd_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                               const float *__restrict__ mr, const float *__restrict__ mu,
                                                               const float *__restrict__ vm, const float *__restrict__ stats,
                                                               const float *__restrict__ gup, const int H, const int W, const float scale,
                                                               float *__restrict__ grad)
{
    __shared__ float sa[SH * SW];       // m r around the tile, 0 outside the image
    __shared__ float sm[SH * SW];       // the window means
    const int tid = threadIdx.x;
    const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
    const long b = blockIdx.z, hw = (long)H * W;

    for (int idx = tid; idx < SH * SW; idx += THREADS) {
        const int qy = y0 - PAD + idx / SW, qx = x0 - PAD + idx % SW;
        float av = 0.f, mv = 0.f;
        if (qy >= 0 && qy < H && qx >= 0 && qx < W) {
            const long o = b * hw + (long)qy * W + qx;
            av = mr[o], mv = mu[o];
        }
        sa[idx] = av;
        sm[idx] = mv;
    }
    __syncthreads();

    const float g = stats[4 * b], smean = stats[4 * b + 1], kb = stats[4 * b + 2];
    const float f = scale * gup[0];
    const float *p3 = pred + 3 * b * hw, *t3 = target + 3 * b * hw;
    float *g3 = grad + 3 * b * hw;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int idx = k * THREADS + tid, r = idx / TW, c = idx % TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        const long off = (long)gy * W + gx;
        const float d0 = p3[off] - t3[off], d1 = p3[off + hw] - t3[off + hw], d2 = p3[off + 2 * hw] - t3[off + 2 * hw];
        const float rv = (fabsf(d0) + fabsf(d1)) + fabsf(d2);   // (|pred - target| = |target - pred| bit for bit)
        float wx[KS];
#pragma unroll
        for (int dx = 0; dx < KS; ++dx) wx[dx] = mult1(gx - PAD + dx, gx, W);
        float through = 0.f;
#pragma unroll
        for (int dy = 0; dy < KS; ++dy) {
            const float wy = mult1(gy - PAD + dy, gy, H);
            float row = 0.f;
#pragma unroll
            for (int dx = 0; dx < KS; ++dx) {
                const int i = (r + dy) * SW + c + dx;
                row += wx[dx] * sa[i] * (rv - sm[i]);
            }
            through += wy * row;
        }
        const float val = f * (g * vm[b * hw + off] + (2.f * INV_N1) * g * through + kb * (rv - smean));
        g3[off] = d0 > 0.f ? val : (d0 < 0.f ? -val : 0.f);
        g3[off + hw] = d1 > 0.f ? val : (d1 < 0.f ? -val : 0.f);
        g3[off + 2 * hw] = d2 > 0.f ? val : (d2 < 0.f ? -val : 0.f);
    }
}

__global__ __launch_bounds__(THREADS) void ldl_scale_map_kernel(const float *__restrict__ vm, const float *__restrict__ stats, const long hw,
                                                                float *__restrict__ w)
{
    const long b = blockIdx.y, i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i < hw) w[b * hw + i] = stats[4 * b] * vm[b * hw + i];
}

bool shape_ok(const int batch, const int h, const int w)
{
    // (the batch and the tile rows / columns within the grid's 65535; a sample's pixel count in 31 bits)
    return batch > 0 && batch <= 65535 && h >= PAD + 1 && w >= PAD + 1 && h <= (1 << 19) && w <= (1 << 19) && (int64_t)h * w <= ((int64_t)1 << 30);
}

int64_t tile_blocks(const int batch, const int h, const int w) { return (int64_t)batch * mrefsr::cdiv(h, TH) * mrefsr::cdiv(w, TW); }

}  // namespace

MREFSR_EXPORT int mrefsr_ldl_loss_blocks(int batch, int h, int w)
{
    if (!shape_ok(batch, h, w)) return -1;
    const int64_t n = tile_blocks(batch, h, w);
    return n > ((int64_t)1 << 28) ? -1 : (int)n;
}

MREFSR_EXPORT int mrefsr_ldl_loss_fwd_f32(const float *pred, const float *target, const float *ema, int batch, int h, int w, float loss_weight,
                                          float *mr, float *mu, float *vm, float *stats, float *partial, uint32_t *ticket, float *loss,
                                          mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(mrefsr_ldl_loss_blocks(batch, h, w) > 0, "ldl_loss_fwd: batch=%d (1..65535) h=%d w=%d (4..2^19, h*w <= 2^30, at most 2^28 tiles)",
                   batch, h, w);
    MREFSR_REQUIRE(pred && target && ema && stats && partial && ticket && loss, "ldl_loss_fwd: null pointer");
    MREFSR_REQUIRE((mr && mu) || (!mr && !mu), "ldl_loss_fwd: the maps m r and mu come both or not at all");
    const dim3 grid(mrefsr::cdiv(w, TW), mrefsr::cdiv(h, TH), batch);
    const double scale = (double)loss_weight / (3.0 * batch * (double)h * w);
    auto kernel = (mr || vm) ? ldl_loss_fwd_kernel<true> : ldl_loss_fwd_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, pred, target, ema, batch, h, w, mr, mu, vm, partial, ticket, stats,
                       scale, loss);
    return mrefsr::check_launch("ldl_loss_fwd");
}

MREFSR_EXPORT int mrefsr_ldl_loss_bwd_f32(const float *pred, const float *target, const float *mr, const float *mu, const float *vm,
                                          const float *stats, const float *grad_loss, int batch, int h, int w, float loss_weight,
                                          float *grad_pred, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(shape_ok(batch, h, w), "ldl_loss_bwd: batch=%d (1..65535) h=%d w=%d (4..2^19, h*w <= 2^30)", batch, h, w);
    MREFSR_REQUIRE(pred && target && mr && mu && vm && stats && grad_loss && grad_pred, "ldl_loss_bwd: null pointer");
    const dim3 grid(mrefsr::cdiv(w, TW), mrefsr::cdiv(h, TH), batch);
    const float scale = (float)((double)loss_weight / (3.0 * batch * (double)h * w));
    hipLaunchKernelGGL(ldl_loss_bwd_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, pred, target, mr, mu, vm, stats, grad_loss, h, w, scale,
                       grad_pred);
    return mrefsr::check_launch("ldl_loss_bwd");
}

MREFSR_EXPORT int mrefsr_ldl_loss_map_f32(const float *vm, const float *stats, int batch, int h, int w, float *wmap, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(shape_ok(batch, h, w), "ldl_loss_map: batch=%d (1..65535) h=%d w=%d (4..2^19, h*w <= 2^30)", batch, h, w);
    MREFSR_REQUIRE(vm && stats && wmap, "ldl_loss_map: null pointer");
    const long hw = (long)h * w;
    hipLaunchKernelGGL(ldl_scale_map_kernel, dim3(mrefsr::cdiv(hw, THREADS), batch), dim3(THREADS), 0, (hipStream_t)stream, vm, stats, hw, wmap);
    return mrefsr::check_launch("ldl_loss_map");
}
