// Perceptual / style loss of the training step (PerceptualLoss, basicsr/models/losses.py:141-238, under
// MultiRefRestorationModel.optimize_parameters, multi_ref_restoration_model.py:237-279): what the VGG19 node of
// mrefsr_amd/archs/nhwc_train.py runs besides the convolutions.
//   maxpool2_nhwc        MaxPool2d(2, 2) (floor sizes, torch's tie rule), optional 3-bit arg-max / sign plane
//   maxpool2_bwd_nhwc    its backward fused with the preceding ReLU's mask, + max |g| for the fp16-split dgrad
//   tap_crit             L1 / Frobenius criterion of several taps: loss partials (fixed order) and / or the gradient
//   gram_nhwc            G[n] = F^T F / (c h w) (or times a given scale: the texture loss's raw Gram, texture.hip) on v_mfma_f32_16x16x4_f32, upper tiles, split-K, fixed-order second stage
//   gram_bwd_nhwc        dF += (2 / (c h w)) F S, S = d loss / d G formed inside from G(x) and G(gt), same MFMA (tile body: gram.h)
//   image_to_nhwc4_bwd   gradient of the image packing + normalisation (fused_act.hip: image_to_nhwc4) -> [N][3][HW]
// All element-wise / reduction kernels are HBM-bound; the Gram products are a few GFLOP per step.
#include "gram.h"

namespace {

using mrefsr::grid_of;
using mrefsr::gram::f32x4;

__device__ inline float relu_in(float v, int relu) { return (relu && v < 0.f) ? 0.f : v; }

// ---------------------------------------------------------------------------------------------------------------
// MaxPool2d(2, 2) on [N][H][W][C] (C % 4 == 0): one thread per output pixel and 4 channels.  Window order (0,0) (0,1) (1,0)
// (1,1); a later element replaces the maximum only when strictly greater (or NaN): torch's max_pool2d, whose first maximum in
// row-major order wins.  relu: the window is max(x, 0) (a pre-activation map whose ReLU was not materialised).
// plane (may be NULL): per output element bits 0-1 = the arg-max, bit 2 = (max > 0), for the backward.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool2_kernel(const float *__restrict__ x, float *__restrict__ out, uchar4 *__restrict__ plane,
                                                       int H, int W, int C4, long total, int relu)
{
    const int Ho = H >> 1, Wo = W >> 1;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        const long q = i / C4;
        const int ox = (int)(q % Wo);
        const long r = q / Wo;
        const int oy = (int)(r % Ho);
        const long n = r / Ho;
        const float4 *src = reinterpret_cast<const float4 *>(x) + ((n * H + 2 * oy) * W + 2 * ox) * C4 + c4;
        const float4 v[4] = {src[0], src[C4], src[(long)W * C4], src[(long)W * C4 + C4]};
        float best[4] = {relu_in(v[0].x, relu), relu_in(v[0].y, relu), relu_in(v[0].z, relu), relu_in(v[0].w, relu)};
        unsigned char arg[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float e[4] = {relu_in(v[k].x, relu), relu_in(v[k].y, relu), relu_in(v[k].z, relu), relu_in(v[k].w, relu)};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e[j] > best[j] || isnan(e[j])) best[j] = e[j], arg[j] = (unsigned char)k;
        }
        reinterpret_cast<float4 *>(out)[i] = make_float4(best[0], best[1], best[2], best[3]);
        if (plane)
            plane[i] = make_uchar4(arg[0] | (best[0] > 0.f ? 4 : 0), arg[1] | (best[1] > 0.f ? 4 : 0), arg[2] | (best[2] > 0.f ? 4 : 0),
                                   arg[3] | (best[3] > 0.f ? 4 : 0));
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Backward of [ReLU ->] MaxPool2d(2, 2): g [N][Ho][Wo][C] -> g_in [N][H][W][C], every element written (the floored last row /
// column of an odd map gets zeros).  One thread per cell of the ceil grid and 4 channels.  The arg-max comes from `plane` or is
// recomputed from x with the forward's rule; mask: the ReLU derivative (max > 0) is applied -- the window's other elements are
// zero anyway, and at the arg-max the ReLU output is the maximum.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float *__restrict__ g, const float *__restrict__ x,
                                                           const uchar4 *__restrict__ plane, float *__restrict__ g_in,
                                                           unsigned int *__restrict__ amax_bits, int H, int W, int C4, long total, int relu,
                                                           int mask)
{
    const int Ho = H >> 1, Wo = W >> 1, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
    float amx = 0.f;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        const long q = i / C4;
        const int cx = (int)(q % Wc);
        const long r = q / Wc;
        const int cy = (int)(r % Hc);
        const long n = r / Hc;
        float4 *dst = reinterpret_cast<float4 *>(g_in) + ((n * H + 2 * cy) * W + 2 * cx) * C4 + c4;
        const bool has_r = 2 * cx + 1 < W, has_d = 2 * cy + 1 < H;
        float o[4][4] = {};   // [window element][channel]
        if (cy < Ho && cx < Wo) {
            const long oi = ((n * Ho + cy) * Wo + cx) * C4 + c4;
            const float4 gv = reinterpret_cast<const float4 *>(g)[oi];
            const float ge[4] = {gv.x, gv.y, gv.z, gv.w};
            int arg[4];
            bool pos[4];
            if (plane) {
                const uchar4 pv = plane[oi];
                const unsigned char pe[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) arg[j] = pe[j] & 3, pos[j] = (pe[j] & 4) != 0;
            } else {
                const float4 *src = reinterpret_cast<const float4 *>(x) + ((n * H + 2 * cy) * W + 2 * cx) * C4 + c4;
                const float4 v[4] = {src[0], src[C4], src[(long)W * C4], src[(long)W * C4 + C4]};
                float best[4] = {relu_in(v[0].x, relu), relu_in(v[0].y, relu), relu_in(v[0].z, relu), relu_in(v[0].w, relu)};
#pragma unroll
                for (int j = 0; j < 4; ++j) arg[j] = 0;
#pragma unroll
                for (int k = 1; k < 4; ++k) {
                    const float e[4] = {relu_in(v[k].x, relu), relu_in(v[k].y, relu), relu_in(v[k].z, relu), relu_in(v[k].w, relu)};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (e[j] > best[j] || isnan(e[j])) best[j] = e[j], arg[j] = k;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) pos[j] = best[j] > 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = (!mask || pos[j]) ? ge[j] : 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k][j] = arg[j] == k ? v : 0.f;   // (selects: no dynamically indexed register array)
                amx = fmaxf(amx, fabsf(v));
            }
        }
        dst[0] = make_float4(o[0][0], o[0][1], o[0][2], o[0][3]);
        if (has_r) dst[C4] = make_float4(o[1][0], o[1][1], o[1][2], o[1][3]);
        if (has_d) dst[(long)W * C4] = make_float4(o[2][0], o[2][1], o[2][2], o[2][3]);
        if (has_r && has_d) dst[(long)W * C4 + C4] = make_float4(o[3][0], o[3][1], o[3][2], o[3][3]);
    }
    if (amax_bits) mrefsr::publish_amax<false>(amax_bits, amx);
}

// ---------------------------------------------------------------------------------------------------------------
// Tap criterion.  Job j owns blocks [first[j], first[j+1]); block b of a job sums the elements b*256 + t + k * nb*256 in a
// fixed order (double), then the block in a fixed tree: partial[first[j] + b].  Gradient (grad != NULL), torch's autograd
// arithmetic of  ((sum_k crit(x_k, y_k) * w_k) * loss_weight) * gup:
//   l1   grad (+)= (((gup * loss_weight) * w_k) * (1 / n)) * sgn(x - y)       (mean backward multiplies by the reciprocal)
//   fro  grad (+)= (x - y) * (((gup * loss_weight) * w_k) / norm_k)            (0 where norm_k == 0)
// ---------------------------------------------------------------------------------------------------------------
struct TapArgs {
    mrefsr_tap_job job[MREFSR_TAP_MAX_JOBS];
    int first[MREFSR_TAP_MAX_JOBS + 1];
    int n_jobs, crit, accumulate;
    float loss_weight[2];
    const float *gup, *norms;
    double *partial;
    unsigned int *amax_bits;
};

__global__ __launch_bounds__(256) void tap_crit_kernel(const TapArgs a)
{
    __shared__ double red[256];
    int j = 0;
    while (j + 1 < a.n_jobs && (int)blockIdx.x >= a.first[j + 1]) ++j;
    const mrefsr_tap_job &jb = a.job[j];
    const int b = blockIdx.x - a.first[j], nb = a.first[j + 1] - a.first[j];
    const long n4 = jb.n / 4;
    const float4 *x = reinterpret_cast<const float4 *>(jb.x), *y = reinterpret_cast<const float4 *>(jb.y);
    float4 *gr = reinterpret_cast<float4 *>(jb.grad);
    float coef = 0.f;
    if (gr) {
        const float up = a.gup ? a.gup[jb.group] : 1.0f;
        const float base = __fmul_rn(__fmul_rn(up, a.loss_weight[jb.group]), jb.weight);
        if (a.crit == 0) coef = __fmul_rn(base, jb.inv_n);
        else {
            const float nrm = a.norms[j];
            coef = nrm == 0.f ? 0.f : base / nrm;
        }
    }
    double s = 0.0;
    float amx = 0.f;
    for (long i = (long)b * 256 + threadIdx.x; i < n4; i += (long)nb * 256) {
        const float4 xv = x[i], yv = y[i];
        const float d[4] = {xv.x - yv.x, xv.y - yv.y, xv.z - yv.z, xv.w - yv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) s += a.crit == 0 ? (double)fabsf(d[k]) : (double)d[k] * (double)d[k];
        if (gr) {
            float gv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float sg = d[k] > 0.f ? 1.f : (d[k] < 0.f ? -1.f : (d[k] == 0.f ? 0.f : d[k]));
                gv[k] = a.crit == 0 ? __fmul_rn(coef, sg) : __fmul_rn(d[k], coef);
            }
            if (a.accumulate) {
                const float4 o = gr[i];
                gv[0] = __fadd_rn(o.x, gv[0]), gv[1] = __fadd_rn(o.y, gv[1]), gv[2] = __fadd_rn(o.z, gv[2]), gv[3] = __fadd_rn(o.w, gv[3]);
            }
            gr[i] = make_float4(gv[0], gv[1], gv[2], gv[3]);
#pragma unroll
            for (int k = 0; k < 4; ++k) amx = fmaxf(amx, fabsf(gv[k]));
        }
    }
    if (a.partial) {
        s = mrefsr::block_sum<256>(red, s);
        if (threadIdx.x == 0) a.partial[blockIdx.x] = s;
    }
    if (gr && a.amax_bits) mrefsr::publish_amax<false>(a.amax_bits, amx);
}

// second stage: loss_k = sum / n (l1) or sqrt(sum) (fro), totals[g] = (sum over the jobs of group g, in order, of loss_k * w_k)
// * loss_weight[g] -- the reference's `loss = 0; loss += crit * w_k; loss *= weight`
__global__ __launch_bounds__(64) void tap_crit_finish_kernel(const TapArgs a, float *__restrict__ losses, float *__restrict__ totals)
{
    __shared__ float lk[MREFSR_TAP_MAX_JOBS];
    const int j = threadIdx.x;
    if (j < a.n_jobs) {
        double s = 0.0;
        for (int b = a.first[j]; b < a.first[j + 1]; ++b) s += a.partial[b];
        const float l = a.crit == 0 ? (float)(s / (double)a.job[j].n) : (float)sqrt(s);
        lk[j] = l;
        if (losses) losses[j] = l;
    }
    __syncthreads();
    if (j == 0 && totals) {
        float t[2] = {0.f, 0.f};
        bool any[2] = {false, false};
        for (int k = 0; k < a.n_jobs; ++k) {
            const int g = a.job[k].group;
            t[g] = __fadd_rn(t[g], __fmul_rn(lk[k], a.job[k].weight));
            any[g] = true;
        }
        totals[0] = any[0] ? __fmul_rn(t[0], a.loss_weight[0]) : 0.f;
        totals[1] = any[1] ? __fmul_rn(t[1], a.loss_weight[1]) : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Gram matrix on the f32 matrix pipe.  Block = 4 waves = one 64 x 64 tile (ti <= tj) of G[n] over one K range of pixels;
// wave w: the 32 x 32 quarter (w >> 1, w & 1), 2 x 2 accumulators of v_mfma_f32_16x16x4_f32 (exact f32 products, one
// rounding per product and sum, k-ordered).  Operands straight from the NHWC rows: lane l reads F[p0 + (l >> 4)][col + (l & 15)],
// 64-byte runs of one pixel (A[i][k] = F[k][i], B[k][j] = F[k][j]).  Partial tile -> ws[s][n][C][C].
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gram_kernel(const float *__restrict__ f, int N, int HW, int C, int S, int chunk,
                                                   float *__restrict__ ws)
{
    const int T = C / 64;
    int pair = blockIdx.x, ti = 0;
    while (pair >= T - ti) pair -= T - ti, ++ti;
    const int tj = ti + pair;
    const int s = blockIdx.y, n = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i0 = ti * 64 + (wave >> 1) * 32, j0 = tj * 64 + (wave & 1) * 32;
    const int kb = s * chunk, ke = min(HW, kb + chunk);
    const float *fn = f + (long)n * HW * C;
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kl = lane >> 4, cl = lane & 15;
    for (int k = kb; k < ke; k += 4) {
        const int p = k + kl;
        const bool ok = p < ke;
        const float *row = fn + (long)(ok ? p : kb) * C;
        float av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) av[a] = ok ? row[i0 + 16 * a + cl] : 0.f;
#pragma unroll
        for (int b = 0; b < 2; ++b) bv[b] = ok ? row[j0 + 16 * b + cl] : 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
    // C/D: column (j) = lane & 15, row (i) = 4 (lane >> 4) + r
    float *out = ws + ((long)s * N + n) * C * C;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(long)(i0 + 16 * a + 4 * kl + r) * C + j0 + 16 * b + cl] = acc[a][b][r];
}

// G[n][i][j] = (sum over s, in order, of the upper tile's partial) * inv_chw; (i, j) in a lower tile reads the mirrored element,
// so G is exactly symmetric
__global__ __launch_bounds__(256) void gram_finish_kernel(const float *__restrict__ ws, float *__restrict__ g, int N, int C, int S,
                                                          float inv_chw)
{
    const long total = (long)N * C * C;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int j = (int)(e % C);
        const long r = e / C;
        const int i = (int)(r % C);
        const long n = r / C;
        const long src = (i / 64 <= j / 64) ? ((long)i * C + j) : ((long)j * C + i);
        float acc = 0.f;
        for (int s = 0; s < S; ++s) acc += ws[((long)s * N + n) * C * C + src];
        g[e] = acc * inv_chw;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Gram backward: dF[n][p][j] (+)= 2 * sum_k F[n][p][k] S'[n][k][j],  S' = sgn(Gx - Gg) * (coef * inv_chw) (symmetric): the tile
// body of gram.h with the scaled sign as its A operand and the factor 2 behind the sums.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gram_bwd_kernel(const float *__restrict__ f, const float *__restrict__ gx, const float *__restrict__ gg,
                                                       float *__restrict__ df, int HW, int C, const float *__restrict__ gup, float loss_weight,
                                                       float weight, float inv_numel, float inv_chw, int accumulate,
                                                       unsigned int *__restrict__ amax_bits)
{
    const float up = gup ? *gup : 1.0f;
    const float coef = __fmul_rn(__fmul_rn(__fmul_rn(up, loss_weight), weight), inv_numel);
    const float sc = __fmul_rn(coef, inv_chw);
    // (the capture is read in front of the selects: read inside them, they compile to 17 more branches instead of v_cndmask)
    mrefsr::gram::bwd_tile(f, gx, gg, df, HW, C, accumulate, amax_bits,
                           [sc](const float d) { const float s = sc; return d > 0.f ? s : (d < 0.f ? -s : 0.f); }, [](long) { return 2.f; }, false);
}

// gradient of image_to_nhwc4: g4 [N][HW][ld] (channels 0..2) -> g_img [N][3][HW] = (g / std) * 0.5 (torch's order: the division's
// backward, then the (x + 1) * 0.5 of norm_img)
__global__ __launch_bounds__(256) void image_bwd_kernel(const float *__restrict__ g4, int ld, float *__restrict__ g_img, long n_px, long HW,
                                                        int range_norm, const float *__restrict__ stdv)
{
    float sd[3] = {1.f, 1.f, 1.f};
    if (stdv) {
#pragma unroll
        for (int c = 0; c < 3; ++c) sd[c] = stdv[c];
    }
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n_px; i += (long)gridDim.x * blockDim.x) {
        const long n = i / HW, p = i - n * HW;
        const float *src = g4 + i * ld;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = src[c];
            if (stdv) v = v / sd[c];
            if (range_norm) v = v * 0.5f;
            g_img[(n * 3 + c) * HW + p] = v;
        }
    }
}

}  // namespace

MREFSR_EXPORT int mrefsr_maxpool2_nhwc_f32(const float *x, float *out, uint8_t *plane, int N, int H, int W, int C, int relu,
                                           mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && out, "maxpool2_nhwc: null pointer");
    MREFSR_REQUIRE(N > 0 && H >= 2 && W >= 2 && C > 0 && C % 4 == 0, "maxpool2_nhwc: N=%d H=%d W=%d C=%d (H, W >= 2, C %% 4 == 0)", N, H, W, C);
    const long total = (long)N * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(maxpool2_kernel, dim3(grid_of((total + 255) / 256, 16384)), dim3(256), 0, (hipStream_t)stream, x, out,
                       reinterpret_cast<uchar4 *>(plane), H, W, C / 4, total, relu);
    return mrefsr::check_launch("maxpool2_nhwc");
}

MREFSR_EXPORT int mrefsr_maxpool2_bwd_nhwc_f32(const float *g, const float *x, const uint8_t *plane, float *g_in, float *amax, int N, int H,
                                               int W, int C, int relu, int mask, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(g && g_in && (x || plane), "maxpool2_bwd_nhwc: null pointer (x or plane is needed)");
    MREFSR_REQUIRE(N > 0 && H >= 2 && W >= 2 && C > 0 && C % 4 == 0, "maxpool2_bwd_nhwc: N=%d H=%d W=%d C=%d (H, W >= 2, C %% 4 == 0)", N, H,
                   W, C);
    const long total = (long)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4);
    hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3(grid_of((total + 255) / 256, 16384)), dim3(256), 0, (hipStream_t)stream, g, x,
                       reinterpret_cast<const uchar4 *>(plane), g_in, reinterpret_cast<unsigned int *>(amax), H, W, C / 4, total, relu, mask);
    return mrefsr::check_launch("maxpool2_bwd_nhwc");
}

MREFSR_EXPORT int mrefsr_tap_crit_blocks(int64_t n)
{
    if (n <= 0) return -1;
    const long b = (n / 4 + 256 * 8 - 1) / (256 * 8);   // >= 8 float4 per thread, at most 256 blocks per job
    return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

MREFSR_EXPORT int mrefsr_tap_crit_f32(const mrefsr_tap_job *jobs, int n_jobs, int crit, float loss_weight0, float loss_weight1, const float *gup,
                                      const float *norms, int accumulate, double *partial, float *losses, float *totals, float *amax,
                                      mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(jobs && n_jobs > 0 && n_jobs <= MREFSR_TAP_MAX_JOBS, "tap_crit: 1..%d jobs, got %d", MREFSR_TAP_MAX_JOBS, n_jobs);
    MREFSR_REQUIRE(crit == 0 || crit == 1, "tap_crit: crit=%d (0 l1, 1 fro)", crit);
    MREFSR_REQUIRE(partial || !(losses || totals), "tap_crit: loss outputs need the partial-sum workspace");
    TapArgs a = {};
    int nb = 0;
    bool any_grad = false;
    for (int j = 0; j < n_jobs; ++j) {
        const mrefsr_tap_job &jb = jobs[j];
        MREFSR_REQUIRE(jb.x && jb.y && jb.n > 0 && jb.n % 4 == 0 && (jb.group == 0 || jb.group == 1),
                       "tap_crit: job %d: null pointer, n=%ld (a positive multiple of 4) or group=%d", j, (long)jb.n, jb.group);
        MREFSR_REQUIRE((reinterpret_cast<uintptr_t>(jb.x) | reinterpret_cast<uintptr_t>(jb.y) | reinterpret_cast<uintptr_t>(jb.grad)) % 16 == 0,
                       "tap_crit: job %d: pointers must be 16-byte aligned", j);
        any_grad |= jb.grad != nullptr;
        a.job[j] = jb;
        a.first[j] = nb;
        nb += mrefsr_tap_crit_blocks(jb.n);
    }
    MREFSR_REQUIRE(!(any_grad && crit == 1 && !norms), "tap_crit: the Frobenius gradient needs the norms of the forward");
    a.first[n_jobs] = nb;
    a.n_jobs = n_jobs, a.crit = crit, a.accumulate = accumulate ? 1 : 0;
    a.loss_weight[0] = loss_weight0, a.loss_weight[1] = loss_weight1;
    a.gup = gup, a.norms = norms, a.partial = partial, a.amax_bits = reinterpret_cast<unsigned int *>(amax);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tap_crit_kernel, dim3(nb), dim3(256), 0, st, a);
    if (losses || totals) hipLaunchKernelGGL(tap_crit_finish_kernel, dim3(1), dim3(64), 0, st, a, losses, totals);
    return mrefsr::check_launch("tap_crit");
}

MREFSR_EXPORT int mrefsr_tap_crit_workspace_bytes(const mrefsr_tap_job *jobs, int n_jobs)
{
    if (!jobs || n_jobs <= 0 || n_jobs > MREFSR_TAP_MAX_JOBS) return -1;
    int nb = 0;
    for (int j = 0; j < n_jobs; ++j) nb += mrefsr_tap_crit_blocks(jobs[j].n);
    return nb * (int)sizeof(double);
}

MREFSR_EXPORT int mrefsr_gram_splits(int N, int HW, int C)
{
    if (N <= 0 || HW <= 0 || C <= 0 || C % 64) return -1;
    const int T = C / 64, tiles = T * (T + 1) / 2;
    int s = (512 + N * tiles - 1) / (N * tiles);          // ~512 blocks in flight
    const int smax = (HW + 63) / 64;                      // >= 64 pixels per split
    return s < 1 ? 1 : (s > smax ? smax : s);
}

MREFSR_EXPORT int64_t mrefsr_gram_workspace_bytes(int N, int HW, int C)
{
    const int s = mrefsr_gram_splits(N, HW, C);
    return s < 0 ? -1 : (int64_t)s * N * C * C * 4;
}

MREFSR_EXPORT int mrefsr_gram_nhwc_scaled_f32(const float *f, int N, int HW, int C, float scale, float *gram, void *workspace,
                                              int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(f && gram && workspace, "gram_nhwc: null pointer");
    if (const int e = mrefsr::gram::check_gram("gram_nhwc", N, HW, C)) return e;
    const int S = mrefsr_gram_splits(N, HW, C);
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_gram_workspace_bytes(N, HW, C), "gram_nhwc: workspace of %ld bytes < %ld", (long)workspace_bytes,
                   (long)mrefsr_gram_workspace_bytes(N, HW, C));
    const int T = C / 64, chunk = ((HW + S - 1) / S + 3) / 4 * 4;
    const int S_used = (HW + chunk - 1) / chunk;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gram_kernel, dim3(T * (T + 1) / 2, S_used, N), dim3(256), 0, st, f, N, HW, C, S_used, chunk, (float *)workspace);
    const long total = (long)N * C * C;
    hipLaunchKernelGGL(gram_finish_kernel, dim3(grid_of((total + 255) / 256, 4096)), dim3(256), 0, st, (const float *)workspace, gram, N, C,
                       S_used, scale);
    return mrefsr::check_launch("gram_nhwc");
}

MREFSR_EXPORT int mrefsr_gram_nhwc_f32(const float *f, int N, int HW, int C, float *gram, void *workspace, int64_t workspace_bytes,
                                       mrefsr_stream_t stream)
{
    return mrefsr_gram_nhwc_scaled_f32(f, N, HW, C, 1.0f / ((float)C * (float)HW), gram, workspace, workspace_bytes, stream);
}

MREFSR_EXPORT int mrefsr_gram_bwd_nhwc_f32(const float *f, const float *gx, const float *gg, float *df, int N, int HW, int C, const float *gup,
                                           float loss_weight, float weight, int accumulate, float *amax, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(f && gx && gg && df, "gram_bwd_nhwc: null pointer");
    if (const int e = mrefsr::gram::check_gram("gram_bwd_nhwc", N, HW, C)) return e;
    const float inv_numel = 1.0f / ((float)N * (float)C * (float)C), inv_chw = 1.0f / ((float)C * (float)HW);
    hipLaunchKernelGGL(gram_bwd_kernel, dim3((HW + 63) / 64, C / 64, N), dim3(256), 0, (hipStream_t)stream, f, gx, gg, df, HW, C, gup,
                       loss_weight, weight, inv_numel, inv_chw, accumulate ? 1 : 0, reinterpret_cast<unsigned int *>(amax));
    return mrefsr::check_launch("gram_bwd_nhwc");
}

MREFSR_EXPORT int mrefsr_image_to_nhwc4_bwd_f32(const float *g4, int ld, float *g_img, int64_t N, int64_t HW, int range_norm, const float *std3,
                                                mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(g4 && g_img, "image_to_nhwc4_bwd: null pointer");
    MREFSR_REQUIRE(N > 0 && HW > 0 && ld >= 3, "image_to_nhwc4_bwd: N=%ld HW=%ld ld=%d", (long)N, (long)HW, ld);
    const long n_px = (long)N * HW;
    hipLaunchKernelGGL(image_bwd_kernel, dim3(grid_of((n_px + 255) / 256, 16384)), dim3(256), 0, (hipStream_t)stream, g4, ld, g_img, n_px,
                       (long)HW, range_norm, std3);
    return mrefsr::check_launch("image_to_nhwc4_bwd");
}
