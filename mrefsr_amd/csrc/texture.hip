// Texture loss of the training step (TextureLoss, basicsr/models/losses.py:430-532) and the swapped reference maps it compares
// against, which the reference model reads but never builds.
//   texture_select      per match position: the valid reference with the largest match value (ties: the lowest k), that value
//                       (the loss's `weights`) and the matched patch index
//   texture_swap_nhwc   maps_s[b][Y][X][:] = mean of the <= 9 reference patches pasted over (Y, X): float4 gathers from the
//                       references' NHWC maps where they lie, ascending (y, x) order, one correctly rounded division
//   texture_coeff       sigmoid(-20 bicubic_s(replicate_pad(weights)) + 0.65) for s = 1, 2, 4 in one launch (torch's
//                       upsample_bicubic2d with align_corners: A = -0.75, clamped taps), evaluated in fp64, rounded once
//   texture_scale_nhwc  Fc = F (.) coeff (broadcast over the channels)
//   texture_crit        per layer ||G(x) - G(maps)||_F (fp64 sums in a fixed order, no atomics), the layer terms and the total
//   texture_gram_bwd    dF (+)= coeff (.) (2 Fc (Gx - Gm)) * sc, sc = gup * loss_weight / 3 / 4 / D / norm (0 where norm == 0),
//                       on v_mfma_f32_16x16x4_f32: the tile body of gram.h, which gram_bwd_nhwc of percep.hip runs too, with max |dF|
//                       for the Winograd input scale
// The Gram matrices themselves are mrefsr_gram_nhwc_scaled_f32 (percep.hip) with scale 1.
// Built with -ffp-contract=off: the swap's additions and its division are the roundings the source spells out.
#include "gram.h"

namespace {

using mrefsr::grid_of;

// ---------------------------------------------------------------------------------------------------------------
// Selection: one thread per (b, position).  idx, val [K][B][P]; valid_bits [B] (bit k = reference k of sample b present; NULL:
// all).  A later reference replaces the best one only when strictly greater: the lowest k among equal maxima wins.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void select_kernel(const long long *__restrict__ idx, const float *__restrict__ val,
                                                     const int *__restrict__ valid_bits, int *__restrict__ sel, float *__restrict__ wts,
                                                     int *__restrict__ pidx, int K, int B, long P)
{
    const long total = (long)B * P;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / P);
        const unsigned int bits = valid_bits ? (unsigned int)valid_bits[b] : 0xffffffffu;
        int best = -1;
        float bv = 0.f;
        for (int k = 0; k < K; ++k) {
            if (!((bits >> k) & 1u)) continue;
            const float v = val[(long)k * total + i];
            if (best < 0 || v > bv) best = k, bv = v;
        }
        if (best < 0) best = 0, bv = val[i];   // (a sample without a valid reference is refused on the host)
        sel[i] = best;
        wts[i] = bv;
        pidx[i] = (int)idx[(long)best * total + i];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Swap: one thread per output pixel and float4 of channels.  feat [K][B][sh][sw][C]; sel, pidx [B][gh][gw], gh = h - 2, gw = w - 2.
// Match position (y, x) covers the pixels s y <= Y < s y + 3 s, i.e. y in {Y / s - 2, .., Y / s} intersected with the grid (and the
// same along x): 1 to 9 positions, counted by index arithmetic.  Source pixel of a term: (s iy + Y - s y, s ix + X - s x) with
// (iy, ix) = divmod(pidx, gw) < (gh, gw), so it is inside the reference map; an out-of-range pidx is clamped to the grid.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swap_kernel(const float *__restrict__ feat, const int *__restrict__ sel, const int *__restrict__ pidx,
                                                   float *__restrict__ out, int K, int B, int h, int w, int s, int C4, long total)
{
    const int gh = h - 2, gw = w - 2, sh = s * h, sw = s * w;
    const float4 *src = reinterpret_cast<const float4 *>(feat);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        const long q = i / C4;
        const int X = (int)(q % sw);
        const long r = q / sw;
        const int Y = (int)(r % sh);
        const int b = (int)(r / sh);
        const int y1 = min(Y / s, gh - 1), y0 = max(Y / s - 2, 0);
        const int x1 = min(X / s, gw - 1), x0 = max(X / s - 2, 0);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int y = y0; y <= y1; ++y) {
            for (int x = x0; x <= x1; ++x) {
                const long m = ((long)b * gh + y) * gw + x;
                const int k = min(max(sel[m], 0), K - 1);
                const int p = min(max(pidx[m], 0), gh * gw - 1);
                const int sy = s * (p / gw) + (Y - s * y), sx = s * (p % gw) + (X - s * x);
                const float4 v = src[((((long)k * B + b) * sh + sy) * sw + sx) * C4 + c4];
                a0 = __fadd_rn(a0, v.x), a1 = __fadd_rn(a1, v.y), a2 = __fadd_rn(a2, v.z), a3 = __fadd_rn(a3, v.w);
            }
        }
        const float cnt = (float)((y1 - y0 + 1) * (x1 - x0 + 1));
        reinterpret_cast<float4 *>(out)[i] = make_float4(__fdiv_rn(a0, cnt), __fdiv_rn(a1, cnt), __fdiv_rn(a2, cnt), __fdiv_rn(a3, cnt));
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Coefficients.  wts [B][gh][gw]; padded map Wp [h][w] = wts clamped (replicate pad by 1).  Output pixel (Y, X) of scale s:
// source coordinate Y (h - 1) / (s h - 1) (align_corners; 0 when s h == 1), taps floor - 1 .. floor + 2 clamped to the map,
// torch's cubic convolution coefficients with A = -0.75.  One thread per output pixel of the three scales together.
// ---------------------------------------------------------------------------------------------------------------
__device__ inline void cubic_taps(double t, double c[4])
{
    const double A = -0.75;
    const double u0 = t + 1.0, u3 = 2.0 - t, u2 = 1.0 - t;
    c[0] = ((A * u0 - 5.0 * A) * u0 + 8.0 * A) * u0 - 4.0 * A;
    c[1] = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0;
    c[2] = ((A + 2.0) * u2 - (A + 3.0)) * u2 * u2 + 1.0;
    c[3] = ((A * u3 - 5.0 * A) * u3 + 8.0 * A) * u3 - 4.0 * A;
}

__global__ __launch_bounds__(256) void coeff_kernel(const float *__restrict__ wts, float *__restrict__ c1, float *__restrict__ c2,
                                                    float *__restrict__ c4, int B, int h, int w)
{
    const int gh = h - 2, gw = w - 2;
    const long n1 = (long)B * h * w, total = 21 * n1;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int s;
        long j;
        float *dst;
        if (i < n1) s = 1, j = i, dst = c1;
        else if (i < 5 * n1) s = 2, j = i - n1, dst = c2;
        else s = 4, j = i - 5 * n1, dst = c4;
        if (!dst) continue;
        const int sh = s * h, sw = s * w;
        const int X = (int)(j % sw);
        const long r = j / sw;
        const int Y = (int)(r % sh);
        const int b = (int)(r / sh);
        const double ry = sh > 1 ? (double)Y * ((double)(h - 1) / (double)(sh - 1)) : 0.0;
        const double rx = sw > 1 ? (double)X * ((double)(w - 1) / (double)(sw - 1)) : 0.0;
        const int iy = (int)floor(ry), ix = (int)floor(rx);
        double cy[4], cx[4];
        cubic_taps(ry - iy, cy);
        cubic_taps(rx - ix, cx);
        const float *wb = wts + (long)b * gh * gw;
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int py = min(max(iy - 1 + a, 0), h - 1);          // row of the padded map
            const int qy = min(max(py - 1, 0), gh - 1);             // row of wts behind the replicate pad
            double row = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int px = min(max(ix - 1 + e, 0), w - 1);
                const int qx = min(max(px - 1, 0), gw - 1);
                row += cx[e] * (double)wb[(long)qy * gw + qx];
            }
            acc += cy[a] * row;
        }
        dst[j] = (float)(1.0 / (1.0 + exp(20.0 * acc - 0.65)));
    }
}

// Fc[n][p][:] = F[n][p][:] * coeff[n][p]: one thread per pixel and float4 of channels
__global__ __launch_bounds__(256) void scale_kernel(const float *__restrict__ f, const float *__restrict__ coeff, float *__restrict__ out, int C4,
                                                    long total)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const float c = coeff[i / C4];
        const float4 v = reinterpret_cast<const float4 *>(f)[i];
        reinterpret_cast<float4 *>(out)[i] = make_float4(v.x * c, v.y * c, v.z * c, v.w * c);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Criterion.  Block (b, l) of MREFSR_TEXTURE_CRIT_BLOCKS per layer: thread t adds the squares (gx - gm)^2 of elements 256 b + t,
// + 256 BLOCKS, .. in double, the block in a fixed tree -> partial[l][b].  Finish: norm_l = sqrt(the partials added in block order);
// then one thread: term_l = norm_l / 4 / D_l, total = ((sum_l term_l) / 3) * loss_weight in
// fp32, the layers in the given order -- the reference's `losses += ...; losses / 3.; * loss_weight`.
// ---------------------------------------------------------------------------------------------------------------
struct CritArgs {
    const float *gx[MREFSR_TEXTURE_MAX_LAYERS], *gm[MREFSR_TEXTURE_MAX_LAYERS];
    long n[MREFSR_TEXTURE_MAX_LAYERS];
    float div[MREFSR_TEXTURE_MAX_LAYERS];
    int n_layers;
    float loss_weight;
};

__global__ __launch_bounds__(256) void crit_kernel(const CritArgs a, double *__restrict__ partial)
{
    __shared__ double red[256];
    const int l = blockIdx.y;
    const float *gx = a.gx[l], *gm = a.gm[l];
    double s = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n[l]; i += (long)MREFSR_TEXTURE_CRIT_BLOCKS * 256) {
        const double d = (double)(gx[i] - gm[i]);
        s += d * d;
    }
    s = mrefsr::block_sum<256>(red, s);
    if (threadIdx.x == 0) partial[l * MREFSR_TEXTURE_CRIT_BLOCKS + blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void crit_finish_kernel(const CritArgs a, const double *__restrict__ partial, float *__restrict__ norms,
                                                         float *__restrict__ terms, float *__restrict__ total)
{
    __shared__ float nl[MREFSR_TEXTURE_MAX_LAYERS];
    const int l = threadIdx.x;
    if (l < a.n_layers) {
        double s = 0.0;
        for (int b = 0; b < MREFSR_TEXTURE_CRIT_BLOCKS; ++b) s += partial[l * MREFSR_TEXTURE_CRIT_BLOCKS + b];
        nl[l] = norms[l] = (float)sqrt(s);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float t = 0.f;
    for (int k = 0; k < a.n_layers; ++k) {
        const float term = __fdiv_rn(__fdiv_rn(nl[k], 4.0f), a.div[k]);
        terms[k] = term;
        t = __fadd_rn(t, term);
    }
    *total = __fmul_rn(__fdiv_rn(t, 3.0f), a.loss_weight);
}

// ---------------------------------------------------------------------------------------------------------------
// Backward of one layer: dF[n][p][j] (+)= coeff[n][p] * sc2 * sum_k Fc[n][p][k] (Gx - Gm)[n][k][j],  sc2 = 2 sc: the tile body of
// gram.h with the Gram difference itself as its A operand.  The scalar factor is applied behind the sums (the differences go
// through the MFMA unscaled: sc is ~1e-20 at the training sizes); norm == 0: exactly zero, whatever the sums hold -- torch's norm
// backward at 0.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gram_bwd_kernel(const float *__restrict__ fc, const float *__restrict__ gx, const float *__restrict__ gm,
                                                       const float *__restrict__ coeff, const float *__restrict__ norm,
                                                       const float *__restrict__ gup, float *__restrict__ df, int HW, int C, float scale,
                                                       int accumulate, unsigned int *__restrict__ amax_bits)
{
    const float nrm = *norm;
    const float up = gup ? *gup : 1.0f;
    const float sc2 = nrm == 0.f ? 0.f : 2.f * ((up * scale) / nrm);
    mrefsr::gram::bwd_tile(fc, gx, gm, df, HW, C, accumulate, amax_bits, [](const float d) { return d; },
                           [coeff, sc2](const long px) { return coeff[px] * sc2; }, nrm == 0.f);
}

}  // namespace

MREFSR_EXPORT int mrefsr_texture_select_f32(const int64_t *idx, const float *val, const int32_t *valid_bits, int32_t *sel, float *weights,
                                            int32_t *pidx, int K, int B, int64_t P, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(idx && val && sel && weights && pidx, "texture_select: null pointer");
    MREFSR_REQUIRE(K >= 1 && K <= 32 && B >= 1 && P >= 1 && (long)B * P < (1l << 31), "texture_select: K=%d B=%d P=%ld (K in 1..32)", K, B,
                   (long)P);
    const long total = (long)B * P;
    hipLaunchKernelGGL(select_kernel, dim3(grid_of((total + 255) / 256, 16384)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long *>(idx), val, valid_bits, sel, weights, pidx, K, B, (long)P);
    return mrefsr::check_launch("texture_select");
}

MREFSR_EXPORT int mrefsr_texture_swap_nhwc_f32(const float *feat, const int32_t *sel, const int32_t *pidx, float *out, int K, int B, int h, int w,
                                               int s, int C, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(feat && sel && pidx && out, "texture_swap_nhwc: null pointer");
    MREFSR_REQUIRE(K >= 1 && B >= 1 && h >= 3 && w >= 3 && s >= 1 && C > 0 && C % 4 == 0, "texture_swap_nhwc: K=%d B=%d h=%d w=%d s=%d C=%d "
                   "(h, w >= 3, C %% 4 == 0)", K, B, h, w, s, C);
    MREFSR_REQUIRE((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(out)) % 16 == 0, "texture_swap_nhwc: pointers must be "
                   "16-byte aligned");
    MREFSR_REQUIRE((long)s * h < 32768 && (long)s * w < 32768, "texture_swap_nhwc: map of %ld x %ld", (long)s * h, (long)s * w);
    const long total = (long)B * s * h * s * w * (C / 4);
    hipLaunchKernelGGL(swap_kernel, dim3(grid_of((total + 255) / 256, 65536)), dim3(256), 0, (hipStream_t)stream, feat, sel, pidx, out, K, B, h, w,
                       s, C / 4, total);
    return mrefsr::check_launch("texture_swap_nhwc");
}

MREFSR_EXPORT int mrefsr_texture_coeff_f32(const float *weights, float *c1, float *c2, float *c4, int B, int h, int w, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(weights && (c1 || c2 || c4), "texture_coeff: null pointer");
    MREFSR_REQUIRE(B >= 1 && h >= 3 && w >= 3 && (long)B * h * w < (1l << 26), "texture_coeff: B=%d h=%d w=%d (h, w >= 3)", B, h, w);
    const long total = 21l * B * h * w;
    hipLaunchKernelGGL(coeff_kernel, dim3(grid_of((total + 255) / 256, 16384)), dim3(256), 0, (hipStream_t)stream, weights, c1, c2, c4, B, h, w);
    return mrefsr::check_launch("texture_coeff");
}

MREFSR_EXPORT int mrefsr_texture_scale_nhwc_f32(const float *f, const float *coeff, float *out, int64_t n_px, int C, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(f && coeff && out, "texture_scale_nhwc: null pointer");
    MREFSR_REQUIRE(n_px >= 1 && C > 0 && C % 4 == 0, "texture_scale_nhwc: n_px=%ld C=%d (C %% 4 == 0)", (long)n_px, C);
    MREFSR_REQUIRE((reinterpret_cast<uintptr_t>(f) | reinterpret_cast<uintptr_t>(out)) % 16 == 0, "texture_scale_nhwc: pointers must be "
                   "16-byte aligned");
    const long total = (long)n_px * (C / 4);
    hipLaunchKernelGGL(scale_kernel, dim3(grid_of((total + 255) / 256, 65536)), dim3(256), 0, (hipStream_t)stream, f, coeff, out, C / 4, total);
    return mrefsr::check_launch("texture_scale_nhwc");
}

MREFSR_EXPORT int mrefsr_texture_crit_f32(const mrefsr_texture_layer *layers, int n_layers, float loss_weight, double *partial, float *norms,
                                          float *terms, float *total, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(layers && partial && norms && terms && total, "texture_crit: null pointer");
    MREFSR_REQUIRE(n_layers >= 1 && n_layers <= MREFSR_TEXTURE_MAX_LAYERS, "texture_crit: 1..%d layers, got %d", MREFSR_TEXTURE_MAX_LAYERS,
                   n_layers);
    CritArgs a = {};
    for (int l = 0; l < n_layers; ++l) {
        MREFSR_REQUIRE(layers[l].gx && layers[l].gm && layers[l].n > 0 && layers[l].div > 0.f, "texture_crit: layer %d: null pointer, n=%ld or "
                       "div=%g", l, (long)layers[l].n, (double)layers[l].div);
        a.gx[l] = layers[l].gx, a.gm[l] = layers[l].gm, a.n[l] = (long)layers[l].n, a.div[l] = layers[l].div;
    }
    a.n_layers = n_layers, a.loss_weight = loss_weight;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(crit_kernel, dim3(MREFSR_TEXTURE_CRIT_BLOCKS, n_layers), dim3(256), 0, st, a, partial);
    hipLaunchKernelGGL(crit_finish_kernel, dim3(1), dim3(64), 0, st, a, (const double *)partial, norms, terms, total);
    return mrefsr::check_launch("texture_crit");
}

MREFSR_EXPORT int mrefsr_texture_gram_bwd_nhwc_f32(const float *fc, const float *gx, const float *gm, const float *coeff, const float *norm,
                                                   const float *gup, float *df, int N, int HW, int C, float scale, int accumulate, float *amax,
                                                   mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(fc && gx && gm && coeff && norm && df, "texture_gram_bwd_nhwc: null pointer");
    if (const int e = mrefsr::gram::check_gram("texture_gram_bwd_nhwc", N, HW, C)) return e;
    hipLaunchKernelGGL(gram_bwd_kernel, dim3((HW + 63) / 64, C / 64, N), dim3(256), 0, (hipStream_t)stream, fc, gx, gm, coeff, norm, gup, df, HW, C,
                       scale, accumulate ? 1 : 0, reinterpret_cast<unsigned int *>(amax));
    return mrefsr::check_launch("texture_gram_bwd_nhwc");
}
