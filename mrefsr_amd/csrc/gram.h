// What the Gram kernels of the style term (percep.hip) and of the texture loss (texture.hip) share: the launchers' shape check and the
// f32-MFMA tile body of both gram_bwd_kernels.  Each file compiles bwd_tile under its own flags (texture.hip: -ffp-contract=off) and
// keeps its scalar prologue, whose arithmetic is the kernel's contract; a body moved here must leave each caller the bits it gave in
// place (tests/test_gram_bits_gpu.py pins them to the library from before this header).
// Not here, on purpose: tap_crit_kernel accumulates with an explicitly rounded __fadd_rn (torch's bits), cx_grad_finish_kernel with a
// + that its file's flags may contract with the multiply in front of it, cx_subsample_bwd_kernel adds in the other order -- one
// "store the gradient" helper would have to branch on its caller.  Nor the other private f32x4 typedefs of csrc/.
#pragma once
#include "common.h"

namespace mrefsr::gram {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// N is gridDim.z of gram_nhwc, gram_bwd_nhwc and texture_gram_bwd_nhwc; a tile is 64 channels wide
inline int check_gram(const char *who, int N, int HW, int C)
{
    MREFSR_REQUIRE(N > 0 && N < 65536 && HW > 0 && C > 0 && C % 64 == 0, "%s: N=%d HW=%d C=%d (N in 1..65535, HW > 0, C a multiple of 64)",
                   who, N, HW, C);
    return MREFSR_OK;
}

// dF[n][p][j] (+)= fac_of(n HW + p) * sum_k F[n][p][k] a_of(Gx - Gy)[n][k][j]: grid ((HW + 63) / 64, C / 64, N), 256 threads.
// Computed transposed, out^T[j][p] = sum_k A[j][k] F[p][k]: A = a_of(Gx - Gy) (rows j; symmetric), B[k][p] = F[p][k].  A lane holds
// a float4 of F[p0 + (l & 15)][k0 + 4 (l >> 4) .. + 3] and feeds element e to the e-th MFMA of the 16-channel step, so the MFMA's
// local k = l >> 4 is channel k0 + 4 (l >> 4) + e -- the A operand takes the same channel.  Wave = 16 pixels x 64 columns (four
// accumulators); block = 4 waves = 64 pixels.  D: column (p) = lane & 15, row (j) = 4 (lane >> 4) + r: a float4 of dF's row.
// fac_of is called for pixels inside the map only; zero: dF gets exact zeros whatever the sums hold; max |dF| -> amax_bits (or NULL).
template <class AOp, class FacOp>
__device__ __forceinline__ void bwd_tile(const float *__restrict__ f, const float *__restrict__ gx, const float *__restrict__ gy,
                                         float *__restrict__ df, const int HW, const int C, const int accumulate,
                                         unsigned int *__restrict__ amax_bits, const AOp a_of, const FacOp fac_of, const bool zero)
{
    const int n = blockIdx.z, jb = blockIdx.y * 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p0 = (blockIdx.x * 4 + wave) * 16;
    const int kl = lane >> 4, cl = lane & 15;
    const float *fn = f + (long)n * HW * C;
    const float *gxn = gx + (long)n * C * C, *gyn = gy + (long)n * C * C;
    const int p = p0 + cl;
    const bool pok = p < HW;
    f32x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < C; k0 += 16) {
        const int kc = k0 + 4 * kl;
        const float4 fv = pok ? *reinterpret_cast<const float4 *>(fn + (long)p * C + kc) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float fe[4] = {fv.x, fv.y, fv.z, fv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long srow = (long)(kc + e) * C + jb + cl;   // A[k][j] = A[j][k]
#pragma unroll
            for (int b = 0; b < 4; ++b)
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_of(gxn[srow + 16 * b] - gyn[srow + 16 * b]), fe[e], acc[b], 0, 0, 0);
        }
    }
    // lane holds out[p0 + (l & 15)][jb + 16 b + 4 (l >> 4) + r]
    float amx = 0.f;
    if (pok) {
        const float cs = zero ? 0.f : fac_of((long)n * HW + p);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            float4 *dst = reinterpret_cast<float4 *>(df + ((long)n * HW + p) * C + jb + 16 * b + 4 * kl);
            float4 v = zero ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(cs * acc[b][0], cs * acc[b][1], cs * acc[b][2], cs * acc[b][3]);
            if (accumulate) {
                const float4 o = *dst;
                v.x += o.x, v.y += o.y, v.z += o.z, v.w += o.w;
            }
            *dst = v;
            amx = fmaxf(amx, amax4(v));
        }
    }
    if (amax_bits) publish_amax<false>(amax_bits, amx);   // max |dF|
}

}  // namespace mrefsr::gram
