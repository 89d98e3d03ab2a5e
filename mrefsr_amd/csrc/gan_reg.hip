// The R1 regulariser of the adversarial step (basicsr/losses/losses.py:391-405, r1_penalty; applied lazily in
// basicsr/models/stylegan2_model.py:208-219): grad.pow(2).view(B, -1).sum(1) of the discriminator's input gradient and the
// backward of that sum, 2 gs[b] g[b][i].  The discriminator's own double backward runs on the nodes that WGAN-GP uses
// (archs/nhwc_*disc.py); these two kernels replace torch's pow / sum / mul launches around it and fix the summation order.
//
// Forward, two launches.  g is `batch` contiguous rows of n floats; a row is cut into T = ceil((n + 3) / 1024) chunks of 1024
// elements (256 lanes x 4), row b's chunks are shared by R = min(ceil(T / 2), 512) blocks, block r taking the contiguous range
// [T r / R, T (r + 1) / R): the grid (R, batch) is a pure function of (batch, n).  Chunk boundaries are shifted by the row's own
// offset inside 16 bytes, so every full group of four elements is one aligned 16-byte load; the at most three elements in front of
// the first and behind the last such group take guarded 4-byte loads.  A lane squares its four elements in fp32, adds them as
// (q0 + q1) + (q2 + q3) (an absent element counts 0) and adds that to its fp32 accumulator: square, then add (-ffp-contract=off,
// Makefile).  The 256 lane sums are added in double -- the shuffle tree inside a wave, then the four waves in index order -- and
// the block writes ONE double into partial[b R + r].  r1_sqnorm_finalize_kernel (one 64-lane block per row) adds the row's R
// partials in ascending block order in double and writes out[b] rounded to fp32.  No atomics, no ticket: the same bits from run
// to run.  A square that overflows fp32 is inf; inf and NaN elements reach out[b] as inf / NaN; nothing is clamped.
//
// Backward, one launch: gg[b][i] = fl32(fl32(2 gs[b]) g[b][i]) -- the factor 2 is exact, so this is one rounding per element and
// the bits of torch's g * (2 * gs).view(B, 1).  A pure streaming kernel on the same chunks: 16-byte accesses when g's and gg's rows
// share their offset inside 16 bytes, lane-contiguous 4-byte accesses otherwise, every access guarded by 0 <= i < n.
#include "common.h"

namespace {

constexpr int CHUNK = 1024;    // elements: 256 lanes x 4
constexpr int THREADS = 256;
constexpr int MAX_ROW_BLOCKS = 512;
constexpr int BWD_ROW_BLOCKS = 2048;
constexpr int FIN_THREADS = 64;

typedef float f32x4 __attribute__((ext_vector_type(4)));
// device-memory addresses: said so, they are accessed with global_* instead of flat_* instructions
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) double gf64;

__host__ __device__ inline long long row_chunks(const long long n) { return (n + 3 + CHUNK - 1) / CHUNK; }

inline int row_blocks(const long long n)
{
    const long long t = row_chunks(n), r = (t + 1) / 2;
    return (int)(r < 1 ? 1 : (r > MAX_ROW_BLOCKS ? MAX_ROW_BLOCKS : r));
}

__global__ __launch_bounds__(THREADS) void r1_sqnorm_partial_kernel(const float *__restrict__ g_, const long long n,
                                                                    double *__restrict__ partial_)
{
    const int tid = threadIdx.x;
    const long long b = blockIdx.y;
    const gf32 *const row = (const gf32 *)g_ + b * n;
    const long long total = row_chunks(n);
    const long long c0 = total * blockIdx.x / gridDim.x, c1 = total * (blockIdx.x + 1) / gridDim.x;
    const int a = (int)(((size_t)row >> 2) & 3);   // elements by which the row lies behind a 16-byte boundary
    float acc = 0.f;
    for (long long c = c0; c < c1; ++c) {
        const long long i0 = c * CHUNK + 4 * tid - a;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (i0 >= 0 && i0 + 4 <= n) {
            v = *(const gf32x4 *)(row + i0);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long i = i0 + e;
                if (i >= 0 && i < n) v[e] = row[i];
            }
        }
        const float q0 = v[0] * v[0], q1 = v[1] * v[1], q2 = v[2] * v[2], q3 = v[3] * v[3];
        acc += (q0 + q1) + (q2 + q3);
    }
    __shared__ double wsum[THREADS / 64];
    const double s = mrefsr::block_sum_by_waves<THREADS>((double)acc, wsum);
    if (tid == 0) ((gf64 *)partial_)[b * gridDim.x + blockIdx.x] = s;
}

// one block per row: the row's partials in ascending block order
__global__ __launch_bounds__(FIN_THREADS) void r1_sqnorm_finalize_kernel(const double *__restrict__ partial_, const int row_blocks,
                                                                         float *__restrict__ out)
{
    __shared__ double part[MAX_ROW_BLOCKS];
    const gf64 *const partial = (const gf64 *)partial_ + (long long)blockIdx.x * row_blocks;
    for (int i = threadIdx.x; i < row_blocks; i += FIN_THREADS) part[i] = partial[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < row_blocks; ++i) s += part[i];
    ((gf32 *)out)[blockIdx.x] = (float)s;
}

__global__ __launch_bounds__(THREADS) void r1_sqnorm_bwd_kernel(const float *__restrict__ g_, const float *__restrict__ gs,
                                                                const long long n, float *__restrict__ gg_)
{
    const int tid = threadIdx.x;
    const long long b = blockIdx.y;
    const gf32 *const g = (const gf32 *)g_ + b * n;
    gf32 *const gg = (gf32 *)gg_ + b * n;
    const float f = 2.f * ((const gf32 *)gs)[b];
    const long long total = row_chunks(n);
    const long long c0 = total * blockIdx.x / gridDim.x, c1 = total * (blockIdx.x + 1) / gridDim.x;
    const bool vec = ((((size_t)g) ^ ((size_t)gg)) & 15) == 0;
    const int a = vec ? (int)(((size_t)g >> 2) & 3) : 0;
    for (long long c = c0; c < c1; ++c) {
        const long long i0 = c * CHUNK + 4 * tid - a;
        if (vec && i0 >= 0 && i0 + 4 <= n) {
            f32x4 v = *(const gf32x4 *)(g + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = f * v[e];
            *(gf32x4 *)(gg + i0) = v;
            continue;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // rows of 16-byte groups: this lane's group is cut by the row's start or end; otherwise lane-contiguous words
            const long long i = vec ? i0 + e : c * CHUNK + e * THREADS + tid;
            if (i >= 0 && i < n) gg[i] = f * g[i];
        }
    }
}

bool shape_ok(const int batch, const int64_t n) { return batch > 0 && batch <= 65535 && n > 0 && n <= ((int64_t)1 << 40); }

}  // namespace

MREFSR_EXPORT int mrefsr_r1_sqnorm_row_blocks(int64_t n) { return n <= 0 || n > ((int64_t)1 << 40) ? -1 : row_blocks(n); }

MREFSR_EXPORT int64_t mrefsr_r1_sqnorm_workspace_bytes(int batch, int64_t n)
{
    return shape_ok(batch, n) ? (int64_t)batch * row_blocks(n) * (int64_t)sizeof(double) : -1;
}

MREFSR_EXPORT int mrefsr_r1_sqnorm_f32(const float *g, int batch, int64_t n, float *out, void *workspace, int64_t workspace_bytes,
                                       mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(shape_ok(batch, n), "r1_sqnorm: batch=%d (1..65535) n=%lld (1..2^40)", batch, (long long)n);
    MREFSR_REQUIRE(g && out && ((size_t)g & 3) == 0 && ((size_t)out & 3) == 0, "r1_sqnorm: g=%p out=%p (4-byte aligned)", (const void *)g,
                   (const void *)out);
    MREFSR_REQUIRE(workspace && workspace_bytes >= mrefsr_r1_sqnorm_workspace_bytes(batch, n) && ((size_t)workspace & 7) == 0,
                   "r1_sqnorm: workspace=%p (8-byte aligned) of %lld bytes, %lld needed", workspace, (long long)workspace_bytes,
                   (long long)mrefsr_r1_sqnorm_workspace_bytes(batch, n));
    const int rb = row_blocks(n);
    hipLaunchKernelGGL(r1_sqnorm_partial_kernel, dim3(rb, batch), dim3(THREADS), 0, (hipStream_t)stream, g, (long long)n, (double *)workspace);
    hipLaunchKernelGGL(r1_sqnorm_finalize_kernel, dim3(batch), dim3(FIN_THREADS), 0, (hipStream_t)stream, (const double *)workspace, rb, out);
    return mrefsr::check_launch("r1_sqnorm");
}

MREFSR_EXPORT int mrefsr_r1_sqnorm_bwd_f32(const float *g, const float *gs, int batch, int64_t n, float *gg, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(shape_ok(batch, n), "r1_sqnorm_bwd: batch=%d (1..65535) n=%lld (1..2^40)", batch, (long long)n);
    MREFSR_REQUIRE(g && gs && gg && (((size_t)g | (size_t)gs | (size_t)gg) & 3) == 0, "r1_sqnorm_bwd: g=%p gs=%p gg=%p (4-byte aligned)",
                   (const void *)g, (const void *)gs, (const void *)gg);
    const long long t = row_chunks(n);
    const int rb = (int)(t < BWD_ROW_BLOCKS ? t : BWD_ROW_BLOCKS);
    hipLaunchKernelGGL(r1_sqnorm_bwd_kernel, dim3(rb, batch), dim3(THREADS), 0, (hipStream_t)stream, g, gs, (long long)n, gg);
    return mrefsr::check_launch("r1_sqnorm_bwd");
}
