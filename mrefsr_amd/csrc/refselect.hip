// Reference pools (ref_select): rank each sample's N candidate references by the matcher's winning correlations and
// gather the K best into the k-major stacks that the rest of the pass reads.
//   ref_select   val [N][B][P] -> scores [B][N], the K chosen candidates per sample in ascending n, the mask word over the K slots
//                (two launches: per-chunk partial sums / win counts, then one wave per sample that finishes, ranks and selects)
//   ref_gather   rows of `row_bytes` bytes copied by the selection table, zeros into unused slots (16-, 8- or 4-byte accesses)
// Built with -ffp-contract=off.  The order of the `mean` sum is spelled out below and depends on P alone:
//   chunk c = positions [1024 c, min(P, 1024 (c + 1)))  (MREFSR_REF_SELECT_CHUNK: 15 chunks per plane at LR 125 x 125);
//   thread t of the chunk's block: a_t = (((0 + v[1024 c + t]) + v[1024 c + t + 256]) + ...) over its <= 4 positions, ascending;
//   the block: a_t += a_{t + w} for w = 128, 64, .., 1 (all t < w);  the chunk's partial is a_0;
//   the sample's wave: S = ((0 + partial_0) + partial_1) + ..., ascending c;  score = S / (float)P, one correctly rounded division.
// No float atomics; the grid is a function of (N, B, P) only and no output bit depends on it.
#include "common.h"

namespace {

constexpr int CHUNK = MREFSR_REF_SELECT_CHUNK, THREADS = 256;

__device__ inline unsigned int pool_bits(const int *valid_bits, int b) { return valid_bits ? (unsigned int)valid_bits[b] : 0xffffffffu; }

// block (c, b, n): the partial sum of candidate n of sample b over chunk c, in the order stated above.  An absent candidate's plane
// is not read (its partial is not read either).
__global__ __launch_bounds__(THREADS) void mean_partial_kernel(const float *__restrict__ val, const int *__restrict__ valid_bits,
                                                               float *__restrict__ part, int B, long P, int chunks)
{
    __shared__ float red[THREADS];
    const int c = blockIdx.x, b = blockIdx.y, n = blockIdx.z;
    if (!((pool_bits(valid_bits, b) >> n) & 1u)) return;
    const float *v = val + ((long)n * B + b) * P;
    const long p1 = min(P, (long)(c + 1) * CHUNK);
    float a = 0.f;
#pragma unroll 4
    for (long p = (long)c * CHUNK + threadIdx.x; p < p1; p += THREADS) a = __fadd_rn(a, v[p]);
    a = mrefsr::block_sum<THREADS>(red, a);   // (additions alone: under -ffp-contract=off a plain + is __fadd_rn)
    if (threadIdx.x == 0) part[((long)n * B + b) * chunks + c] = a;
}

// block (c, b): per position of the chunk the present candidate with the largest val -- a later one replaces the best only when
// strictly greater (select_kernel of texture.hip: the lowest n among equal maxima), and a NaN never wins -- counted per candidate in
// LDS (integer atomics: exact in any order).  part [N][B][chunks] as int.
__global__ __launch_bounds__(THREADS) void wins_partial_kernel(const float *__restrict__ val, const int *__restrict__ valid_bits,
                                                               int *__restrict__ part, int N, int B, long P, int chunks)
{
    __shared__ int cnt[32];
    const int c = blockIdx.x, b = blockIdx.y;
    const unsigned int bits = pool_bits(valid_bits, b);
    if (threadIdx.x < 32) cnt[threadIdx.x] = 0;
    __syncthreads();
    const long p1 = min(P, (long)(c + 1) * CHUNK), plane = (long)B * P;
    for (long p = (long)c * CHUNK + threadIdx.x; p < p1; p += THREADS) {
        const float *v = val + (long)b * P + p;
        int best = -1;
        float bv = 0.f;
        for (int n = 0; n < N; ++n) {
            if (!((bits >> n) & 1u)) continue;
            const float x = v[(long)n * plane];
            if (x == x && (best < 0 || x > bv)) best = n, bv = x;
        }
        if (best >= 0) atomicAdd(&cnt[best], 1);
    }
    __syncthreads();
    if ((int)threadIdx.x < N) part[((long)threadIdx.x * B + b) * chunks + c] = cnt[threadIdx.x];
}

// m stands in front of n: the larger score, the lower index among equal ones; a NaN stands behind every number
__device__ inline bool before(float sm, int m, float sn, int n)
{
    const bool nan_m = sm != sm, nan_n = sn != sn;
    if (nan_m || nan_n) return nan_m == nan_n ? m < n : nan_n;
    return sm > sn || (sm == sn && m < n);
}

// one wave per sample, lane n = candidate n: finish the score, rank among the present candidates, keep the first K, emit them in
// ascending n (the slot of a kept candidate = the number of kept ones below it)
__global__ __launch_bounds__(64) void finish_kernel(const float *__restrict__ part, const int *__restrict__ valid_bits,
                                                    float *__restrict__ scores, int *__restrict__ sel, int *__restrict__ slot_bits, int N,
                                                    int B, long P, int K, int chunks, int mode)
{
    __shared__ float sc[64];
    const int b = blockIdx.x, n = threadIdx.x;
    const unsigned int bits = pool_bits(valid_bits, b);
    const bool valid = n < N && ((bits >> n) & 1u);
    float score = -INFINITY;
    if (valid) {
        const long row = ((long)n * B + b) * chunks;
        if (mode == MREFSR_REF_SCORE_MEAN) {
            float s = 0.f;
            for (int c = 0; c < chunks; ++c) s = __fadd_rn(s, part[row + c]);
            score = __fdiv_rn(s, (float)P);
        } else {
            const int *pi = reinterpret_cast<const int *>(part);
            int s = 0;
            for (int c = 0; c < chunks; ++c) s += pi[row + c];
            score = (float)s;   // (exact: P <= 2^24)
        }
    }
    sc[n] = score;
    __syncthreads();
    int rank = 0;
    if (valid)
        for (int m = 0; m < N; ++m)
            if (m != n && ((bits >> m) & 1u) && before(sc[m], m, score, n)) ++rank;
    const bool chosen = valid && rank < K;
    const unsigned long long kept = __ballot(chosen);
    const int count = __popcll(kept);
    if (chosen) sel[(long)b * K + __popcll(kept & ((1ull << n) - 1ull))] = n;
    if (n < K && n >= count) sel[(long)b * K + n] = -1;
    if (n == 0) slot_bits[b] = (int)(count >= 32 ? 0xffffffffu : (1u << count) - 1u);
    if (n < N) scores[(long)b * N + n] = score;
}

// dst row k B + b <- src row sel[b][k] B + b, zeros where sel[b][k] is not in 0..N-1; rows of row_v elements of V
template <typename V>
__global__ __launch_bounds__(THREADS) void gather_kernel(const V *__restrict__ src, V *__restrict__ dst, const int *__restrict__ sel, int N,
                                                         int B, int K, long row_v)
{
    const int row = blockIdx.y, k = row / B, b = row - k * B;
    const int s = sel[(long)b * K + k];
    const bool ok = s >= 0 && s < N;
    const V *sp = src + ((long)(ok ? s : 0) * B + b) * row_v;
    V *dp = dst + (long)row * row_v;
    V zero = {};
#pragma unroll 4
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < row_v; i += (long)gridDim.x * THREADS) dp[i] = ok ? sp[i] : zero;
}

template <typename V>
void launch_gather(const void *src, void *dst, const int *sel, int N, int B, int K, long row_bytes, hipStream_t st)
{
    const long row_v = row_bytes / (long)sizeof(V);
    const long bx = (row_v + 4 * THREADS - 1) / (4 * THREADS);   // four accesses per thread in flight
    hipLaunchKernelGGL(gather_kernel<V>, dim3((unsigned)(bx < 1 ? 1 : (bx < 4096 ? bx : 4096)), K * B), dim3(THREADS), 0, st,
                       static_cast<const V *>(src), static_cast<V *>(dst), sel, N, B, K, row_v);
}

}  // namespace

MREFSR_EXPORT int64_t mrefsr_ref_select_workspace_bytes(int N, int B, int64_t P)
{
    if (N < 1 || B < 1 || P < 1) return -1;
    return 4 * (int64_t)N * B * ((P + MREFSR_REF_SELECT_CHUNK - 1) / MREFSR_REF_SELECT_CHUNK);
}

MREFSR_EXPORT int mrefsr_ref_select_f32(const float *val, const int32_t *valid_bits, float *scores, int32_t *sel, int32_t *slot_bits, int N,
                                        int B, int64_t P, int K, int mode, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(val && scores && sel && slot_bits && workspace, "ref_select: null pointer");
    MREFSR_REQUIRE(N >= 1 && N <= 32 && K >= 1 && K <= 32 && B >= 1 && B <= 65535 && P >= 1 && P <= (1l << 24),
                   "ref_select: N=%d B=%d P=%ld K=%d (N, K in 1..32, B <= 65535, P <= 2^24)", N, B, (long)P, K);
    MREFSR_REQUIRE(mode == MREFSR_REF_SCORE_MEAN || mode == MREFSR_REF_SCORE_WINS, "ref_select: mode %d is neither mean nor wins", mode);
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_ref_select_workspace_bytes(N, B, P), "ref_select: workspace of %ld bytes, %ld needed",
                   (long)workspace_bytes, (long)mrefsr_ref_select_workspace_bytes(N, B, P));
    const int chunks = (int)((P + CHUNK - 1) / CHUNK);
    hipStream_t st = (hipStream_t)stream;
    if (mode == MREFSR_REF_SCORE_MEAN)
        hipLaunchKernelGGL(mean_partial_kernel, dim3(chunks, B, N), dim3(THREADS), 0, st, val, valid_bits, static_cast<float *>(workspace), B,
                           (long)P, chunks);
    else
        hipLaunchKernelGGL(wins_partial_kernel, dim3(chunks, B), dim3(THREADS), 0, st, val, valid_bits, static_cast<int *>(workspace), N, B,
                           (long)P, chunks);
    hipLaunchKernelGGL(finish_kernel, dim3(B), dim3(64), 0, st, static_cast<const float *>(workspace), valid_bits, scores, sel, slot_bits, N, B,
                       (long)P, K, chunks, mode);
    return mrefsr::check_launch("ref_select");
}

MREFSR_EXPORT int mrefsr_ref_gather(const void *src, void *dst, const int32_t *sel, int N, int B, int K, int64_t row_bytes,
                                    mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(src && dst && sel, "ref_gather: null pointer");
    MREFSR_REQUIRE(N >= 1 && N <= 32 && K >= 1 && K <= 32 && B >= 1 && (long)K * B <= 65535 && row_bytes >= 4 && row_bytes % 4 == 0,
                   "ref_gather: N=%d B=%d K=%d row_bytes=%ld (N, K in 1..32, K B <= 65535, rows of whole 4-byte words)", N, B, K,
                   (long)row_bytes);
    const uintptr_t align = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)row_bytes;
    MREFSR_REQUIRE(align % 4 == 0, "ref_gather: pointers must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (align % 16 == 0) launch_gather<uint4>(src, dst, sel, N, B, K, (long)row_bytes, st);
    else if (align % 8 == 0) launch_gather<uint2>(src, dst, sel, N, B, K, (long)row_bytes, st);
    else launch_gather<unsigned int>(src, dst, sel, N, B, K, (long)row_bytes, st);
    return mrefsr::check_launch("ref_gather");
}
