// The parameter update of the training step: Adam (torch.optim.Adam's arithmetic; the reference builds a plain Adam,
// multi_ref_restoration_model.py:90-104) and the exponential moving average of net_g (base_model.py:75-82, model_ema), for every
// tensor of an optimiser in ONE launch driven by a job table in device memory -- the pattern of mrefsr_conv_pack_weights_multi_f32.
//
// A pure streaming kernel: 7 words of traffic per element for Adam (p, g, m, v read; p, m, v written), 2 more for the EMA copy,
// which is written in the same pass that has the new parameter in a register.  The table's elements are cut into chunks of 1024
// (one 16-byte access per lane and stream); the grid is fixed, block b takes the contiguous chunk range [T b / G, T (b + 1) / G)
// of the T chunks and walks the jobs it meets, so neither the number of tensors nor their sizes shape the launch, no block waits
// for another and nothing is accumulated: no atomics, the same bits from run to run.  Latency is hidden by occupancy (8 blocks of
// 4 waves per CU, 4-5 independent 16-byte loads each) rather than by unrolling across chunk -- and job -- boundaries.
//
// Alignment: a tensor may start at any 4-byte boundary.  When all streams of a job share their offset inside 16 bytes (always, for
// tensors that are allocations of their own), chunk boundaries are shifted by that offset so that every full group of four
// elements is one aligned 16-byte access; the at most three elements in front of the first and behind the last such group, and
// jobs whose streams disagree, take 4-byte accesses.  Every access is guarded by 0 <= i < n of its job.
//
// Built with -ffp-contract=off (Makefile): the roundings are the ones written here, in the 16-byte and the 4-byte path alike.
#include "common.h"

namespace {

constexpr int CHUNK = 1024;    // elements: 256 lanes x 4
constexpr int THREADS = 256;
constexpr int GRID = 2048;     // 8 blocks per CU on 256 CUs

typedef float f32x4 __attribute__((ext_vector_type(4)));
// the table's pointers are device-memory addresses: said so, they are accessed with global_* instead of flat_* instructions
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

__host__ __device__ inline int job_chunks(const long long n) { return n > 0 ? (int)((n + 3 + CHUNK - 1) / CHUNK) : 0; }

struct Coef {
    float b1, omb1, b2, omb2, step_size, bc2_sqrt, eps, wd;
};

__device__ inline double powi(double b, long long e)
{
    double r = 1.0;
    for (; e > 0; e >>= 1, b *= b)
        if (e & 1) r *= b;
    return r;
}

// torch's _fused_adam: the bias corrections in double from the double hyper-parameters, the element arithmetic in float
__device__ inline Coef group_coef(const mrefsr_adam_group &g)
{
    Coef c;
    c.b1 = (float)g.beta1;
    c.omb1 = (float)(1.0 - g.beta1);
    c.b2 = (float)g.beta2;
    c.omb2 = (float)(1.0 - g.beta2);
    c.step_size = (float)(g.lr / (1.0 - powi(g.beta1, g.step)));
    c.bc2_sqrt = (float)sqrt(1.0 - powi(g.beta2, g.step));
    c.eps = (float)g.eps;
    c.wd = (float)g.weight_decay;
    return c;
}

__device__ __forceinline__ void adam1(float &p, float g, float &m, float &v, const Coef &c)
{
    if (c.wd != 0.f) g = fmaf(c.wd, p, g);
    m = fmaf(c.b1, m, c.omb1 * g);
    v = fmaf(c.b2, v, c.omb2 * g * g);
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p -= c.step_size * m / denom;
}

// (decay 0 is the reference's copy, model_ema(0): the callers store p's bits then, whatever the EMA tensor held)
__device__ __forceinline__ float ema1(const float e, const float p, const float d, const float a) { return fmaf(e, d, p * a); }

template <bool ADAM>
__global__ __launch_bounds__(THREADS) void optim_multi_kernel(const mrefsr_optim_job *__restrict__ jobs, const int n_jobs,
                                                               const mrefsr_adam_group *__restrict__ groups, const int n_groups,
                                                               const float ema_d, const float ema_a)
{
    const long long total = (long long)jobs[n_jobs - 1].first_chunk + job_chunks(jobs[n_jobs - 1].n);
    const long long c0 = total * blockIdx.x / gridDim.x, c1 = total * (blockIdx.x + 1) / gridDim.x;
    if (c0 >= c1) return;
    int j = 0;
    for (int hi = n_jobs - 1; j < hi;) {   // the last job whose first chunk is <= c0
        const int mid = (j + hi + 1) >> 1;
        if (jobs[mid].first_chunk <= c0) j = mid; else hi = mid - 1;
    }
    const int tid = threadIdx.x;
    for (long long c = c0; c < c1;) {
        while (j + 1 < n_jobs && jobs[j + 1].first_chunk <= c) ++j;
        const mrefsr_optim_job job = jobs[j];
        const long long jend = j + 1 < n_jobs ? (long long)jobs[j + 1].first_chunk : total;
        const long long cend = c1 < jend ? c1 : jend;
        const long long n = job.n;
        gf32 *const p = (gf32 *)job.p, *const ema = (gf32 *)job.ema, *const pm = (gf32 *)job.m, *const pv2 = (gf32 *)job.v;
        const gf32 *const pg = (const gf32 *)job.g;
        const bool step = ADAM && job.g && job.m && job.v && job.group >= 0 && job.group < n_groups;   // torch skips .grad None
        if (!p || (!step && !ema)) { c = cend; continue; }
        Coef cf = {};
        if (ADAM && step) cf = group_coef(groups[job.group]);
        size_t mis = 0;   // bits in which a stream's address differs from p's
        if (step) mis |= ((size_t)job.g ^ (size_t)p) | ((size_t)job.m ^ (size_t)p) | ((size_t)job.v ^ (size_t)p);
        if (ema) mis |= (size_t)ema ^ (size_t)p;
        const bool vec = (mis & 15) == 0;
        const int a = vec ? (int)(((size_t)p >> 2) & 3) : 0;   // elements by which p lies behind a 16-byte boundary
        for (; c < cend; ++c) {
            const long long k = c - job.first_chunk;
            const long long i0 = k * CHUNK + 4 * tid - a;
            if (vec && i0 >= 0 && i0 + 4 <= n) {
                f32x4 pv = *(const gf32x4 *)(p + i0), ev = {};
                if (ema && ema_d != 0.f) ev = *(const gf32x4 *)(ema + i0);
                if (step) {
                    const f32x4 gv = *(const gf32x4 *)(pg + i0);
                    f32x4 mv = *(const gf32x4 *)(pm + i0), vv = *(const gf32x4 *)(pv2 + i0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float pe = pv[e], me = mv[e], ve = vv[e];
                        adam1(pe, gv[e], me, ve, cf);
                        pv[e] = pe, mv[e] = me, vv[e] = ve;
                    }
                    *(gf32x4 *)(p + i0) = pv;
                    *(gf32x4 *)(pm + i0) = mv;
                    *(gf32x4 *)(pv2 + i0) = vv;
                }
                if (ema) {
                    if (ema_d != 0.f) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) pv[e] = ema1(ev[e], pv[e], ema_d, ema_a);
                    }
                    *(gf32x4 *)(ema + i0) = pv;
                }
                continue;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // a job of 16-byte groups: this lane's group is cut by the tensor's start or end; otherwise lane-contiguous words
                const long long i = vec ? i0 + e : k * CHUNK + e * THREADS + tid;
                if (i < 0 || i >= n) continue;
                float pe = p[i];
                if (step) {
                    float me = pm[i], ve = pv2[i];
                    adam1(pe, pg[i], me, ve, cf);
                    p[i] = pe;
                    pm[i] = me;
                    pv2[i] = ve;
                }
                if (ema) ema[i] = ema_d != 0.f ? ema1(ema[i], pe, ema_d, ema_a) : pe;
            }
        }
    }
}

}  // namespace

MREFSR_EXPORT int mrefsr_optim_job_chunks(int64_t n) { return n < 0 || n > ((int64_t)1 << 40) ? -1 : job_chunks(n); }

MREFSR_EXPORT int mrefsr_ema_multi_f32(const mrefsr_optim_job *jobs, int n_jobs, float decay, float one_minus_decay, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(jobs && n_jobs > 0, "ema_multi: jobs=%p n_jobs=%d", (const void *)jobs, n_jobs);
    MREFSR_REQUIRE(decay >= 0.f && decay <= 1.f, "ema_multi: decay=%g outside [0, 1]", (double)decay);
    hipLaunchKernelGGL(optim_multi_kernel<false>, dim3(GRID), dim3(THREADS), 0, (hipStream_t)stream, jobs, n_jobs,
                       (const mrefsr_adam_group *)nullptr, 0, decay, one_minus_decay);
    return mrefsr::check_launch("ema_multi");
}

MREFSR_EXPORT int mrefsr_adam_multi_f32(const mrefsr_optim_job *jobs, int n_jobs, const mrefsr_adam_group *groups, int n_groups,
                                        float ema_decay, float one_minus_ema_decay, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(jobs && n_jobs > 0 && groups && n_groups > 0, "adam_multi: jobs=%p n_jobs=%d groups=%p n_groups=%d", (const void *)jobs,
                   n_jobs, (const void *)groups, n_groups);
    MREFSR_REQUIRE(ema_decay >= 0.f && ema_decay <= 1.f, "adam_multi: ema_decay=%g outside [0, 1]", (double)ema_decay);
    hipLaunchKernelGGL(optim_multi_kernel<true>, dim3(GRID), dim3(THREADS), 0, (hipStream_t)stream, jobs, n_jobs, groups, n_groups,
                       ema_decay, one_minus_ema_decay);
    return mrefsr::check_launch("adam_multi");
}
