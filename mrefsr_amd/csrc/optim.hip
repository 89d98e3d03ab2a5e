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
// Gradient-norm clipping and non-finite step skipping (torch.nn.utils.clip_grad_norm_, norm_type 2, error_if_nonfinite False)
// ride on the same table and the same chunk partition: grad_sqnorm_kernel reads every gradient once (16-byte loads, aligned by the
// gradient's own address), each lane adds its squares in fp32, the block adds its lanes on a fixed tree in double and writes ONE
// double into a workspace; grad_norm_finalize_kernel (one block) adds those in index order and writes mrefsr_grad_clip_state --
// the norm, the clip coefficient, found_inf and the count of skipped steps, which only this one-block launch ever writes.  The
// consumers read that state: optim_multi_kernel<true, true> multiplies the gradient by the coefficient in registers (the gradient
// tensors stay as they are), leaves p, m and v alone on a skipped step -- the EMA is still written -- and takes its bias
// corrections at step - skipped; grad_scale_kernel multiplies the gradients in place for torch's own Adam.  No atomics anywhere.
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

// CLIP: `clip` (written by grad_norm_finalize_kernel, a launch before this one) gives the factor every gradient is multiplied by
// on its way into adam1 and, with `skip`, whether this update is left out; <true, false> is the kernel without any of it
template <bool ADAM, bool CLIP>
__global__ __launch_bounds__(THREADS) void optim_multi_kernel(const mrefsr_optim_job *__restrict__ jobs, const int n_jobs,
                                                               const mrefsr_adam_group *__restrict__ groups, const int n_groups,
                                                               const float ema_d, const float ema_a,
                                                               const mrefsr_grad_clip_state *__restrict__ clip, const int skip)
{
    float gcoef = 1.f;
    long long skipped = 0;
    bool hold = false;   // a skipped step: no job takes its Adam update
    if (CLIP) {
        gcoef = clip->coef;
        skipped = clip->skipped;
        hold = skip && clip->found_inf != 0.f;
    }
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
        const bool step = ADAM && !(CLIP && hold) && job.g && job.m && job.v && job.group >= 0 && job.group < n_groups;   // torch skips .grad None
        if (!p || (!step && !ema)) { c = cend; continue; }
        Coef cf = {};
        if (ADAM && step) {
            if (CLIP) {   // the steps that were skipped did not count (the host's counters go on counting them)
                mrefsr_adam_group grp = groups[job.group];
                grp.step = grp.step - skipped > 1 ? grp.step - skipped : 1;
                cf = group_coef(grp);
            } else {
                cf = group_coef(groups[job.group]);
            }
        }
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
                        adam1(pe, CLIP ? gv[e] * gcoef : gv[e], me, ve, cf);
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
                    adam1(pe, CLIP ? pg[i] * gcoef : pg[i], me, ve, cf);
                    p[i] = pe;
                    pm[i] = me;
                    pv2[i] = ve;
                }
                if (ema) ema[i] = ema_d != 0.f ? ema1(ema[i], pe, ema_d, ema_a) : pe;
            }
        }
    }
}

// ---- the global gradient norm
// One pass over job.g in the partition of optim_multi_kernel.  A gradient is the only stream, so every job is walked in 16-byte
// groups aligned by the gradient's own address; the groups cut by its start or end take guarded 4-byte accesses.
// SCALE false: the lane adds g * g (two roundings: squares in fp32, one that overflows is inf and makes the norm non-finite),
// the block's lanes are added in double -- wave by wave on the shuffle tree, then the four waves in order -- and partial[block] is
// written, 0 by a block without chunks.  SCALE true: g *= clip->coef in place, nothing else.
template <bool SCALE>
__global__ __launch_bounds__(THREADS) void grad_walk_kernel(const mrefsr_optim_job *__restrict__ jobs, const int n_jobs,
                                                             double *__restrict__ partial,
                                                             const mrefsr_grad_clip_state *__restrict__ clip)
{
    const long long total = (long long)jobs[n_jobs - 1].first_chunk + job_chunks(jobs[n_jobs - 1].n);
    const long long c0 = total * blockIdx.x / gridDim.x, c1 = total * (blockIdx.x + 1) / gridDim.x;
    const int tid = threadIdx.x;
    const float coef = SCALE ? clip->coef : 1.f;
    float acc = 0.f;
    if (c0 < c1) {
        int j = 0;
        for (int hi = n_jobs - 1; j < hi;) {   // the last job whose first chunk is <= c0
            const int mid = (j + hi + 1) >> 1;
            if (jobs[mid].first_chunk <= c0) j = mid; else hi = mid - 1;
        }
        for (long long c = c0; c < c1;) {
            while (j + 1 < n_jobs && jobs[j + 1].first_chunk <= c) ++j;
            const mrefsr_optim_job job = jobs[j];
            const long long jend = j + 1 < n_jobs ? (long long)jobs[j + 1].first_chunk : total;
            const long long cend = c1 < jend ? c1 : jend;
            const long long n = job.n;
            gf32 *const pg = (gf32 *)job.g;
            if (!pg) { c = cend; continue; }
            const int a = (int)(((size_t)pg >> 2) & 3);   // elements by which g lies behind a 16-byte boundary
            for (; c < cend; ++c) {
                const long long i0 = (c - job.first_chunk) * CHUNK + 4 * tid - a;
                if (i0 >= 0 && i0 + 4 <= n) {
                    f32x4 gv = *(const gf32x4 *)(pg + i0);
                    if (SCALE) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) gv[e] = gv[e] * coef;
                        *(gf32x4 *)(pg + i0) = gv;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc += gv[e] * gv[e];
                    }
                    continue;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long long i = i0 + e;
                    if (i < 0 || i >= n) continue;
                    const float ge = pg[i];
                    if (SCALE) pg[i] = ge * coef; else acc += ge * ge;
                }
            }
        }
    }
    if (SCALE) return;
    __shared__ double wsum[THREADS / 64];
    const double s = mrefsr::block_sum_by_waves<THREADS>((double)acc, wsum);
    if (tid == 0) partial[blockIdx.x] = s;
}

// one block: the partials in index order, then the state.  torch's clip_grad_norm_: coef = min(max_norm / (norm + 1e-6), 1) in
// fp32 (a NaN stays a NaN, as under torch.clamp); max_norm <= 0: no clipping, coef 1.  `skipped` has this one writer.
__global__ __launch_bounds__(THREADS) void grad_norm_finalize_kernel(const double *__restrict__ partial, const int n_partial,
                                                                      const float max_norm, const int skip,
                                                                      mrefsr_grad_clip_state *__restrict__ state)
{
    __shared__ double part[GRID];
    for (int i = threadIdx.x; i < n_partial; i += THREADS) part[i] = partial[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < n_partial; ++i) s += part[i];
    const float norm = (float)sqrt(s);
    const bool bad = !(fabsf(norm) <= 3.402823466e+38f);   // inf or NaN
    float coef = 1.f;
    if (max_norm > 0.f) {
        const float den = norm + 1e-6f;
        coef = (float)((double)max_norm / (double)den);   // (the correctly rounded fp32 quotient)
        if (coef > 1.f) coef = 1.f;
    }
    state->total_norm = norm;
    state->coef = coef;
    state->found_inf = bad ? 1.f : 0.f;
    if (bad && skip) state->skipped = state->skipped + 1;
}

}  // namespace

MREFSR_EXPORT int mrefsr_optim_job_chunks(int64_t n) { return n < 0 || n > ((int64_t)1 << 40) ? -1 : job_chunks(n); }

MREFSR_EXPORT int mrefsr_ema_multi_f32(const mrefsr_optim_job *jobs, int n_jobs, float decay, float one_minus_decay, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(jobs && n_jobs > 0, "ema_multi: jobs=%p n_jobs=%d", (const void *)jobs, n_jobs);
    MREFSR_REQUIRE(decay >= 0.f && decay <= 1.f, "ema_multi: decay=%g outside [0, 1]", (double)decay);
    hipLaunchKernelGGL((optim_multi_kernel<false, false>), dim3(GRID), dim3(THREADS), 0, (hipStream_t)stream, jobs, n_jobs,
                       (const mrefsr_adam_group *)nullptr, 0, decay, one_minus_decay, (const mrefsr_grad_clip_state *)nullptr, 0);
    return mrefsr::check_launch("ema_multi");
}

MREFSR_EXPORT int mrefsr_adam_multi_f32(const mrefsr_optim_job *jobs, int n_jobs, const mrefsr_adam_group *groups, int n_groups,
                                        float ema_decay, float one_minus_ema_decay, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(jobs && n_jobs > 0 && groups && n_groups > 0, "adam_multi: jobs=%p n_jobs=%d groups=%p n_groups=%d", (const void *)jobs,
                   n_jobs, (const void *)groups, n_groups);
    MREFSR_REQUIRE(ema_decay >= 0.f && ema_decay <= 1.f, "adam_multi: ema_decay=%g outside [0, 1]", (double)ema_decay);
    hipLaunchKernelGGL((optim_multi_kernel<true, false>), dim3(GRID), dim3(THREADS), 0, (hipStream_t)stream, jobs, n_jobs, groups, n_groups,
                       ema_decay, one_minus_ema_decay, (const mrefsr_grad_clip_state *)nullptr, 0);
    return mrefsr::check_launch("adam_multi");
}

MREFSR_EXPORT int64_t mrefsr_grad_norm_workspace_bytes(void) { return (int64_t)GRID * (int64_t)sizeof(double); }

MREFSR_EXPORT int mrefsr_grad_sqnorm_multi_f32(const mrefsr_optim_job *jobs, int n_jobs, void *workspace, int64_t workspace_bytes,
                                               mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(jobs && n_jobs > 0, "grad_sqnorm_multi: jobs=%p n_jobs=%d", (const void *)jobs, n_jobs);
    MREFSR_REQUIRE(workspace && workspace_bytes >= mrefsr_grad_norm_workspace_bytes() && ((size_t)workspace & 7) == 0,
                   "grad_sqnorm_multi: workspace=%p (8-byte aligned) of %lld bytes, %lld needed", workspace, (long long)workspace_bytes,
                   (long long)mrefsr_grad_norm_workspace_bytes());
    hipLaunchKernelGGL(grad_walk_kernel<false>, dim3(GRID), dim3(THREADS), 0, (hipStream_t)stream, jobs, n_jobs, (double *)workspace,
                       (const mrefsr_grad_clip_state *)nullptr);
    return mrefsr::check_launch("grad_sqnorm_multi");
}

MREFSR_EXPORT int mrefsr_grad_norm_finalize_f32(const void *workspace, int64_t workspace_bytes, float max_norm, int skip_nonfinite,
                                                mrefsr_grad_clip_state *state, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(workspace && workspace_bytes >= mrefsr_grad_norm_workspace_bytes() && ((size_t)workspace & 7) == 0,
                   "grad_norm_finalize: workspace=%p (8-byte aligned) of %lld bytes, %lld needed", workspace, (long long)workspace_bytes,
                   (long long)mrefsr_grad_norm_workspace_bytes());
    MREFSR_REQUIRE(state && ((size_t)state & 7) == 0, "grad_norm_finalize: state=%p (8-byte aligned)", (const void *)state);
    MREFSR_REQUIRE(max_norm == max_norm && max_norm <= 3.402823466e+38f, "grad_norm_finalize: max_norm=%g (finite; <= 0: no clipping)",
                   (double)max_norm);
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, (const double *)workspace, GRID, max_norm,
                       skip_nonfinite ? 1 : 0, state);
    return mrefsr::check_launch("grad_norm_finalize");
}

MREFSR_EXPORT int mrefsr_grad_scale_multi_f32(const mrefsr_optim_job *jobs, int n_jobs, const mrefsr_grad_clip_state *state,
                                              mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(jobs && n_jobs > 0 && state, "grad_scale_multi: jobs=%p n_jobs=%d state=%p", (const void *)jobs, n_jobs, (const void *)state);
    hipLaunchKernelGGL(grad_walk_kernel<true>, dim3(GRID), dim3(THREADS), 0, (hipStream_t)stream, jobs, n_jobs, (double *)nullptr, state);
    return mrefsr::check_launch("grad_scale_multi");
}

MREFSR_EXPORT int mrefsr_adam_multi_clip_f32(const mrefsr_optim_job *jobs, int n_jobs, const mrefsr_adam_group *groups, int n_groups,
                                             float ema_decay, float one_minus_ema_decay, const mrefsr_grad_clip_state *state,
                                             int skip_nonfinite, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(jobs && n_jobs > 0 && groups && n_groups > 0 && state, "adam_multi_clip: jobs=%p n_jobs=%d groups=%p n_groups=%d state=%p",
                   (const void *)jobs, n_jobs, (const void *)groups, n_groups, (const void *)state);
    MREFSR_REQUIRE(ema_decay >= 0.f && ema_decay <= 1.f, "adam_multi_clip: ema_decay=%g outside [0, 1]", (double)ema_decay);
    hipLaunchKernelGGL((optim_multi_kernel<true, true>), dim3(GRID), dim3(THREADS), 0, (hipStream_t)stream, jobs, n_jobs, groups, n_groups,
                       ema_decay, one_minus_ema_decay, state, skip_nonfinite ? 1 : 0);
    return mrefsr::check_launch("adam_multi_clip");
}
