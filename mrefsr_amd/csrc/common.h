// Shared helpers for the gfx950 kernels of libmrefsr_hip.so (no torch, no CUDA shims).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/mrefsr_hip.h"

#define MREFSR_EXPORT extern "C" __attribute__((visibility("default")))

namespace mrefsr {

char *err_buf();  // thread-local, 512 bytes (defined in api.hip)

inline int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

inline int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MREFSR_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return MREFSR_OK;
}

// "set this kernel's function attribute once" is once PER DEVICE: a process that drives a second GPU needs it there too.
// `done` is a per-kernel bit mask indexed by the current device id (racing first calls both set the attribute: harmless).
inline bool first_use_on_device(unsigned long long &done)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return true;
    const unsigned long long bit = 1ull << dev;
    if (done & bit) return false;
    done |= bit;
    return true;
}

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Switches of A/B measurements (tools/; MREFSR_HIP_LIB = a -DMREFSR_AB_KERNELS build): such a build reads them from the environment
// per call.  In the product they are their defaults at compile time: no getenv, and the branch a switch guards folds away.
#ifdef MREFSR_AB_KERNELS
inline long ab_int(const char *name, long dflt) { const char *e = getenv(name); return e ? atol(e) : dflt; }
inline bool ab_flag(const char *name, bool dflt) { const char *e = getenv(name); return e ? e[0] != '0' : dflt; }
#else
constexpr long ab_int(const char *, long dflt) { return dflt; }
constexpr bool ab_flag(const char *, bool dflt) { return dflt; }
#endif

#ifdef __HIPCC__
// The fixed-order ("deterministic") reductions of the training step (train.hip, dynagg.hip, conv_nhwc.hip): every block writes
// its partial sums to its own row of a workspace with store_partial (write-through stores: they reach memory without a release
// of the block's other, much larger output from L2); the block that draws the last ticket adds the rows in ascending row order.
// last_block_by_ticket is called by ALL threads of the block behind those stores; true in every thread of the one block that
// arrived last, whose loads then see every row: every wave waits for its own stores, the block meets, lane 0 draws the ticket and
// -- last -- acquires at agent scope (the XCDs' L2s are not coherent with each other, nor is this CU's L1) before anyone reads.
// The last block puts the ticket word back to 0, so a launch needs no memset in front of it and can be replayed from a graph.
// `lds_flag`: one word of the block's LDS that nothing else uses across this call.
__device__ __forceinline__ void store_partial(float *p, const float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ bool last_block_by_ticket(unsigned int *ticket, const unsigned int nblocks, int *lds_flag)
{
    constexpr int VMCNT0 = 0x0F70;   // s_waitcnt vmcnt(0) alone (gfx9 encoding: expcnt and lgkmcnt left at their maxima)
    __builtin_amdgcn_s_waitcnt(VMCNT0);
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nblocks - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __builtin_amdgcn_s_waitcnt(VMCNT0);   // (the invalidate has completed before the block is let through the barrier)
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        *lds_flag = last ? 1 : 0;
    }
    __syncthreads();
    return *lds_flag != 0;
}

// rows [n_rows] of `ld` floats each: column c added in ascending row order, eight loads in flight
__device__ __forceinline__ float sum_rows_in_order(const float *part, const int n_rows, const long ld, const int c)
{
    float s = 0.f;
    int r = 0;
    for (; r + 8 <= n_rows; r += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = part[(long)(r + k) * ld + c];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; r < n_rows; ++r) s += part[(long)r * ld + c];
    return s;
}
#endif

// corr.hip: exact correlation kernel on the query tiles flagged by the pre-filter (corr_prefilter.hip)
int launch_corr_top1_flagged(const float *y_in, const float *y_ref, const float *inv_ref, const float *nrm_in, int64_t *max_idx,
                             float *max_val, int n_in, int n_pair, int Cp, int h, int w, const int *tile_flag, const int *flag_count,
                             int min_flags, hipStream_t stream);

}  // namespace mrefsr

namespace mrefsr_corr { struct PrefilterOut; }
namespace mrefsr {
// corr_rowstream.hip: row-stationary fp16 pre-filter (pass A of mrefsr_corr_top1_prefilter_f32, Cp = 256)
int launch_corr_prefilter_rs16(const void *yh_in, const void *yh_ref, const float *inv_ref, const float *nrm_in, const float *tau,
                               const mrefsr_corr::PrefilterOut &out, int n_in, int n_pair, int h, int w, float tau_scale, float *dbg,
                               void *scratch, hipStream_t stream);
// bytes of `scratch` (per-lane candidate lists of the exchanged-products kernel)
int64_t corr_prefilter_rs16_scratch_bytes(int n_pair, int h, int w);
int64_t corr_prefilter_rs16_mfma_flop(int h, int w, const char **name);
}  // namespace mrefsr

#define MREFSR_REQUIRE(cond, ...) \
    do { if (!(cond)) return mrefsr::fail(MREFSR_E_INVALID, __VA_ARGS__); } while (0)
