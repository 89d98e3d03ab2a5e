// Wave, block and last-block reductions of the gfx950 kernels (device code only; common.h includes this under __HIPCC__).
// Every order of additions below is fixed and part of the kernels' contracts (bit-reproducible losses, metrics and gradients).
// The helpers hold additions and maxima only -- no multiply that -ffp-contract could fuse with an add -- so they give the same bits
// in the files built with -ffp-contract=off (metrics, refselect, optim, gan_reg, texture) as in the others, and a plain `+` gives
// the bits of the __fadd_rn that refselect.hip's stated order asks for.
#pragma once
#include <hip/hip_runtime.h>

namespace mrefsr {

// ---- one wave -------------------------------------------------------------------------------------------------
// Called by all 64 lanes of a wave (any number of waves).  wave_max: xor butterfly, every lane holds the maximum afterwards.
// wave_sum: __shfl_down by 32 .. 1, lane 0 alone holds the total afterwards (float, double, 64-bit integers).  No LDS, no barrier.
__device__ __forceinline__ float wave_max(float m)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    return m;
}

template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// max |x| of a launch into the zero-initialised word `dst` (non-negative floats order like their bit patterns): called by all
// lanes of a wave with the lane's running maximum m >= 0; one wave reduction, then lane 0 raises the word with one atomic unless
// the maximum is 0 or not finite.  `dst` is not NULL: the caller tests that.  1-D blocks (lane = threadIdx.x & 63).
// PEEK: one plain read first: after the first blocks most waves' maxima are below the word already -- tens of thousands of atomics
// on ONE address cost the bandwidth-bound launches 0.3 ms.
template <bool PEEK>
__device__ __forceinline__ void publish_amax(unsigned int *dst, float m)
{
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0 && m > 0.f && m < 3.0e38f && (!PEEK || __float_as_uint(m) > __builtin_nontemporal_load(dst)))
        atomicMax(dst, __float_as_uint(m));
}

// max of the four |components|: what a thread that stores a float4 folds into its running maximum
__device__ __forceinline__ float amax4(const float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }

// ---- one block ------------------------------------------------------------------------------------------------
// The halving tree over the THREADS values of a 1-D block of THREADS threads: red[t] = op(red[t], red[t + o]) for all t < o,
// o = THREADS / 2 .. 1.  Called by ALL threads of the block; every thread gets the result.  `red`: THREADS elements of LDS.
// The one barrier rule: the block meets before `red` is written (whatever the caller kept there has been read by then) and again
// behind the read of red[0], so on return `red` is free -- for the next block_reduce or for anything else, with no barrier of the
// caller's in between.  T: float, double, long long.
template <int THREADS, class T, class Op>
__device__ __forceinline__ T block_reduce(T *red, const T v, const Op op)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = op(red[tid], red[tid + o]);
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}

template <int THREADS, class T>
__device__ __forceinline__ T block_sum(T *red, const T v)
{
    return block_reduce<THREADS>(red, v, [](const T a, const T b) { return a + b; });
}

template <int THREADS>
__device__ __forceinline__ float block_max(float *red, const float v)
{
    return block_reduce<THREADS>(red, v, [](const float a, const float b) { return fmaxf(a, b); });
}

// The other fixed order, in double: each wave by wave_sum, then thread 0 adds the waves' totals in ascending wave order.  Called by
// ALL threads of a 1-D block of THREADS; the total is valid in thread 0 alone.  `wsum`: THREADS / 64 doubles of LDS that nothing
// else uses in the kernel (no barrier in front of its write, none behind its read).  Not the tree's association: the two stay apart.
template <int THREADS>
__device__ __forceinline__ double block_sum_by_waves(double v, double *wsum)
{
    const int tid = threadIdx.x;
    v = wave_sum(v);
    if ((tid & 63) == 0) wsum[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (tid == 0) {
        s = wsum[0];
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w) s += wsum[w];
    }
    return s;
}

// ---- all blocks of a launch: the last block finishes ------------------------------------------------------------
// The fixed-order ("deterministic") reductions of the training step (train.hip, dynagg.hip, conv_nhwc.hip) and of the losses: every
// block writes its partial sums to its own row of a workspace with store_partial (write-through stores: they reach memory without
// a release of the block's other, much larger output from L2); the block that draws the last ticket adds the rows in ascending row
// order.
// last_block_by_ticket is called by ALL threads of the block behind those stores; true in every thread of the one block that
// arrived last, whose loads then see every row: every wave waits for its own stores, the block meets, lane 0 draws the ticket and
// -- last -- acquires at agent scope (the XCDs' L2s are not coherent with each other, nor is this CU's L1) before anyone reads.
// The last block puts the ticket word back to 0, so a launch needs no memset in front of it and can be replayed from a graph.
// `lds_flag`: one word of the block's LDS that nothing else uses across this call.
__device__ __forceinline__ void store_partial(float *p, const float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_partial(double *p, const double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

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

// One partial per block, the scalar finish: called by ALL threads of the last block (256 threads, 1-D) behind a true
// last_block_by_ticket.  The partials come into `red` (256 floats of LDS) 256 at a time by agent-scope relaxed loads, and thread 0
// adds each chunk in ascending block order in double: the total is valid in thread 0 alone.  The block meets before every chunk
// overwrites `red` (thread 0 has read the chunk before) and not behind the last one: `red` is still thread 0's on return.
__device__ __forceinline__ double sum_partials_in_order(const float *partial, const unsigned int nblocks, float *red)
{
    constexpr unsigned int CHUNK = 256;
    const unsigned int tid = threadIdx.x;
    double total = 0.0;
    for (unsigned int base = 0; base < nblocks; base += CHUNK) {
        __syncthreads();
        red[tid] = base + tid < nblocks ? __hip_atomic_load(partial + base + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
        __syncthreads();
        if (tid == 0) {
            const int n = (int)min(CHUNK, nblocks - base);
            for (int q = 0; q < n; ++q) total += (double)red[q];
        }
    }
    return total;
}

}  // namespace mrefsr
