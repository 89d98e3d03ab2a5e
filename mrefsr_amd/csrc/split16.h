// The arithmetic every hot kernel rests on, in one place: fp32-equivalent results from the 16-bit matrix pipe by
// splitting the operands exactly.
//   terms 16: fp16 (11-bit significands), two-term split = 22 bits, three products:
//        a = ah + al,  al stored as AL = fp16(al * 2^11)            (same binade as a: never denormal before a is)
//        w * S = wh + wl, S = 2^s chosen at pack time so that max|w| * S is in [2^13, 2^14)
//                         (wl ~ 2^-11 wh stays a normal fp16 for every weight within 2^-17 of the largest);
//                         a third plane WH2 = wh * 2^-11 (exact) pairs with AL
//        a * w * S  ~=  ah*wh + ah*wl + AL*WH2        (dropped al*wl: 2^-22 relative), fp32 accumulation,
//        the epilogue multiplies by 1/S.  Requires |a| < 65504 (fp16 range).
//   terms 6:  bf16, activations and weights as hi + mid + lo, six partial products >= 2^-24.
// Vector typedefs, the packed 16-bit conversions, the MFMA wrappers, the power-of-two scale of an activation or gradient tensor
// and the splits themselves.  The conversions, the splits and the scale also compile for the host (tests/test_split16_cpu.py).
//
// Some sites reach the same VALUES by another instruction sequence, each for a measured reason that its own comment gives; they
// stay where they are, and a change of the arithmetic here has to visit them too:
//   conv_wino_common.h  split_pair       the unscaled-low split with the remainder formed by v_fma_mixlo / mixhi_f16
//   dcn.hip             gather_commit    the scaled-low split as fma(h, -2048, v * 2048), the fp16 half read in place
//   wgrad.hip           commit_x / _g    scalar _Float16 casts, the halves of a pair stored apart
//   conv_wino4.hip      transform        the splits in place, on the packed registers of its micro-operations
//   conv_nhwc.hip       split4           the bf16 peel four wide, the last term without its remainder
//   dcn.hip             gather_commit    the bf16 peel on packed pairs, between the stores of the planes
#pragma once
#include <hip/hip_runtime.h>

namespace mrefsr_split16 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define SPLIT16_HD __host__ __device__ __forceinline__

SPLIT16_HD bf16x8 as_bf(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }

// packed round-to-nearest-even bf16 of two floats, and back
SPLIT16_HD unsigned int pk_bf16(float a, float b)
{
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
SPLIT16_HD float bf_lo(unsigned int p) { return __builtin_bit_cast(float, p << 16); }
SPLIT16_HD float bf_hi(unsigned int p) { return __builtin_bit_cast(float, p & 0xffff0000u); }

// packed round-to-nearest-even fp16 of two floats, and back
SPLIT16_HD unsigned int pk_f16(float a, float b)
{
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(f32x2{a, b}, f16x2));
}
SPLIT16_HD f32x2 un_f16(unsigned int p) { return __builtin_convertvector(__builtin_bit_cast(f16x2, p), f32x2); }

// WH2 = wh * 2^-11 of 8 packed fp16: exact while the result is a normal fp16, round-to-nearest-even into the
// denormals exactly like the pack kernel's conversion (plain v_pk_mul_f16: safe next to MFMAs, tools/hazard/)
SPLIT16_HD u32x4 scale_wh(u32x4 v)
{
    const f16x2 k = {(_Float16)0.00048828125f, (_Float16)0.00048828125f};
    u32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned int d = v[i];
        r[i] = __builtin_bit_cast(unsigned int, __builtin_bit_cast(f16x2, d) * k);
    }
    return r;
}

// one 32x32x16 MFMA step on 8 packed 16-bit values per lane and operand, fp32 accumulation: fp16, and its bf16 twin
__device__ __forceinline__ f32x16 mma16(const u32x4 a, const u32x4 b, const f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mma16_bf(const u32x4 a, const u32x4 b, const f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf(a), as_bf(b), c, 0, 0, 0);
}

// The scale of an activation or gradient tensor whose magnitudes would sit in the fp16 subnormals (training dgrad / wgrad):
// `amax` is max |x| of the tensor(s), in device memory, and may be NULL.  x is multiplied by in_s = 2^(TOP - e), which brings
// that maximum into [2^(TOP-1), 2^TOP), before the fp16 split, and the result by its inverse (multiplied into the caller's
// oscale).  Exact powers of two either way.  TOP = 14 for the direct kernels; 12 for the Winograd kernels, whose input transform
// grows a value by up to 4.  A maximum of 0, a subnormal one, inf or NaN leaves both untouched.
// (The form that takes the value serves the kernels that have loaded it already, or know the pointer to be valid.)
template <int TOP>
SPLIT16_HD void amax_scale(const float am, float &in_s, float &oscale)
{
    if (am > 1.0e-30f && am < 3.0e38f) {
        int e;
        (void)frexpf(am, &e);                      // am = m 2^e, m in [0.5, 1): floor(log2 am) = e - 1
        in_s = ldexpf(1.f, TOP - e);
        oscale *= ldexpf(1.f, e - TOP);
    }
}
template <int TOP>
SPLIT16_HD void amax_scale(const float *amax, float &in_s, float &oscale)
{
    if (amax) amax_scale<TOP>(*amax, in_s, oscale);
}

// 2 floats -> packed (ah, AL = fp16((a - ah) * 2^11)): the scaled-low split of the activations.  a - ah is representable and
// the power of two scales it exactly, so AL carries 11 more bits of a whatever a's binade.  (hi and lo may be words of LDS: the
// high word is written as soon as the low one no longer needs it, where the kernels wrote it.)
SPLIT16_HD void split_scaled(const float a, const float b, unsigned int &hi, unsigned int &lo)
{
    const unsigned int p = pk_f16(a, b);
    const f32x2 h = un_f16(p);
    hi = p;
    lo = pk_f16((a - h[0]) * 2048.f, (b - h[1]) * 2048.f);
}
// the same for 4 floats (both conversions, then both remainders)
SPLIT16_HD void split_scaled4(const float a, const float b, const float c, const float d, u32x2 &hi, u32x2 &lo)
{
    const unsigned int p0 = pk_f16(a, b), p1 = pk_f16(c, d);
    const f32x2 h0 = un_f16(p0), h1 = un_f16(p1);
    hi = u32x2{p0, p1};
    lo = u32x2{pk_f16((a - h0[0]) * 2048.f, (b - h0[1]) * 2048.f), pk_f16((c - h1[0]) * 2048.f, (d - h1[1]) * 2048.f)};
}
// 2 floats -> packed (gh, gl = fp16(g - gh)): the unscaled-low split of an operand that was scaled into [2^13, 2^14) first
// (gradients: amax_scale) and whose partner supplies the 2^-11 (scale_wh of the high plane pairs with the other operand's AL)
SPLIT16_HD void split_plain(const float a, const float b, unsigned int &hi, unsigned int &lo)
{
    const unsigned int p = pk_f16(a, b);
    const f32x2 h = un_f16(p);
    hi = p;
    lo = pk_f16(a - h[0], b - h[1]);
}
// one weight, already multiplied by S -> the planes wh, wl = fp16(v - wh), WH2 = fp16(wh * 2^-11)
SPLIT16_HD void split_weight(const float v, unsigned short &wh, unsigned short &wl, unsigned short &wh2)
{
    const unsigned int ph = pk_f16(v, 0.f);
    const float h = un_f16(ph)[0];
    wh = (unsigned short)(ph & 0xffffu);
    wl = (unsigned short)(pk_f16(v - h, 0.f) & 0xffffu);
    wh2 = (unsigned short)(pk_f16(h * (1.0f / 2048.f), 0.f) & 0xffffu);
}
// one term of the bf16 multi-term split (hi + mid + lo, 8 significand bits each, 24 together: exact): the bf16 of v, written
// where it goes (a pack kernel's plane), and v left holding the (exact) remainder
SPLIT16_HD void peel_bf16(float &v, unsigned short &term)
{
    const unsigned int p = pk_bf16(v, 0.f);
    term = (unsigned short)(p & 0xffffu);
    v -= bf_lo(p);
}

#undef SPLIT16_HD

}  // namespace mrefsr_split16
