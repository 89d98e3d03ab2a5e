// The sampling rule of the deformable convolution, in one place: the shape check of every DCN entry point, the position of a
// sample and its bilinear set-up (deform_conv_cuda_kernel.cu:467-497 for the value, :526-568 for the derivatives).
//   position   (ho * stride - pad + i * dil) + off_y, (wo * stride - pad + j * dil) + off_x: the integers summed first, then
//              the offset added in the arithmetic type;
//   window     the sample contributes only inside (-1, H) x (-1, W);
//   corners    floor / floor + 1 on both axes; a corner out of range has weight 0 and takes no gradient.
// Every kernel of dcn.hip, dcn_bwd.hip and dcn_any.hip builds its set-up here and reads the members it needs; the others fold
// away.  All of it also compiles for the host (tests/test_dcn_sample_cpu.py evaluates the rule on the CPU).
#pragma once
#include <math.h>

#include "common.h"

namespace mrefsr_dcn {

#define DCN_HD __host__ __device__ __forceinline__

struct Geo {
    int B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, groups, dg, Ho, Wo;
};

inline int make_geo(const mrefsr_dcn_shape *s, Geo &g, const char *who)
{
    if (!s) return mrefsr::fail(MREFSR_E_INVALID, "%s: null shape", who);
    g = Geo{s->B, s->C, s->H, s->W, s->Co, s->kh, s->kw, s->stride_h, s->stride_w, s->pad_h, s->pad_w, s->dil_h, s->dil_w, s->groups, s->dg, 0, 0};
    if (g.B <= 0 || g.C <= 0 || g.H <= 0 || g.W <= 0 || g.Co <= 0 || g.kh <= 0 || g.kw <= 0 || g.sh <= 0 || g.sw <= 0 || g.dh <= 0 ||
        g.dw <= 0 || g.groups <= 0 || g.dg <= 0 || g.ph < 0 || g.pw < 0)
        return mrefsr::fail(MREFSR_E_INVALID, "%s: non-positive dimension in shape", who);
    if (g.C % g.groups || g.Co % g.groups || g.C % g.dg)
        return mrefsr::fail(MREFSR_E_INVALID, "%s: C=%d / Co=%d not divisible by groups=%d / dg=%d", who, g.C, g.Co, g.groups, g.dg);
    g.Ho = (g.H + 2 * g.ph - (g.dh * (g.kh - 1) + 1)) / g.sh + 1;
    g.Wo = (g.W + 2 * g.pw - (g.dw * (g.kw - 1) + 1)) / g.sw + 1;
    if (g.Ho <= 0 || g.Wo <= 0) return mrefsr::fail(MREFSR_E_INVALID, "%s: empty output %dx%d", who, g.Ho, g.Wo);
    return 0;
}

// position of the sample of output pixel (ho, wo) under tap (ti, tj) with offsets (oh, ow)
template <typename A>
DCN_HD void sample_pos(const Geo &g, int ho, int wo, int ti, int tj, A oh, A ow, A &hi, A &wi)
{
    hi = (A)(ho * g.sh - g.ph + ti * g.dh) + oh, wi = (A)(wo * g.sw - g.pw + tj * g.dw) + ow;
}

// Four SCALAR fp32 products.  Left to itself the SLP vectoriser pairs (uh*lw, lh*uw) into
//     v_pk_mul_f32 vD, vA, vB op_sel:[0,1] op_sel_hi:[1,0]          (crossed halves)
// and on gfx950 that instruction returned wrong values in lanes 48..63 whenever waves of OTHER workgroups
// were issuing bf16 MFMAs on the same SIMD (run-to-run different DCN results at full size, 0.2-2 % of the
// pixels; DESIGN 3.2 has the bisection: one workgroup per CU, no MFMA, -fno-slp-vectorize and this form
// are clean, the hand-written instruction fails with or without wait states around it).  The empty asm
// statement makes a product opaque to the vectoriser; tests/test_boundary.py checks the built library
// for the instruction form.  (The host has no such instruction, and fp64 products do not pack.)
DCN_HD void keep_scalar(float &p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(p));
#else
    (void)p;
#endif
}
DCN_HD void keep_scalar(double &) {}

// the bilinear set-up of one sample at (hi, wi) of an H x W map, in the arithmetic type A (float, double)
template <typename A>
struct Bilinear {
    // What the set-up stores is what the fused kernels keep in registers across their pipeline stages, in this order and of
    // this size: their register allocation follows it (a further stored member moved registers in 28 instantiations of the
    // forward kernels).  The validities are therefore one word of bits, and what derives from them is computed where it is read.
    int o[4];            // pixel index of the four corners (hl wl, hl wh, hh wl, hh wh), clamped into the map
    A w[4];              // bilinear weights, 0 where the corner is not valid
    A lh, lw;            // fractions
    int ok;              // bit k: corner k is in range and the sample inside the window; bit 4: the sample is inside the window

    DCN_HD bool inside() const { return (ok & 16) != 0; }
    // corner k takes part (its weight may still be 0 by value)
    DCN_HD bool v(int k) const { return ((ok >> k) & 1) != 0; }
    // d(sample) / d(h), d(w): coefficient of corner k's value, 0 where the corner is not valid
    DCN_HD A dh(int k) const
    {
        const A uw = (A)1 - lw;
        return v(k) ? (k == 0 ? -uw : k == 1 ? -lw : k == 2 ? uw : lw) : (A)0;
    }
    DCN_HD A dw(int k) const
    {
        const A uh = (A)1 - lh;
        return v(k) ? (k == 0 ? -uh : k == 1 ? uh : k == 2 ? -lh : lh) : (A)0;
    }

    Bilinear() = default;
    DCN_HD Bilinear(const A hi, const A wi, const int H, const int W)
    {
        const bool inside = (hi > (A)-1) && (wi > (A)-1) && (hi < (A)H) && (wi < (A)W);
        const A fh = floor(hi), fw = floor(wi);
        const int hl = (int)fh, wl = (int)fw, hh = hl + 1, wh = wl + 1;
        lh = hi - fh;
        lw = wi - fw;
        const A uh = (A)1 - lh, uw = (A)1 - lw;
        const bool okhl = inside && hl >= 0, okhh = inside && hh <= H - 1;
        const bool okwl = wl >= 0, okwh = wh <= W - 1;
        const int chl = min(max(hl, 0), H - 1), chh = min(max(hh, 0), H - 1);
        const int cwl = min(max(wl, 0), W - 1), cwh = min(max(wh, 0), W - 1);
        o[0] = chl * W + cwl;
        o[1] = chl * W + cwh;
        o[2] = chh * W + cwl;
        o[3] = chh * W + cwh;
        A p1 = uh * uw, p2 = uh * lw, p3 = lh * uw, p4 = lh * lw;
        keep_scalar(p1);
        keep_scalar(p2);
        keep_scalar(p3);
        keep_scalar(p4);
        w[0] = (okhl && okwl) ? p1 : (A)0;
        w[1] = (okhl && okwh) ? p2 : (A)0;
        w[2] = (okhh && okwl) ? p3 : (A)0;
        w[3] = (okhh && okwh) ? p4 : (A)0;
        ok = (int)(okhl && okwl) | (int)(okhl && okwh) << 1 | (int)(okhh && okwl) << 2 | (int)(okhh && okwh) << 3 | (int)inside << 4;
    }
};

}  // namespace mrefsr_dcn
