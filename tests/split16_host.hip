// Host check of csrc/split16.h (tests/test_split16_cpu.py compiles this with -fsanitize=undefined on the host side and runs it):
// the conversions, the splits and the amax scale are __host__ __device__, so what the kernels compute is computed here on the CPU.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "split16.h"

using namespace mrefsr_split16;

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++g_fail <= 20) {                         \
                std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

static float f16_lo(unsigned int p) { return un_f16(p)[0]; }
static float f16_hi(unsigned int p) { return un_f16(p)[1]; }

// ---- the amax scale: amax * in_s in [2^(TOP-1), 2^TOP), in_s * out_s == 1, the caller's oscale multiplied, the guard's cases untouched
template <int TOP> static void check_scale()
{
    const float ms[3] = {1.f, 1.5f, 1.9999999f};
    for (int ex = -99; ex <= 126; ++ex)
        for (const float m : ms) {
            const float amax = std::ldexp(m, ex);
            float in_s = 1.f, out_s = 1.f;
            amax_scale<TOP>(&amax, in_s, out_s);
            const float top = amax * in_s;
            CHECK(top >= std::ldexp(1.f, TOP - 1) && top < std::ldexp(1.f, TOP), "TOP %d amax %g in_s %g", TOP, amax, in_s);
            CHECK(in_s * out_s == 1.f, "TOP %d amax %g in_s %g out_s %g", TOP, amax, in_s, out_s);
            float in2 = 1.f, o3 = 3.f;   // a caller's initial oscale is multiplied, not replaced
            amax_scale<TOP>(&amax, in2, o3);
            CHECK(in2 == in_s && o3 == 3.f * out_s, "TOP %d amax %g oscale %g", TOP, amax, o3);
            float in4 = 1.f, o4 = 3.f;   // the form that takes the value
            amax_scale<TOP>(amax, in4, o4);
            CHECK(in4 == in_s && o4 == o3, "TOP %d amax %g (by value)", TOP, amax);
        }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float guarded[4] = {0.f, 1e-31f, inf, nan};
    for (const float g : guarded) {
        float in_s = 7.f, out_s = 3.f;
        amax_scale<TOP>(&g, in_s, out_s);
        CHECK(in_s == 7.f && out_s == 3.f, "TOP %d guarded amax %g: %g %g", TOP, g, in_s, out_s);
        amax_scale<TOP>(g, in_s, out_s);
        CHECK(in_s == 7.f && out_s == 3.f, "TOP %d guarded amax %g (by value): %g %g", TOP, g, in_s, out_s);
    }
    float in_s = 7.f, out_s = 3.f;
    amax_scale<TOP>(static_cast<const float *>(nullptr), in_s, out_s);
    CHECK(in_s == 7.f && out_s == 3.f, "TOP %d NULL: %g %g", TOP, in_s, out_s);
}

// values of every fp16 binade (its edges, a tie of the fp16 rounding, odd significands), both signs; the fp16 maximum and the
// largest float that still rounds to it; values below 2^-14, whose high term is an fp16 subnormal; 0
static std::vector<float> activations()
{
    std::vector<float> v = {0.f, 65504.f, -65504.f, 65519.f, -65519.f};
    for (int k = -24; k <= 15; ++k) {
        const float b = std::ldexp(1.f, k);
        const float c[] = {b, std::nextafter(b, 0.f), std::nextafter(b, 2.f * b), b * (1.f + 0x1p-11f), b * (1.f + 0x1p-11f + 0x1p-23f),
                           b * (1.f + 0x1p-12f), b * 1.2345678f, b * 1.9990234f, b * (1.f + 0x1p-10f + 0x1p-22f), b * (1.f + 0x1p-23f)};
        for (const float x : c)
            if (x < 65520.f) v.push_back(x), v.push_back(-x);
    }
    unsigned int s = 12345u;   // and a few thousand pseudo-random significands over the same binades
    for (int i = 0; i < 4000; ++i) {
        s = s * 1664525u + 1013904223u;
        const float m = 1.f + (float)(s >> 9) * 0x1p-23f;
        s = s * 1664525u + 1013904223u;
        const float x = std::ldexp(m, -24 + (int)((s >> 8) % 40u));
        if (x < 65520.f) v.push_back((s & 1u) ? x : -x);
    }
    return v;
}

// ---- the scaled-low split.  For |a| >= 2^-14 (a normal fp16 range; the high term takes 11 of a's 24 bits, the remainder is
// exact in fp32 and at most 2^-11 |a|, its scaled fp16 is rounded by at most 2^-11 relative or, where it is an fp16 subnormal,
// by 2^-25 absolute = 2^-36 after the 2^-11 -- no more than 2^-22 |a| from 2^-14 up): |hi + lo 2^-11 - a| <= 2^-22 |a|.
// Below 2^-14 both terms are fp16 subnormals and the error is the absolute 2^-36.
static void check_split_scaled(const std::vector<float> &vals)
{
    int n_sub_lo = 0;
    for (size_t i = 0; i + 1 < vals.size(); i += 2) {
        const float a = vals[i], b = vals[i + 1];
        unsigned int hi, lo;
        split_scaled(a, b, hi, lo);
        const float ab[2] = {a, b}, h[2] = {f16_lo(hi), f16_hi(hi)}, l[2] = {f16_lo(lo), f16_hi(lo)};
        for (int k = 0; k < 2; ++k) {
            const double err = std::fabs((double)h[k] + (double)l[k] * 0x1p-11 - (double)ab[k]);
            const double bound = std::fabs(ab[k]) >= 0x1p-14f ? 0x1p-22 * std::fabs((double)ab[k]) : 0x1p-36;
            CHECK(err <= bound, "split_scaled a %.9g hi %.9g lo %.9g err %.3g bound %.3g", ab[k], h[k], l[k], err, bound);
            if (std::fabs(ab[k]) >= 0x1p-14f && l[k] != 0.f && std::fabs(l[k]) < 0x1p-14f) ++n_sub_lo;
        }
        // the 4-wide form and the unscaled-low split give the same high words; the unscaled low term is the scaled one's value / 2^11
        // wherever both are normal fp16
        u32x2 h4, l4;
        split_scaled4(a, b, b, a, h4, l4);
        unsigned int hr, lr;
        split_scaled(b, a, hr, lr);
        CHECK(h4[0] == hi && l4[0] == lo && h4[1] == hr && l4[1] == lr, "split_scaled4 differs from split_scaled at %.9g %.9g", a, b);
        unsigned int hp, lp;
        split_plain(a, b, hp, lp);
        CHECK(hp == hi, "split_plain high word at %.9g %.9g", a, b);
        const float lpv[2] = {f16_lo(lp), f16_hi(lp)};
        for (int k = 0; k < 2; ++k)
            if (std::fabs(lpv[k]) >= 0x1p-14f) CHECK(lpv[k] * 2048.f == l[k], "split_plain low term %.9g vs %.9g at %.9g", lpv[k], l[k], ab[k]);
    }
    CHECK(n_sub_lo > 10, "only %d values with a subnormal low term were tested", n_sub_lo);
}

// ---- the weight triple of v = w S (max |v| in [2^13, 2^14)): WH2 == wh 2^-11 exactly while that is a normal fp16 (|wh| >= 2^-3),
// and the same bits as scale_wh of the packed high plane everywhere.  wh + wl against v: wl = fp16(v - wh) is not scaled, so its
// rounding is 2^-11 relative while it is normal and 2^-25 absolute once it is a subnormal: |wh + wl - v| <= max(2^-22 |v|, 2^-25),
// which is 2^-22 |v| for |v| >= 2^-3 -- every weight within 2^-17 of the largest.
static void check_split_weight()
{
    std::vector<float> vs = {0.f};
    unsigned int s = 777u;
    for (int k = -12; k <= 13; ++k)
        for (int i = 0; i < 200; ++i) {
            s = s * 1664525u + 1013904223u;
            const float m = i == 0 ? 1.f : (i == 1 ? 1.9999999f : 1.f + (float)(s >> 9) * 0x1p-23f);
            vs.push_back(std::ldexp((s & 1u) ? m : -m, k));
        }
    for (const float v : vs) {
        unsigned short wh, wl, wh2;
        split_weight(v, wh, wl, wh2);
        const float h = f16_lo(wh), l = f16_lo(wl), h2 = f16_lo(wh2);
        if (std::fabs(h) >= 0x1p-3f) CHECK(h2 == h * 0x1p-11f, "WH2 %.9g != wh 2^-11 = %.9g (v %.9g)", h2, h * 0x1p-11f, v);
        const u32x4 sw = scale_wh(u32x4{(unsigned int)wh | ((unsigned int)wh << 16), wh, 0u, (unsigned int)wh << 16});
        CHECK((sw[0] & 0xffffu) == wh2 && (sw[0] >> 16) == wh2 && sw[1] == wh2 && (sw[3] >> 16) == wh2 && (sw[3] & 0xffffu) == 0u && sw[2] == 0u,
              "scale_wh %08x vs WH2 %04x (v %.9g)", sw[0], wh2, v);
        const double err = std::fabs((double)h + (double)l - (double)v);
        const double bound = std::fabs(v) >= 0x1p-3f ? 0x1p-22 * std::fabs((double)v) : 0x1p-25;
        CHECK(err <= bound, "split_weight v %.9g wh %.9g wl %.9g err %.3g bound %.3g", v, h, l, err, bound);
    }
}

// ---- the bf16 peel: three terms of 8 significand bits reproduce a float exactly (24 bits), whatever its binade in the kernels' range
static void check_peel(const std::vector<float> &vals)
{
    for (const float x : vals) {
        float v = x;
        unsigned short t3[3];
        for (int t = 0; t < 3; ++t) peel_bf16(v, t3[t]);
        CHECK((double)bf_lo(t3[0]) + bf_lo(t3[1]) + bf_lo(t3[2]) == (double)x && v == 0.f, "peel_bf16 %.9g: rest %.3g", x, v);
        const unsigned int p = pk_bf16(x, -x);   // the packed pair and its two halves
        CHECK((p & 0xffffu) == t3[0] && bf_hi(p) == -bf_lo(p), "pk_bf16 %.9g: %08x", x, p);
    }
}

int main()
{
    check_scale<14>();
    check_scale<12>();
    const std::vector<float> vals = activations();
    check_split_scaled(vals);
    check_split_weight();
    check_peel(vals);
    std::printf("split16 host check: %d failures\n", g_fail);
    return g_fail ? 1 : 0;
}
