// Host check of csrc/dcn_sample.h (tests/test_dcn_sample_cpu.py compiles this with -fsanitize=undefined on the host side and runs
// it): the bilinear set-up and the shape check are __host__ __device__ / host code, so the rule the kernels sample by is evaluated
// here on the CPU, for float and double, on every pair of the 16 x 16 edge classes of tests/golden/dcn_edge_cases.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "dcn_sample.h"

using namespace mrefsr_dcn;

namespace mrefsr {
char *err_buf()   // (the library's is in api.hip)
{
    static thread_local char buf[512];
    return buf;
}
}  // namespace mrefsr

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

// the 16 target positions of one axis of length L, by class index (dcn_edge_cases.edge_values): all multiples of 1/8
static void edge_values(int L, double (&e)[16])
{
    const double k = (L - 1) / 2, l = L;
    const double v[16] = {-1.125, -1.0, -0.875, -0.5, -0.125, 0.0, 0.125, k, k + 0.5, l - 1.125, l - 1.0, l - 0.875, l - 0.5, l - 0.125, l, l + 0.5};
    std::memcpy(e, v, sizeof(v));
}

// The rule restated plainly, one `if` per corner: the value's weights as deform_conv_cuda_kernel.cu:467-497 forms them, the
// derivative coefficients as :526-568 does ((low + 1 - position) and (position - low), not 1 - fraction), the window as :531.
template <typename A>
struct Plain {
    int o[4];
    bool v[4], inside;
    A w[4], dh[4], dw[4];
    Plain(A h, A w_, int H, int W)
    {
        inside = !(h <= -1 || h >= H || w_ <= -1 || w_ >= W);
        const int hl = (int)std::floor(h), wl = (int)std::floor(w_), hh = hl + 1, wh = wl + 1;
        const A lh = h - hl, lw = w_ - wl, uh = 1 - lh, uw = 1 - lw;
        const int ch[4] = {hl, hl, hh, hh}, cw[4] = {wl, wh, wl, wh};
        for (int k = 0; k < 4; ++k) {
            v[k] = false, w[k] = 0, dh[k] = 0, dw[k] = 0;
            int y = ch[k], x = cw[k];   // (an out-of-range corner is never read; its offset stays inside the map)
            if (y < 0) y = 0;
            if (y > H - 1) y = H - 1;
            if (x < 0) x = 0;
            if (x > W - 1) x = W - 1;
            o[k] = y * W + x;
        }
        if (!inside) return;
        if (hl >= 0 && wl >= 0) v[0] = true, w[0] = uh * uw, dh[0] = -1 * (wl + 1 - w_), dw[0] = -1 * (hl + 1 - h);
        if (hl >= 0 && wh <= W - 1) v[1] = true, w[1] = uh * lw, dh[1] = -1 * (w_ - wl), dw[1] = (hl + 1 - h);
        if (hh <= H - 1 && wl >= 0) v[2] = true, w[2] = lh * uw, dh[2] = (wl + 1 - w_), dw[2] = -1 * (h - hl);
        if (hh <= H - 1 && wh <= W - 1) v[3] = true, w[3] = lh * lw, dh[3] = (w_ - wl), dw[3] = (h - hl);
    }
};

template <typename A>
static void check_rule(const char *name)
{
    const int Ls[3] = {1, 5, 70};
    const A ulp1 = std::numeric_limits<A>::epsilon();   // one ulp of 1
    long n = 0;
    for (const int H : Ls)
        for (const int W : Ls) {
            double ey[16], ex[16];
            edge_values(H, ey);
            edge_values(W, ex);
            for (int cy = 0; cy < 16; ++cy)
                for (int cx = 0; cx < 16; ++cx, ++n) {
                    const A h = (A)ey[cy], w = (A)ex[cx];
                    const Bilinear<A> b(h, w, H, W);
                    const Plain<A> p(h, w, H, W);
                    CHECK(b.inside() == p.inside, "%s H %d W %d (%g, %g): inside", name, H, W, (double)h, (double)w);
                    bool all_valid = true;
                    A sum = 0;
                    for (int k = 0; k < 4; ++k) {
                        CHECK(b.o[k] == p.o[k] && b.o[k] >= 0 && b.o[k] < H * W, "%s H %d W %d (%g, %g) corner %d: offset %d, expected %d", name, H,
                              W, (double)h, (double)w, k, b.o[k], p.o[k]);
                        CHECK(b.v(k) == p.v[k], "%s H %d W %d (%g, %g) corner %d: validity", name, H, W, (double)h, (double)w, k);
                        CHECK(b.w[k] == p.w[k], "%s H %d W %d (%g, %g) corner %d: weight %.17g, expected %.17g", name, H, W, (double)h, (double)w,
                              k, (double)b.w[k], (double)p.w[k]);
                        CHECK(b.dh(k) == p.dh[k] && b.dw(k) == p.dw[k], "%s H %d W %d (%g, %g) corner %d: d/dh %.17g (%.17g), d/dw %.17g (%.17g)",
                              name, H, W, (double)h, (double)w, k, (double)b.dh(k), (double)p.dh[k], (double)b.dw(k), (double)p.dw[k]);
                        if (h <= -1 || h >= H || w <= -1 || w >= W)   // on or outside the window boundary: nothing contributes
                            CHECK(b.w[k] == 0 && b.dh(k) == 0 && b.dw(k) == 0 && !b.v(k), "%s H %d W %d (%g, %g) corner %d: nonzero outside the window",
                                  name, H, W, (double)h, (double)w, k);
                        all_valid = all_valid && b.v(k);
                        sum += b.w[k];
                    }
                    if (all_valid) CHECK(std::fabs(sum - (A)1) <= ulp1, "%s H %d W %d (%g, %g): weights sum to %.17g", name, H, W, (double)h, (double)w, (double)sum);
                }
        }
    std::printf("%s: %ld positions\n", name, n);
}

static void check_pos()
{
    Geo g{};
    g.sh = 2, g.sw = 3, g.ph = 1, g.pw = 2, g.dh = 2, g.dw = 1;
    float hi, wi;
    sample_pos(g, 5, 7, 2, 1, 0.25f, -0.5f, hi, wi);
    CHECK(hi == (float)(5 * 2 - 1 + 2 * 2) + 0.25f && wi == (float)(7 * 3 - 2 + 1 * 1) - 0.5f, "sample_pos: (%g, %g)", hi, wi);
}

static void check_geo()
{
    const mrefsr_dcn_shape ok = {2, 8, 9, 11, 8, 3, 3, 1, 1, 1, 1, 1, 1, 1, 4};
    Geo g;
    CHECK(make_geo(&ok, g, "t") == MREFSR_OK && g.Ho == 9 && g.Wo == 11 && g.sh == 1 && g.dg == 4, "make_geo: %d x %d", g.Ho, g.Wo);
    CHECK(make_geo(nullptr, g, "t") == MREFSR_E_INVALID && std::strstr(mrefsr::err_buf(), "null shape"), "null shape: %s", mrefsr::err_buf());
    mrefsr_dcn_shape s = ok;
    s.W = 0;
    CHECK(make_geo(&s, g, "t") == MREFSR_E_INVALID && std::strstr(mrefsr::err_buf(), "non-positive"), "zero dimension: %s", mrefsr::err_buf());
    s = ok, s.pad_h = -1;
    CHECK(make_geo(&s, g, "t") == MREFSR_E_INVALID, "negative padding");
    s = ok, s.dg = 3;   // C % dg != 0
    CHECK(make_geo(&s, g, "t") == MREFSR_E_INVALID && std::strstr(mrefsr::err_buf(), "not divisible"), "C %% dg: %s", mrefsr::err_buf());
    s = ok, s.H = 1, s.pad_h = 0;   // a 3-tap window on one row without padding
    CHECK(make_geo(&s, g, "t") == MREFSR_E_INVALID && std::strstr(mrefsr::err_buf(), "empty output"), "empty output: %s", mrefsr::err_buf());
}

int main()
{
    check_rule<float>("float");
    check_rule<double>("double");
    check_pos();
    check_geo();
    std::printf("dcn_sample host check: %d failures\n", g_fail);
    return g_fail ? 1 : 0;
}
