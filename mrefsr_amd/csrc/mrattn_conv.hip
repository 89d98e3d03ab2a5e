// Multi-reference attention head, assembly side (ref_mrapa_restoration_arch.py:321-335): the softmax blend of the T warped reference
// maps moved IN FRONT of conv_ass.  conv_ass is a plain 3x3 convolution (bias, no activation) and the softmax weights p_t depend on
// the output pixel x only, so
//     r(x) = sum_t p_t(x) (sum_d W_d s_t(x + d) + b)  =  sum_d W_d u_d(x) + b sum_t p_t(x),     u_d(x) = sum_t p_t(x) s_t(x + d)
// -- one implicit GEMM over the N images instead of a convolution over T * N images followed by a pass that folds T results into
// one.  The arithmetic is the direct kernels' (conv_nhwc.hip, terms 16): u is formed in fp32, split exactly into two fp16 terms,
// each product is three v_mfma_f32_32x32x16_f16 with fp32 accumulation against the packed weights of conv_nhwc
// ([cout block of 64][cin chunk of 16][tap][wh | wl | wh 2^-11][64][16], per-layer power-of-two scale).
//
// Block = 256 threads = 4 waves, 4 rows x 32 columns of output pixels x 128 couts; wave w owns row w (one A fragment, four cout
// columns).  TWO blocks live on a CU (64 KB of LDS and at most 256 registers each: __launch_bounds__(256, 2)): a SIMD holds one
// wave of each, and while one block fetches and stages its tiles the other one's blend and MFMAs run -- the tiles of a pass are in
// registers only between their request and their LDS store, never across the tap loop.  The tap loop is straight-line code per
// number of staged maps, pipelined by one tap: the blend of tap d + 1 issues between the MFMAs of tap d.  Per
// 16-channel chunk the (6 x 34)-pixel halo tiles of up to TG raw fp32 reference maps are
// staged in LDS as [t][channel quad][pixel][4 floats] (a lane's `ds_read_b128` walks the pixels at a 16-byte stride:
// conflict-free), unscaled; the 3x3 shifts are whole pixels, so the one tile serves the nine taps.  For a tap a lane (pixel
// lane & 31, channels 8 (lane >> 5) .. + 8 of the chunk) reads its pixel's T references at x + d, blends them with the pixel's
// weights (registers, multiplied once by the power-of-two input scale: fma(p 2^s, v, u) has the bits of fma(p, v 2^s, u); fma
// chain, t ascending, absent t skipped: never staged, never read), splits and multiplies: no column buffer exists.  The fp16 range
// guard looks at the values the CENTRE tap reads: every pixel of the image is the centre of exactly one output pixel.
// Accumulation order of every output: channel chunk, (group of TG references when T > TG: u is linear in t, each group's partial
// blend is split and multiplied on its own), tap, term -- fixed, no atomics but the range flag: bit-reproducible.
#include <type_traits>

#include "conv_common.h"

namespace {
using namespace mrefsr_conv;

constexpr int TG = 5;                       // reference maps staged per pass (5 x 12.75 KB of LDS)
constexpr int TR = 4, TW = 32;              // output tile
constexpr int PH = TR + 2, PW = TW + 2, NPIX = PH * PW;
constexpr int QPL = NPIX * 16;              // bytes of one channel quad's plane
constexpr int TPL = 4 * QPL;                // bytes per staged map
constexpr int NPIECE = NPIX * 4;            // 16-byte pieces per staged map
constexpr int NPK = (NPIECE + 255) / 256;     // pieces of one staged map per thread
constexpr int NJ = 4;                       // 32-cout MFMA columns per wave (128 couts per block)
constexpr int LDS_RAW = TG * TPL;
constexpr int LDS_BYTES = LDS_RAW + TR * TW * 4 + 64 + 16;   // + sum_t p per pixel + the list of present references
static_assert(2 * LDS_BYTES <= 160 * 1024, "two blocks per CU");

struct BlendArgs {
    const float *refs, *prob, *bias, *in_amax;
    const unsigned short *wp;
    const unsigned int *valid_bits;
    int *range_flag;
    float *out;
    int N, T, H, W, ncb;
    float out_scale;
};

template <int C, bool MASKED>
__global__ __launch_bounds__(256, 2) void mrattn_blend_conv_kernel(const BlendArgs A)
{
    constexpr int NCH = C / KC, COUT = 2 * C, TAPS = 9, NW = 3;
    extern __shared__ __align__(16) unsigned char smem[];
    float *psum = reinterpret_cast<float *>(smem + LDS_RAW);
    int *tlist = reinterpret_cast<int *>(smem + LDS_RAW + TR * TW * 4);   // [16] present t ascending, [16] their count
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const int H = A.H, W = A.W, T = A.T, N = A.N;
    // Workgroups go to the 8 XCDs round-robin in dispatch order.  The ncb blocks that share a pixel tile (and read the same halo
    // tiles) are the ncb consecutive blocks of ONE XCD: block L is the (L / 8)-th of XCD L % 8, that XCD's s-th block works on
    // cout block s % ncb of tile (s / ncb) * 8 + xcd.  The first reader brings the tiles into the XCD's L2, the others find them.
    // (The dispatch order is an assumption about speed only: under any other order every block still computes its own tile.)
    const int tx_n = (W + TW - 1) / TW, ty_n = (H + TR - 1) / TR;
    const unsigned int lin = blockIdx.x, seq = lin >> 3;
    const int cbk = (int)(seq % (unsigned)A.ncb);
    const long tile = (long)(seq / (unsigned)A.ncb) * 8 + (lin & 7u);
    if (tile >= (long)tx_n * ty_n * N) return;   // (the grid is padded to whole groups of 8 tiles; the whole block leaves)
    const int n = (int)(tile / (tx_n * ty_n)), trem = (int)(tile - (long)n * (tx_n * ty_n));
    const int y0 = (trem / tx_n) * TR, x0 = (trem % tx_n) * TW;

    if (tid == 0) {
        const unsigned int vb = MASKED ? A.valid_bits[n] : 0xffffffffu;
        int c = 0;
        for (int t = 0; t < T; ++t)
            if ((vb >> t) & 1u) tlist[c++] = t;
        tlist[16] = c;
    }
    float in_s = 1.f, oscale = A.out_scale;
    amax_scale<14>(A.in_amax, in_s, oscale);   // the input tensor's maximum brought into [2^13, 2^14) by an exact power of two
    // fp16 range guard: |v| in_s > 65000 or NaN  <=>  the bits of |v| above those of 65000 / in_s (a power of two: exact; an
    // infinite quotient is brought back so that an infinite v still trips)
    const unsigned int guard_bits = __float_as_uint(fminf(65000.f / in_s, 3.4028234664e38f));
    __syncthreads();
    const int total = __builtin_amdgcn_readfirstlane(tlist[16]);
    const int n_grp = (total + TG - 1) / TG, n_it = NCH * n_grp;

    // sum_t p_t of the wave's own pixels (present t ascending, fp32): the weight of the bias
    const int gy_w = y0 + wv, gx_w = x0 + l31;
    const bool pok = gy_w < H && gx_w < W;
    const float *prow = A.prob + (((size_t)n * H + (gy_w < H ? gy_w : H - 1)) * W + (gx_w < W ? gx_w : W - 1)) * T;
    {
        float s = 0.f;
        for (int k = 0; k < total; ++k) s += prow[__builtin_amdgcn_readfirstlane(tlist[k])];
        if (kh == 0) psum[wv * TW + l31] = pok ? s : 0.f;
    }

    f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

    // the halo tiles of pass `it` (chunk it / n_grp, reference group it % n_grp) -> registers -> LDS.  A thread owns the same NPK
    // 16-byte pieces (pixel, channel quad) of every staged map: their offsets inside a map and inside an LDS tile are computed once,
    // a map's base address is wave-uniform.  A piece outside the map is zero in every pass (the convolution's zero padding): it is
    // written here, once, and its lane stays out of the passes' stores (its request reads the map's first bytes instead); a map that
    // is not staged is not requested.
    unsigned int goff[NPK], loff[NPK];
    bool in_map[NPK];
#pragma unroll
    for (int k = 0; k < NPK; ++k) {
        const int i = tid + k * 256;
        const int p = i >> 2, q = i & 3;
        const int py = p / PW, px = p - py * PW;
        const int gy = y0 + py - 1, gx = x0 + px - 1;
        const bool tile = i < NPIECE;
        in_map[k] = tile && gy >= 0 && gy < H && gx >= 0 && gx < W;
        goff[k] = in_map[k] ? (unsigned int)((gy * W + gx) * C + 4 * q) : 0u;   // floats (below 2^31: the entry checks H W 256)
        loff[k] = tile ? q * QPL + p * 16 : 0;
        if (tile && !in_map[k]) {
#pragma unroll
            for (int tg = 0; tg < TG; ++tg) *reinterpret_cast<float4 *>(smem + tg * TPL + loff[k]) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }

    // B fragments of one tap: NJ columns x (wh, wl); column j sits in cout block 2 cbk + (j >> 1), rows 32 (j & 1) ..: a uniform
    // base per cout block, one lane offset, the rest in the instruction
    const unsigned int wl_off = (unsigned int)(l31 * KC + kh * 8) * 2u;
    auto bload = [&](const int lin, u32x4 (&b)[NJ][2]) {   // lin = chunk * 9 + tap
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                const unsigned short *wu = A.wp + (((size_t)(cbk * 2 + (j >> 1)) * NCH * TAPS + lin) * NW * NB) * KC;
                b[j][sp] = *reinterpret_cast<const u32x4 *>(reinterpret_cast<const unsigned char *>(wu) + wl_off + (sp * NB + (j & 1) * 32) * KC * 2);
            }
    };

    unsigned int worst = 0u;   // the largest |v| bits the centre tap has read
    // The nine taps of a pass over CNT staged maps, straight-line, software-pipelined by one tap: while the 12 MFMAs of tap d run,
    // the LDS reads of tap d + 1 are in flight and its blend (fma chain, t ascending), range guard and split issue between them, in
    // 12 slots of one MFMA each (sched_barrier: left to itself the compiler puts the blend in front of the MFMAs).  The products of a
    // tap, smallest first: ah wl, AL WH2 (the third weight plane wh 2^-11 is derived, not loaded), ah wh.
    const unsigned char *sp0 = smem + (2 * kh) * QPL + (wv * PW + l31) * 16;
    auto taps = [&](auto cnt_c, const int cnt, const int ch, u32x4 (&b)[2][NJ][2], const float (&pr)[TG]) {
        constexpr int CNT = decltype(cnt_c)::value ? decltype(cnt_c)::value : TG;   // (0: the count is `cnt`, known at run time only)
        constexpr bool FIXED = decltype(cnt_c)::value != 0;
        f32x4 s[CNT][2];
        float u[8];
        u32x4 ah, al, nh, nl, w2[NJ];
        auto rd = [&](const int tap) {
            const unsigned char *sp = sp0 + (((tap * 11) >> 5) * (PW - 3) + tap) * 16;   // (dy PW + dx) pixels, tap = 3 dy + dx
#pragma unroll
            for (int k = 0; k < CNT; ++k)
                if (FIXED || k < cnt) {
                    s[k][0] = *reinterpret_cast<const f32x4 *>(sp + k * TPL);
                    s[k][1] = *reinterpret_cast<const f32x4 *>(sp + k * TPL + QPL);
                }
        };
        auto chain = [&](const int k, const bool centre) {
            if (!FIXED && k >= cnt) return;
            const float w = pr[k];
#pragma unroll
            for (int c = 0; c < 4; ++c) u[c] = fmaf(w, s[k][0][c], k ? u[c] : 0.f), u[4 + c] = fmaf(w, s[k][1][c], k ? u[4 + c] : 0.f);
            if (centre) {   // the centre tap reads the wave's own output pixels
                const unsigned int m = 0x7fffffffu;
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    worst = max(worst, max(max(__float_as_uint(s[k][h][0]) & m, __float_as_uint(s[k][h][1]) & m),
                                           max(__float_as_uint(s[k][h][2]) & m, __float_as_uint(s[k][h][3]) & m)));
            }
        };
        auto split = [&](const int c) {   // a = ah + al, al kept as fp16(al * 2^11): split16.h
            unsigned int h, l;
            split_scaled(u[2 * c], u[2 * c + 1], h, l);
            nh[c] = h, nl[c] = l;
        };
        rd(0);
#pragma unroll
        for (int k = 0; k < CNT; ++k) chain(k, false);
#pragma unroll
        for (int c = 0; c < 4; ++c) split(c);
        ah = nh, al = nl;
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) {
            const bool more = tap + 1 < TAPS;
            u32x4 (&bc)[NJ][2] = b[tap & 1];
            if (more) {
                bload(ch * TAPS + tap + 1, b[(tap + 1) & 1]);
                rd(tap + 1);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int sl = 0; sl < 12; ++sl) {
                const int j = sl & 3;
                if (sl < 4) acc[j] = mma16(ah, bc[j][1], acc[j]);
                else if (sl < 8) acc[j] = mma16(al, w2[j], acc[j]);
                else acc[j] = mma16(ah, bc[j][0], acc[j]);
                if (sl < 2) w2[2 * sl] = scale_wh(bc[2 * sl][0]), w2[2 * sl + 1] = scale_wh(bc[2 * sl + 1][0]);
                if (more) {
                    if (sl >= 2 && sl - 2 < CNT) chain(sl - 2, tap + 1 == 4);
                    if (sl >= 7 && sl < 11) split(sl - 7);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (more) ah = nh, al = nl;
        }
    };
    float pr[TG];
    // the passes, specialised on the number of staged maps where every pass of the block has the same (at most TG present references)
    auto passes = [&](auto cnt_c) {
        for (int it = 0; it < n_it; ++it) {
            const int ch = it / n_grp, g = it - ch * n_grp;
            const int cnt = total - g * TG < TG ? total - g * TG : TG;
            {
                f32x4 pf[TG][NPK];
#pragma unroll
                for (int tg = 0; tg < TG; ++tg)
                    if (tg < cnt) {
                        const int t = __builtin_amdgcn_readfirstlane(tlist[g * TG + tg]);
                        const float *base = A.refs + ((size_t)t * N + n) * H * W * C + ch * KC;
#pragma unroll
                        for (int k = 0; k < NPK; ++k) pf[tg][k] = *reinterpret_cast<const f32x4 *>(base + goff[k]);
                    } else {   // (defined on every path: no register lives from one pass into the next)
#pragma unroll
                        for (int k = 0; k < NPK; ++k) pf[tg][k] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                if (it) __syncthreads();   // the previous pass's tiles have been read
#pragma unroll
                for (int tg = 0; tg < TG; ++tg)
                    if (tg < cnt) {
#pragma unroll
                        for (int k = 0; k < NPK; ++k)
                            if (in_map[k]) *reinterpret_cast<f32x4 *>(smem + tg * TPL + loff[k]) = pf[tg][k];
                    }
            }
            __builtin_amdgcn_sched_barrier(0);   // the tiles leave the registers before the weight fragments claim theirs
            if (n_grp > 1 || it == 0) {
#pragma unroll
                for (int k = 0; k < TG; ++k) pr[k] = (k < cnt && pok) ? prow[__builtin_amdgcn_readfirstlane(tlist[g * TG + k])] * in_s : 0.f;
            }
            u32x4 b[2][NJ][2];   // the weight fragments run one tap ahead: even taps in [0], odd taps in [1]
            bload(ch * TAPS, b[0]);
            __syncthreads();
            taps(cnt_c, cnt, ch, b, pr);
        }
    };
    switch (total <= TG ? total : 0) {
    case 1: passes(std::integral_constant<int, 1>{}); break;
    case 2: passes(std::integral_constant<int, 2>{}); break;
    case 3: passes(std::integral_constant<int, 3>{}); break;
    case 4: passes(std::integral_constant<int, 4>{}); break;
    case 5: passes(std::integral_constant<int, 5>{}); break;
    default: passes(std::integral_constant<int, 0>{}); break;
    }
    if (worst > guard_bits && A.range_flag) atomicOr(A.range_flag, 1);
    __syncthreads();   // psum of every row is written (a block without a present reference ran no pass)

    // MFMA result: a lane holds cout 32 j + (lane & 31) of pixels x = (e & 3) + 8 (e >> 2) + 4 kh of the row: a store instruction
    // writes two pixels' 128 contiguous bytes
    if (gy_w < H) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int co = cbk * (NJ * 32) + j * 32 + l31;
            const float bv = A.bias ? A.bias[co] : 0.f;
            float *orow = A.out + (((size_t)n * H + gy_w) * W) * COUT + co;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int x = (e & 3) + 8 * (e >> 2) + 4 * kh, gx = x0 + x;
                if (gx < W) orow[(size_t)gx * COUT] = acc[j][e] * oscale + bv * psum[wv * TW + x];
            }
        }
    }
}

// The launch needs more than 64 KB of dynamic LDS: the kernel's limit is raised on first use, once PER DEVICE (a process that drives a
// second GPU needs it there too).  A set that fails is reported and tried again by the next call: without it the launch cannot run.
template <int C, bool MASKED> int launch_blend_c(const BlendArgs &a, const dim3 grid, hipStream_t st)
{
    static unsigned long long attr_done = 0;
    if (mrefsr::first_use_on_device(attr_done)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&mrattn_blend_conv_kernel<C, MASKED>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
        if (e != hipSuccess) {
            attr_done = 0;
            (void)hipGetLastError();
            return mrefsr::fail(MREFSR_E_LAUNCH, "mrattn_blend_conv: %d bytes of dynamic LDS refused: %s", LDS_BYTES, hipGetErrorString(e));
        }
    }
    hipLaunchKernelGGL((mrattn_blend_conv_kernel<C, MASKED>), grid, dim3(256), LDS_BYTES, st, a);
    return mrefsr::check_launch("mrattn_blend_conv");
}

template <bool MASKED> int launch_blend(const BlendArgs &a, int C, hipStream_t st)
{
    const long tiles = (long)((a.W + TW - 1) / TW) * ((a.H + TR - 1) / TR) * a.N;
    const dim3 grid((unsigned)(((tiles + 7) / 8) * 8 * a.ncb));
    if (C == 64) return launch_blend_c<64, MASKED>(a, grid, st);
    if (C == 128) return launch_blend_c<128, MASKED>(a, grid, st);
    return launch_blend_c<256, MASKED>(a, grid, st);
}

}  // namespace

MREFSR_EXPORT int mrefsr_mrattn_blend_conv_f32(const float *refs, const float *prob, const void *packed, const float *bias,
                                               const uint32_t *valid_bits, const float *in_amax, int *range_flag, float *out, int N, int T,
                                               int H, int W, int C, float wscale, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(refs && prob && packed && out, "mrattn_blend_conv: null pointer");
    MREFSR_REQUIRE(N > 0 && T > 0 && T <= 16 && H > 0 && W > 0, "mrattn_blend_conv: N=%d T=%d H=%d W=%d (T <= 16)", N, T, H, W);
    MREFSR_REQUIRE((int64_t)((W + TW - 1) / TW) * ((H + TR - 1) / TR) * N < (int64_t)1 << 28, "mrattn_blend_conv: N=%d H=%d W=%d (too many tiles)", N, H, W);
    MREFSR_REQUIRE((int64_t)H * W * 256 < (int64_t)1 << 31, "mrattn_blend_conv: H=%d W=%d (32-bit offsets inside a map)", H, W);
    MREFSR_REQUIRE(wscale > 0.f, "mrattn_blend_conv: wscale=%g", (double)wscale);
    if (C != 64 && C != 128 && C != 256)
        return mrefsr::fail(MREFSR_E_UNSUPPORTED, "mrattn_blend_conv: c=%d (64, 128 or 256: the three MRAPAFusion heads)", C);
    BlendArgs a;
    a.refs = refs, a.prob = prob, a.bias = bias, a.in_amax = in_amax;
    a.wp = reinterpret_cast<const unsigned short *>(packed);
    a.valid_bits = valid_bits, a.range_flag = range_flag, a.out = out;
    a.N = N, a.T = T, a.H = H, a.W = W, a.ncb = 2 * C / (NJ * 32);
    a.out_scale = 1.0f / wscale;
    return valid_bits ? launch_blend<true>(a, C, (hipStream_t)stream) : launch_blend<false>(a, C, (hipStream_t)stream);
}
