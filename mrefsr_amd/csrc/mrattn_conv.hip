// Multi-reference attention head, assembly side (ref_mrapa_restoration_arch.py:321-335): the softmax blend of the T warped reference
// maps moved IN FRONT of conv_ass.  conv_ass is a plain 3x3 convolution (bias, no activation) and the softmax weights p_t depend on
// the output pixel x only, so
//     r(x) = sum_t p_t(x) (sum_d W_d s_t(x + d) + b)  =  sum_d W_d u_d(x) + b sum_t p_t(x),     u_d(x) = sum_t p_t(x) s_t(x + d)
// -- one implicit GEMM over the N images instead of a convolution over T * N images followed by a pass that folds T results into
// one.  The arithmetic is the direct kernels' (conv_nhwc.hip, terms 16): u is formed in fp32, split exactly into two fp16 terms,
// each product is three v_mfma_f32_32x32x16_f16 with fp32 accumulation against the packed weights of conv_nhwc
// ([cout block of 64][cin chunk of 16][tap][wh | wl | wh 2^-11][64][16], per-layer power-of-two scale).
//
// Block = 256 threads = 4 waves, 8 rows x 32 columns of output pixels x 128 couts; wave w owns rows 2w, 2w + 1 (two A fragments per
// weight fragment).  Per 16-channel chunk the (10 x 34)-pixel halo tiles of up to TG raw fp32 reference maps are staged in LDS as
// [t][channel quad][pixel][4 floats] (a lane's `ds_read_b128` walks the pixels at a 16-byte stride: conflict-free); the 3x3 shifts
// are whole pixels, so the one tile serves the nine taps.  For a tap a lane (pixel lane & 31, channels 8 (lane >> 5) .. + 8 of the
// chunk) reads its pixel's T references at x + d, blends them with the pixel's weights (registers; fma chain, t ascending, absent t
// skipped: never staged, never read), splits and multiplies: no column buffer exists.  The next chunk's tiles travel in registers
// beside the MFMAs.  Accumulation order of every output: channel chunk, (group of TG references when T > TG: u is linear in t, each
// group's partial blend is split and multiplied on its own), tap, term -- fixed, no atomics but the range flag: bit-reproducible.
#include "conv_common.h"

namespace {
using namespace mrefsr_conv;

constexpr int TG = 5;                       // reference maps staged per pass (5 x 21.25 KB of LDS)
constexpr int TR = 8, TW = 32;              // output tile
constexpr int PH = TR + 2, PW = TW + 2, NPIX = PH * PW;
constexpr int QPL = NPIX * 16;              // bytes of one channel quad's plane
constexpr int TPL = 4 * QPL;                // bytes per staged map
constexpr int NPIECE = NPIX * 4;            // 16-byte pieces per staged map
constexpr int NPK = (NPIECE + 255) / 256;     // pieces of one staged map per thread
constexpr int NJ = 4;                       // 32-cout MFMA columns per wave (128 couts per block)
constexpr int LDS_RAW = TG * TPL;
constexpr int LDS_BYTES = LDS_RAW + TR * TW * 4 + 64 + 16;   // + sum_t p per pixel + the list of present references

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
__global__ __launch_bounds__(256) void mrattn_blend_conv_kernel(const BlendArgs A)
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
    __syncthreads();
    const int total = __builtin_amdgcn_readfirstlane(tlist[16]);
    const int n_grp = (total + TG - 1) / TG, n_it = NCH * n_grp;

    // sum_t p_t of the wave's own pixels (present t ascending, fp32): the weight of the bias
    const float *prow[2];
    bool pok[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int gy = y0 + wv * 2 + m, gx = x0 + l31;
        pok[m] = gy < H && gx < W;
        prow[m] = A.prob + (((size_t)n * H + (gy < H ? gy : H - 1)) * W + (gx < W ? gx : W - 1)) * T;
        float s = 0.f;
        for (int k = 0; k < total; ++k) s += prow[m][__builtin_amdgcn_readfirstlane(tlist[k])];
        if (kh == 0) psum[(wv * 2 + m) * TW + l31] = pok[m] ? s : 0.f;
    }

    f32x16 acc[2][NJ];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][j][e] = 0.f;

    // the halo tiles of pass `it` (chunk it / n_grp, reference group it % n_grp) -> registers.  A thread owns the same NPK 16-byte
    // pieces (pixel, channel quad) of every staged map: their offsets inside a map and inside an LDS tile are computed once, a map's
    // base address is wave-uniform.  A piece outside the map is zero (the convolution's zero padding); a map that is not staged
    // is not requested.
    int goff[NPK], loff[NPK];
    unsigned int in_map = 0u, in_tile = 0u;
#pragma unroll
    for (int k = 0; k < NPK; ++k) {
        const int i = tid + k * 256;
        const int p = i >> 2, q = i & 3;
        const int py = p / PW, px = p - py * PW;
        const int gy = y0 + py - 1, gx = x0 + px - 1;
        const bool tile = i < NPIECE, ok = tile && gy >= 0 && gy < H && gx >= 0 && gx < W;
        goff[k] = ok ? (gy * W + gx) * C + 4 * q : 0;
        loff[k] = q * QPL + p * 16;
        in_map |= (ok ? 1u : 0u) << k, in_tile |= (tile ? 1u : 0u) << k;
    }
    float4 pf[TG][NPK];
    auto fetch = [&](const int it) {
        const int ch = it / n_grp, g = it - ch * n_grp;
        const int cnt = total - g * TG < TG ? total - g * TG : TG;
#pragma unroll
        for (int tg = 0; tg < TG; ++tg)
            if (tg < cnt) {
                const int t = __builtin_amdgcn_readfirstlane(tlist[g * TG + tg]);
                const float *base = A.refs + ((size_t)t * N + n) * H * W * C + ch * KC;
#pragma unroll
                for (int k = 0; k < NPK; ++k)
                    pf[tg][k] = ((in_map >> k) & 1u) ? *reinterpret_cast<const float4 *>(base + goff[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
    };
    if (n_it) fetch(0);

    // B fragments of one tap: NJ columns x (wh, wl); column j sits in cout block 2 cbk + (j >> 1), rows 32 (j & 1) ..
    const unsigned short *wlane = A.wp + (size_t)l31 * KC + kh * 8;
    auto bload = [&](const int lin, u32x4 (&b)[NJ][2]) {   // lin = chunk * 9 + tap
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int sp = 0; sp < 2; ++sp)
                b[j][sp] = *reinterpret_cast<const u32x4 *>(wlane + ((((size_t)(cbk * 2 + (j >> 1)) * NCH * TAPS + lin) * NW + sp) * NB + (j & 1) * 32) * KC);
    };

    bool bad = false;
    float pr[2][TG];
    for (int it = 0; it < n_it; ++it) {
        const int ch = it / n_grp, g = it - ch * n_grp;
        const int cnt = total - g * TG < TG ? total - g * TG : TG;
        if (it) __syncthreads();   // the previous pass's tiles have been read
#pragma unroll
        for (int tg = 0; tg < TG; ++tg)
            if (tg < cnt) {
#pragma unroll
                for (int k = 0; k < NPK; ++k) {
                    float4 v = pf[tg][k];
                    v.x *= in_s, v.y *= in_s, v.z *= in_s, v.w *= in_s;
                    bad = bad || !(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))) <= 65000.f);   // fp16 range guard
                    if ((in_tile >> k) & 1u) *reinterpret_cast<float4 *>(smem + tg * TPL + loff[k]) = v;
                }
            }
        __syncthreads();
        if (it + 1 < n_it) fetch(it + 1);   // the next pass's tiles travel in registers beside the MFMAs
        if (n_grp > 1 || it == 0) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int k = 0; k < TG; ++k) pr[m][k] = (k < cnt && pok[m]) ? prow[m][__builtin_amdgcn_readfirstlane(tlist[g * TG + k])] : 0.f;
        }
        u32x4 b[NJ][2];
        bload(ch * TAPS, b);
#pragma nounroll
        for (int tap = 0; tap < TAPS; ++tap) {
            const int dy = (tap * 11) >> 5, dx = tap - 3 * dy;
            u32x4 bn[NJ][2];
            if (tap + 1 < TAPS) bload(ch * TAPS + tap + 1, bn);   // the weight fragments run one tap ahead
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const unsigned char *sp = smem + (2 * kh) * QPL + ((wv * 2 + m + dy) * PW + l31 + dx) * 16;
                float u[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) u[c] = 0.f;
#pragma unroll
                for (int k = 0; k < TG; ++k)   // fma chain, t ascending over the staged (= present) maps
                    if (k < cnt) {
                        const float4 s0 = *reinterpret_cast<const float4 *>(sp + k * TPL);
                        const float4 s1 = *reinterpret_cast<const float4 *>(sp + k * TPL + QPL);
                        const float w = pr[m][k];
                        u[0] = fmaf(w, s0.x, u[0]), u[1] = fmaf(w, s0.y, u[1]), u[2] = fmaf(w, s0.z, u[2]), u[3] = fmaf(w, s0.w, u[3]);
                        u[4] = fmaf(w, s1.x, u[4]), u[5] = fmaf(w, s1.y, u[5]), u[6] = fmaf(w, s1.z, u[6]), u[7] = fmaf(w, s1.w, u[7]);
                    }
                // a = ah + al, al kept as fp16(al * 2^11): split16.h
                u32x4 ah, al;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    unsigned int h, l;
                    split_scaled(u[2 * c], u[2 * c + 1], h, l);
                    ah[c] = h, al[c] = l;
                }
                // partial products smallest first: ah wl, AL WH2 (the third weight plane wh 2^-11 is derived, not loaded), ah wh
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[m][j] = mma16(ah, b[j][1], acc[m][j]);
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[m][j] = mma16(al, scale_wh(b[j][0]), acc[m][j]);
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[m][j] = mma16(ah, b[j][0], acc[m][j]);
            }
            if (tap + 1 < TAPS) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) b[j][0] = bn[j][0], b[j][1] = bn[j][1];
            }
        }
    }
    if (bad && A.range_flag) atomicOr(A.range_flag, 1);
    __syncthreads();   // psum of every row is written (a block without a present reference ran no pass)

    // MFMA result: a lane holds cout 32 j + (lane & 31) of pixels x = (e & 3) + 8 (e >> 2) + 4 kh of row m: a store instruction
    // writes two pixels' 128 contiguous bytes
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int gy = y0 + wv * 2 + m;
        if (gy >= H) continue;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int co = cbk * (NJ * 32) + j * 32 + l31;
            const float bv = A.bias ? A.bias[co] : 0.f;
            float *orow = A.out + (((size_t)n * H + gy) * W) * COUT + co;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int x = (e & 3) + 8 * (e >> 2) + 4 * kh, gx = x0 + x;
                if (gx < W) orow[(size_t)gx * COUT] = acc[m][j][e] * oscale + bv * psum[(wv * 2 + m) * TW + x];
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
