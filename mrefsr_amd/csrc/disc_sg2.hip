// StyleGAN2Discriminator of the adversarial training step (basicsr/archs/stylegan2_arch.py:733-799; trained by
// MultiRefRestorationModel.optimize_parameters and differentiated twice by gradient_penalty_loss): the kernels of
// mrefsr_amd/archs/nhwc_sg2disc.py that csrc/disc_vgg.hip and csrc/disc.hip do not have.  conv1 of every ResBlock and final_conv run on
// disc_vgg.hip's 3x3 / stride-1 convolution, final_linear on its linear head, the image packing and the bias gradient on disc.hip.
//   sg2_fir<ADJ>            upfirdn2d(x, outer(k, k), down d, pad (p0, p1)) on a channels-last map with a separable FIR of 2 .. 4 taps,
//                           and its adjoint (the input gradient): both gathers, each one's backward is the other
//   sconv_gemm<KS, MODE>    the convolution behind the FIR, pad 0: KS = 3 (stride 2: conv2 of a ResBlock, on the blurred
//                           (H + 1) x (W + 1) map) or KS = 1 (stride 1: the skip, on the FIR's stride-2 output, and the input stage on
//                           the packed image), as an implicit GEMM on v_mfma_f32_16x16x4_f32 with the tiling of disc_vgg.hip's
//                           vconv_gemm (64 x 64 tile per 4 waves, k in chunks of 16 through LDS):
//                             MODE 0  forward + bias + LeakyReLU + residual (the ResBlock's merge) in the epilogue
//                             MODE 1  input gradient (KS = 3: four input-parity phases of 4, 2, 2 and 1 taps)
//                             MODE 2  weight gradient
//                           with the same fixed split of k into blockIdx.z ranges added in order by sconv_finish / sconv_wgrad_finish
// No float atomics anywhere: two runs give the same bits.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

inline int grid_of(long work, int cap) { return (int)(work < 1 ? 1 : (work < cap ? work : cap)); }

__device__ inline float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// ---------------------------------------------------------------------------------------------------------------
// FIR.  kf = the taps as upfirdn2d applies them (the normalised 1-D kernel, flipped).  One thread per (pixel, 4 channels).
//   ADJ 0: out [N][Ho][Wo][C], out(oy, ox) = sum_{ky, kx} kf[ky] kf[kx] x(oy d + ky - p0, ox d + kx - p0)   (x [N][H][W][C])
//   ADJ 1: out [N][H][W][C],   out(iy, ix) = sum over (ky, kx) with (iy + p0 - ky) = d oy, (ix + p0 - kx) = d ox of
//                                             kf[ky] kf[kx] g(oy, ox)                                         (g [N][Ho][Wo][C])
// ---------------------------------------------------------------------------------------------------------------
struct Fir {
    float k[4];
    int L, p0, d;
};

template <int ADJ>
__global__ __launch_bounds__(256) void sg2_fir_kernel(const float *__restrict__ src, float *__restrict__ out, int N, int H, int W, int Ho, int Wo, int C,
                                                      const Fir f)
{
    const int C4 = C >> 2;
    const int Hd = ADJ ? H : Ho, Wd = ADJ ? W : Wo;   // the written map
    const int Hs = ADJ ? Ho : H, Ws = ADJ ? Wo : W;   // the read map
    const long total = (long)N * Hd * Wd * C4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = 4 * (int)(i % C4);
        long r = i / C4;
        const int x = (int)(r % Wd);
        r /= Wd;
        const int y = (int)(r % Hd);
        const long n = r / Hd;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int ky = 0; ky < f.L; ++ky) {
            int sy;
            if (ADJ) {
                const int t = y + f.p0 - ky;
                if (t < 0 || t % f.d) continue;
                sy = t / f.d;
            } else {
                sy = y * f.d + ky - f.p0;
            }
            if (sy < 0 || sy >= Hs) continue;
            for (int kx = 0; kx < f.L; ++kx) {
                int sx;
                if (ADJ) {
                    const int t = x + f.p0 - kx;
                    if (t < 0 || t % f.d) continue;
                    sx = t / f.d;
                } else {
                    sx = x * f.d + kx - f.p0;
                }
                if (sx < 0 || sx >= Ws) continue;
                const float wgt = f.k[ky] * f.k[kx];
                const float4 v = *reinterpret_cast<const float4 *>(src + ((n * Hs + sy) * Ws + sx) * C + c);
                acc.x += wgt * v.x, acc.y += wgt * v.y, acc.z += wgt * v.z, acc.w += wgt * v.w;
            }
        }
        *reinterpret_cast<float4 *>(out + ((n * Hd + y) * Wd + x) * C + c) = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// weight packing: w [Cout][CinR][T] -> dgrad 0: [Cout][T][Cin], 1: [Cin][T][Cout]; channels CinR..Cin-1 are 0
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sconv_pack_weight_kernel(const float *__restrict__ w, float *__restrict__ out, int Cout, int CinR, int Cin,
                                                                int T, int dgrad)
{
    const long total = (long)T * Cin * Cout;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int ci, co, t;
        if (dgrad) {
            co = (int)(i % Cout);
            const long r = i / Cout;
            t = (int)(r % T), ci = (int)(r / T);
        } else {
            ci = (int)(i % Cin);
            const long r = i / Cin;
            t = (int)(r % T), co = (int)(r / T);
        }
        out[i] = ci < CinR ? w[((long)co * CinR + ci) * T + t] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The convolution GEMM (pad 0; stride ST = 2 for KS = 3, 1 for KS = 1).  Tiling, LDS layout and MFMA feeding as vconv_gemm of
// disc_vgg.hip: block = 4 waves = a 64 x 64 tile, k in chunks of 16, As[row][k] / Bs[col][k] with a row pitch of 20 floats.
//   MODE 0: rows m = (n, oy, ox) of [N][Ho][Wo]; k = tap Kc + c (Kc = Cin); A = x at (oy ST + ky, ox ST + kx); B^T = wpk [Cout][T][Cin].
//   MODE 1: rows = input pixels.  KS = 1: one tap, source = the same pixel.  KS = 3: phase (py, px) = blockIdx.z & 3 holds the input
//           pixels (2 yy + py, 2 xx + px); its taps are ky = py + 2 a (a < 2 - py), kx = px + 2 b (b < 2 - px): k = (a (2 - px) + b) Kc
//           + c (Kc = Cout), source (yy - a, xx - b) of dy.  B^T = wpk_d [Cin][T][Cout].
//   MODE 2: rows r = tap Kc + ci (Kc = Cin), columns co, k = output pixel q; A = x at the pixel of (q, tap), B = dy [Q][Cout].
// The partial tile of split blockIdx.z (>> 2 for MODE 1, KS = 3) goes to out (S = 1, MODE 0: + bias, LeakyReLU, + res) or to ws[split].
// ---------------------------------------------------------------------------------------------------------------
constexpr int TM = 64, TN = 64, TK = 16, LDK = TK + 4;

struct SGeo {
    int N, H, W, Ho, Wo;   // input H x W, output Ho x Wo
    int Kc, Nc;            // channels per tap of k, columns (MODE 0: Cin, Cout; 1: Cout, Cin; 2: Cin, Cout)
    int cps, S;            // chunks of 16 k per split, splits
};

template <int KS, int MODE>
__global__ __launch_bounds__(256) void sconv_gemm_kernel(const float *__restrict__ src, const float *__restrict__ wsrc, const float *__restrict__ bias,
                                                         const float *__restrict__ res, float *__restrict__ out, float *__restrict__ ws, const SGeo g,
                                                         float slope, int act)
{
    constexpr int ST = KS == 3 ? 2 : 1;
    constexpr int TW = KS * KS;
    constexpr bool PH = MODE == 1 && KS == 3;   // parity phases
    __shared__ __attribute__((aligned(16))) float As[TM][LDK];
    __shared__ __attribute__((aligned(16))) float Bs[TN][LDK];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ph = PH ? (int)(blockIdx.z & 3) : 0;
    const int split = PH ? (int)(blockIdx.z >> 2) : (int)blockIdx.z;
    const int py = ph >> 1, px = ph & 1;
    const int nx = 2 - px;
    const int T = MODE == 1 ? (PH ? (2 - py) * nx : 1) : TW;   // taps per row of this GEMM
    const int Hr = MODE == 0 ? g.Ho : (PH ? (g.H - py + 1) >> 1 : g.H);
    const int Wr = MODE == 0 ? g.Wo : (PH ? (g.W - px + 1) >> 1 : g.W);
    const long M = MODE == 2 ? (long)T * g.Kc : (long)g.N * Hr * Wr;
    const long m0 = (long)blockIdx.x * TM;
    if (m0 >= M) return;   // (block-uniform: a small parity phase)
    const int n0 = blockIdx.y * TN;
    const long K = MODE == 2 ? (long)g.N * g.Ho * g.Wo : (long)T * g.Kc;
    const long KC = (K + TK - 1) / TK;
    const long cb = (long)split * g.cps, ce = min(KC, cb + g.cps);

    int ln = 0, ly = 0, lx = 0;   // MODE 0/1: the pixel of the A row
    bool lrow = false;
    int ltap = 0, lci = 0;        // MODE 2: the (tap, ci) of the A rows
    if (MODE != 2) {
        const long m = m0 + (tid >> 2);
        lrow = m < M;
        const long mm = lrow ? m : 0;
        lx = (int)(mm % Wr);
        const long q = mm / Wr;
        ly = (int)(q % Hr);
        ln = (int)(q / Hr);
    } else {
        const long r = m0 + 4 * (tid & 15);
        lrow = r < M;
        ltap = lrow ? (int)(r / g.Kc) : 0;
        lci = lrow ? (int)(r - (long)ltap * g.Kc) : 0;
    }
    const int bcol = MODE != 2 ? n0 + (tid >> 2) : n0 + 4 * (tid & 15);
    const bool bok = bcol < g.Nc;

    auto load = [&](long ch, float4 &va, float4 &vb) {
        va = vb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MODE != 2) {
            const long k = ch * TK + 4 * (tid & 3);
            if (k >= K) return;
            const int ti = (int)(k / g.Kc), c = (int)(k - (long)ti * g.Kc);
            int sy, sx, rt;
            if (MODE == 0) {
                const int ky = ti / KS, kx = ti - KS * (ti / KS);
                sy = ly * ST + ky, sx = lx * ST + kx, rt = ti;
            } else if (PH) {
                const int a = ti / nx, b = ti - nx * (ti / nx);
                sy = ly - a, sx = lx - b, rt = (py + 2 * a) * 3 + (px + 2 * b);
            } else {
                sy = ly, sx = lx, rt = 0;
            }
            const int Hs = MODE == 0 ? g.H : g.Ho, Ws = MODE == 0 ? g.W : g.Wo;
            if (lrow && sy >= 0 && sy < Hs && sx >= 0 && sx < Ws)
                va = *reinterpret_cast<const float4 *>(src + (((long)ln * Hs + sy) * Ws + sx) * g.Kc + c);
            if (bok) vb = *reinterpret_cast<const float4 *>(wsrc + ((long)bcol * TW + rt) * g.Kc + c);
        } else {
            const long q = ch * TK + (tid >> 4);
            if (q >= K) return;
            const int ox = (int)(q % g.Wo);
            const long t2 = q / g.Wo;
            const int oy = (int)(t2 % g.Ho);
            const long n = t2 / g.Ho;
            const int ky = ltap / KS, kx = ltap - KS * (ltap / KS);
            const int iy = oy * ST + ky, ix = ox * ST + kx;
            if (lrow && iy < g.H && ix < g.W) va = *reinterpret_cast<const float4 *>(src + ((n * g.H + iy) * g.W + ix) * g.Kc + lci);
            if (bok) vb = *reinterpret_cast<const float4 *>(wsrc + q * g.Nc + bcol);
        }
    };
    auto store = [&](const float4 &va, const float4 &vb) {
        if (MODE != 2) {
            *reinterpret_cast<float4 *>(&As[tid >> 2][4 * (tid & 3)]) = va;
            *reinterpret_cast<float4 *>(&Bs[tid >> 2][4 * (tid & 3)]) = vb;
        } else {
            const int k = tid >> 4, r = 4 * (tid & 15);
            As[r][k] = va.x, As[r + 1][k] = va.y, As[r + 2][k] = va.z, As[r + 3][k] = va.w;
            Bs[r][k] = vb.x, Bs[r + 1][k] = vb.y, Bs[r + 2][k] = vb.z, Bs[r + 3][k] = vb.w;
        }
    };

    const int wm = wave & 1, wn = wave >> 1, l16 = lane & 15, kq = lane >> 4;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 pa, pb;
    if (cb < ce) load(cb, pa, pb);
    for (long ch = cb; ch < ce; ++ch) {
        __syncthreads();
        store(pa, pb);
        __syncthreads();
        if (ch + 1 < ce) load(ch + 1, pa, pb);
        float4 a4[2], b4[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a4[i] = *reinterpret_cast<const float4 *>(&As[wm * 32 + 16 * i + l16][4 * kq]);
#pragma unroll
        for (int j = 0; j < 2; ++j) b4[j] = *reinterpret_cast<const float4 *>(&Bs[wn * 32 + 16 * j + l16][4 * kq]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[i][e], b4[j][e], acc[i][j], 0, 0, 0);
    }

    // store: row m0 + 32 wm + 16 i + 4 kq + r, column n0 + 32 wn + 16 j + l16
    const long plane = (MODE == 2 ? M : (MODE == 0 ? (long)g.N * g.Ho * g.Wo : (long)g.N * g.H * g.W)) * g.Nc;   // one split's partials
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long m = m0 + 32 * wm + 16 * i + 4 * kq + r;
            if (m >= M) continue;
            long orow = m;   // the output's row: MODE 0: the output pixel, 1: the input pixel, 2: (tap, ci)
            if (PH) {
                const int xx = (int)(m % Wr);
                const long q = m / Wr;
                const int yy = (int)(q % Hr);
                const long nn = q / Hr;
                orow = (nn * g.H + 2 * yy + py) * g.W + 2 * xx + px;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = n0 + 32 * wn + 16 * j + l16;
                if (col >= g.Nc) continue;
                float v = acc[i][j][r];
                if (g.S > 1 || MODE == 2) {
                    ws[(long)split * plane + orow * g.Nc + col] = v;
                } else {
                    if (MODE == 0 && bias) v += bias[col];
                    if (MODE == 0 && act) v = lrelu(v, slope);
                    if (MODE == 0 && res) v += res[orow * g.Nc + col];
                    out[orow * g.Nc + col] = v;
                }
            }
        }
}

// out[i] = sum_s ws[s][i] in order (+ bias, LeakyReLU, + res)
__global__ __launch_bounds__(256) void sconv_finish_kernel(const float *__restrict__ ws, const float *__restrict__ bias, const float *__restrict__ res,
                                                           float *__restrict__ out, long total, int S, int Nc, float slope, int act)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int s = 0; s < S; ++s) v += ws[(long)s * total + i];
        if (bias) v += bias[i % Nc];
        if (act) v = lrelu(v, slope);
        if (res) v += res[i];
        out[i] = v;
    }
}

// dw [Cout][CinR][T] = sum_s ws[s][t Cin + ci][co] in order
__global__ __launch_bounds__(256) void sconv_wgrad_finish_kernel(const float *__restrict__ ws, float *__restrict__ dw, int S, int Cin, int CinR,
                                                                 int Cout, int T)
{
    const long total = (long)Cout * CinR * T;
    const long R = (long)T * Cin;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int t = (int)(i % T);
        const long r = i / T;
        const int ci = (int)(r % CinR);
        const int co = (int)(r / CinR);
        const long src = ((long)t * Cin + ci) * Cout + co;
        float acc = 0.f;
        for (int s = 0; s < S; ++s) acc += ws[(long)s * R * Cout + src];
        dw[i] = acc;
    }
}

// ------------------------------------------------------------------------------------------------- host side
int sout(int n, int ks) { return ks == 3 ? (n - 3) / 2 + 1 : n; }

// splits of k: ~512 blocks in all, at least 8 chunks of 16 per split
void ssplits(long tiles, long KC, int &cps, int &S)
{
    long s = (512 + tiles - 1) / tiles;
    const long smax = KC / 8;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    cps = (int)((KC + s - 1) / s);
    S = (int)((KC + cps - 1) / cps);
}

int check_sconv(const char *what, int N, int H, int W, int Cin, int Cout, int ks)
{
    if (ks != 1 && ks != 3) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: kernel size %d (1: stride 1, 3: stride 2; pad 0)", what, ks);
    if (N <= 0 || H < ks || W < ks) return mrefsr::fail(MREFSR_E_INVALID, "%s: N=%d H=%d W=%d", what, N, H, W);
    if (Cin <= 0 || Cin % 4) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: Cin=%d (a multiple of 4)", what, Cin);
    if (Cout <= 0 || Cout % 16) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: Cout=%d (a multiple of 16)", what, Cout);
    return MREFSR_OK;
}

// the GEMM's geometry and grid of MODE (0, 1) for a layer; S and cps from ssplits (MODE 1, ks 3: of the largest phase, 2 x 2 taps)
SGeo sgeo(int mode, int N, int H, int W, int Cin, int Cout, int ks, dim3 &grid)
{
    SGeo g = {N, H, W, sout(H, ks), sout(W, ks), mode == 1 ? Cout : Cin, mode == 1 ? Cin : Cout, 1, 1};
    long rows, K;
    int phases = 1;
    if (mode == 0) rows = (long)N * g.Ho * g.Wo, K = (long)ks * ks * Cin;
    else if (ks == 3) rows = (long)N * ((H + 1) / 2) * ((W + 1) / 2), K = 4L * Cout, phases = 4;
    else rows = (long)N * H * W, K = Cout;
    const long mt = (rows + TM - 1) / TM, nt = (g.Nc + TN - 1) / TN;
    ssplits(mt * nt * phases, (K + TK - 1) / TK, g.cps, g.S);
    grid = dim3((unsigned)mt, (unsigned)nt, (unsigned)(g.S * phases));
    return g;
}

SGeo sgeo_wgrad(int N, int H, int W, int Cin, int Cout, int ks, dim3 &grid)
{
    SGeo g = {N, H, W, sout(H, ks), sout(W, ks), Cin, Cout, 1, 1};
    const long R = (long)ks * ks * Cin, Q = (long)N * g.Ho * g.Wo;
    const long mt = (R + TM - 1) / TM, nt = (Cout + TN - 1) / TN;
    ssplits(mt * nt, (Q + TK - 1) / TK, g.cps, g.S);
    grid = dim3((unsigned)mt, (unsigned)nt, (unsigned)g.S);
    return g;
}

template <int MODE>
void launch_sgemm(int ks, dim3 grid, hipStream_t st, const float *src, const float *w, const float *bias, const float *res, float *out, float *ws,
                  const SGeo &g, float slope, int act)
{
    if (ks == 3) hipLaunchKernelGGL((sconv_gemm_kernel<3, MODE>), grid, dim3(256), 0, st, src, w, bias, res, out, ws, g, slope, act);
    else hipLaunchKernelGGL((sconv_gemm_kernel<1, MODE>), grid, dim3(256), 0, st, src, w, bias, res, out, ws, g, slope, act);
}

int fir_out(int n, int L, int p0, int p1, int d) { return (n + p0 + p1 - L) / d + 1; }

int check_fir(const char *what, int N, int H, int W, int C, const float *taps, int L, int p0, int p1, int d)
{
    if (!taps || L < 2 || L > 4) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: a separable FIR of 2 .. 4 taps (got %d)", what, L);
    if (d != 1 && d != 2) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: down=%d (1 or 2)", what, d);
    if (p0 < 0 || p1 < 0 || p0 >= L || p1 >= L) return mrefsr::fail(MREFSR_E_INVALID, "%s: pad (%d, %d) for %d taps", what, p0, p1, L);
    if (N <= 0 || C <= 0 || C % 4) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: N=%d C=%d (C a multiple of 4)", what, N, C);
    if (H + p0 + p1 < L || W + p0 + p1 < L) return mrefsr::fail(MREFSR_E_INVALID, "%s: H=%d W=%d", what, H, W);
    return MREFSR_OK;
}

Fir make_fir(const float *taps, int L, int p0, int d)
{
    Fir f = {{0.f, 0.f, 0.f, 0.f}, L, p0, d};
    for (int i = 0; i < L; ++i) f.k[i] = taps[L - 1 - i];   // upfirdn2d convolves: the kernel is applied flipped
    return f;
}

}  // namespace

MREFSR_EXPORT int mrefsr_disc_sg2_fir_f32(const float *x, float *y, int N, int H, int W, int C, const float *taps, int L, int pad0, int pad1, int down,
                                          int adjoint, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && y, "disc_sg2_fir: null pointer");
    int rc = check_fir("disc_sg2_fir", N, H, W, C, taps, L, pad0, pad1, down);
    if (rc) return rc;
    const int Ho = fir_out(H, L, pad0, pad1, down), Wo = fir_out(W, L, pad0, pad1, down);
    const Fir f = make_fir(taps, L, pad0, down);
    const long total = (long)N * (adjoint ? (long)H * W : (long)Ho * Wo) * (C / 4);
    const dim3 grid(grid_of((total + 255) / 256, 16384));
    if (adjoint) hipLaunchKernelGGL(sg2_fir_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, Ho, Wo, C, f);
    else hipLaunchKernelGGL(sg2_fir_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, Ho, Wo, C, f);
    return mrefsr::check_launch("disc_sg2_fir");
}

MREFSR_EXPORT int mrefsr_disc_sg2_pack_weight_f32(const float *w, float *wpk, int Cout, int CinR, int Cin, int ks, int dgrad, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(w && wpk, "disc_sg2_pack_weight: null pointer");
    MREFSR_REQUIRE(Cout > 0 && CinR > 0 && CinR <= Cin && (ks == 1 || ks == 3), "disc_sg2_pack_weight: Cout=%d CinR=%d Cin=%d ks=%d", Cout, CinR,
                   Cin, ks);
    const long total = (long)ks * ks * Cin * Cout;
    hipLaunchKernelGGL(sconv_pack_weight_kernel, dim3(grid_of((total + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)stream, w, wpk, Cout, CinR, Cin,
                       ks * ks, dgrad ? 1 : 0);
    return mrefsr::check_launch("disc_sg2_pack_weight");
}

MREFSR_EXPORT int64_t mrefsr_disc_sg2_conv_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks, int dgrad)
{
    if (check_sconv("disc_sg2_conv_workspace_bytes", N, H, W, Cin, Cout, ks)) return -1;
    dim3 grid;
    const SGeo g = sgeo(dgrad ? 1 : 0, N, H, W, Cin, Cout, ks, grid);
    const long pix = dgrad ? (long)N * H * W : (long)N * g.Ho * g.Wo;
    return g.S > 1 ? (int64_t)g.S * pix * g.Nc * 4 : 0;
}

MREFSR_EXPORT int mrefsr_disc_sg2_conv_f32(const float *x, const float *wpk, const float *bias, const float *res, float *y, int N, int H, int W, int Cin,
                                           int Cout, int ks, int act, float slope, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && wpk && y, "disc_sg2_conv: null pointer");
    int rc = check_sconv("disc_sg2_conv", N, H, W, Cin, Cout, ks);
    if (rc) return rc;
    dim3 grid;
    const SGeo g = sgeo(0, N, H, W, Cin, Cout, ks, grid);
    const int64_t need = mrefsr_disc_sg2_conv_workspace_bytes(N, H, W, Cin, Cout, ks, 0);
    MREFSR_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "disc_sg2_conv: workspace of %ld bytes < %ld", (long)workspace_bytes, (long)need);
    hipStream_t st = (hipStream_t)stream;
    launch_sgemm<0>(ks, grid, st, x, wpk, bias, res, y, (float *)workspace, g, slope, act ? 1 : 0);
    if (g.S > 1) {
        const long total = (long)N * g.Ho * g.Wo * Cout;
        hipLaunchKernelGGL(sconv_finish_kernel, dim3(grid_of((total + 255) / 256, 8192)), dim3(256), 0, st, (const float *)workspace, bias, res, y,
                           total, g.S, Cout, slope, act ? 1 : 0);
    }
    return mrefsr::check_launch("disc_sg2_conv");
}

MREFSR_EXPORT int mrefsr_disc_sg2_conv_dgrad_f32(const float *dy, const float *wpk_d, float *dx, int N, int H, int W, int Cin, int Cout, int ks,
                                                 void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(dy && wpk_d && dx, "disc_sg2_conv_dgrad: null pointer");
    int rc = check_sconv("disc_sg2_conv_dgrad", N, H, W, Cin, Cout, ks);
    if (rc) return rc;
    dim3 grid;
    const SGeo g = sgeo(1, N, H, W, Cin, Cout, ks, grid);
    const int64_t need = mrefsr_disc_sg2_conv_workspace_bytes(N, H, W, Cin, Cout, ks, 1);
    MREFSR_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "disc_sg2_conv_dgrad: workspace of %ld bytes < %ld", (long)workspace_bytes,
                   (long)need);
    hipStream_t st = (hipStream_t)stream;
    launch_sgemm<1>(ks, grid, st, dy, wpk_d, nullptr, nullptr, dx, (float *)workspace, g, 0.f, 0);
    if (g.S > 1) {
        const long total = (long)N * H * W * Cin;
        hipLaunchKernelGGL(sconv_finish_kernel, dim3(grid_of((total + 255) / 256, 8192)), dim3(256), 0, st, (const float *)workspace, nullptr, nullptr,
                           dx, total, g.S, Cin, 0.f, 0);
    }
    return mrefsr::check_launch("disc_sg2_conv_dgrad");
}

MREFSR_EXPORT int64_t mrefsr_disc_sg2_conv_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks)
{
    if (check_sconv("disc_sg2_conv_wgrad_workspace_bytes", N, H, W, Cin, Cout, ks)) return -1;
    dim3 grid;
    const SGeo g = sgeo_wgrad(N, H, W, Cin, Cout, ks, grid);
    return (int64_t)g.S * ks * ks * Cin * Cout * 4;
}

MREFSR_EXPORT int mrefsr_disc_sg2_conv_wgrad_f32(const float *x, const float *dy, float *dw, int N, int H, int W, int Cin, int CinR, int Cout, int ks,
                                                 void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && dy && dw && workspace, "disc_sg2_conv_wgrad: null pointer");
    int rc = check_sconv("disc_sg2_conv_wgrad", N, H, W, Cin, Cout, ks);
    if (rc) return rc;
    MREFSR_REQUIRE(CinR > 0 && CinR <= Cin, "disc_sg2_conv_wgrad: CinR=%d Cin=%d", CinR, Cin);
    const int64_t need = mrefsr_disc_sg2_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout, ks);
    MREFSR_REQUIRE(workspace_bytes >= need, "disc_sg2_conv_wgrad: workspace of %ld bytes < %ld", (long)workspace_bytes, (long)need);
    dim3 grid;
    const SGeo g = sgeo_wgrad(N, H, W, Cin, Cout, ks, grid);
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    launch_sgemm<2>(ks, grid, st, x, dy, nullptr, nullptr, nullptr, ws, g, 0.f, 0);
    const long total = (long)Cout * CinR * ks * ks;
    hipLaunchKernelGGL(sconv_wgrad_finish_kernel, dim3(grid_of((total + 255) / 256, 4096)), dim3(256), 0, st, ws, dw, g.S, Cin, CinR, Cout, ks * ks);
    return mrefsr::check_launch("disc_sg2_conv_wgrad");
}
