// The convolution of the discriminators as an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32 products), for the layers of
// disc_vgg.hip (3x3 / stride 1 / pad 1, 4x4 / stride 2 / pad 1) and disc_sg2.hip (3x3 / stride 2 / pad 0, 1x1 / stride 1 / pad 0):
// the kernels, the split heuristic, the geometry and the host drivers behind the exported entry points of both files.  Each file
// lists the layers it accepts in a table of ConvLayer and so instantiates the kernels of those layers alone.  Everything here is
// local to the including translation unit.  No float atomics: every sum has a fixed order.
#pragma once
#include "disc_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// weight packing: w [Cout][CinR][T] -> dgrad 0: [Cout][T][Cin], 1: [Cin][T][Cout]; channels CinR..Cin-1 are 0
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dconv_pack_weight_kernel(const float *__restrict__ w, float *__restrict__ out, int Cout, int CinR, int Cin,
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
// The convolution GEMM of a KS x KS / stride ST (1 or 2) / pad PAD layer.  Block = 4 waves = a 64 x 64 output tile (wave (wm, wn)
// = rows 32 wm.., columns 32 wn..: 2 x 2 MFMA tiles).  k runs in chunks of 16: each thread loads one float4 of A and one of B per
// chunk into registers (the next chunk's loads are in flight while the current one is multiplied), the block stores them to LDS as
// As[row][k] / Bs[col][k] (row pitch 20 floats: the 16-lane groups of ds_read_b128 hit distinct 16-byte slots), and each lane reads
// As[row][4 q ..] / Bs[col][4 q ..] for its k-quad q = lane >> 4 and feeds element e to the e-th MFMA: the MFMA's k index 4 q + e
// is the same for A and B.
//   MODE 0: forward.  Rows m = (n, oy, ox) of [N][Ho][Wo]; k = tap Kc + c (Kc = Cin, a multiple of 4; K padded to 16 with zeros);
//           A = x at (oy ST + ky - PAD, ox ST + kx - PAD); B^T = wpk [Cout][T][Cin].
//   MODE 1: input gradient.  Rows = input pixels, k = i Kc + c (Kc = Cout) over taps i, B^T = wpk_d [Cin][T][Cout].  ST = 1: one
//           GEMM, (ky, kx) = (i / KS, i % KS), source (iy + PAD - ky, ix + PAD - kx) of dy.  ST = 2: four parity phases (py, px) =
//           blockIdx.z & 3 of the input pixels (2 yy + py, 2 xx + px), each a gather over the taps of its parity alone:
//           ky = ky0 + 2 a with ky0 = (py + PAD) & 1 and a < ny = (KS - ky0 + 1) / 2, source row yy + (py + PAD - ky0) / 2 - a,
//           the same in x, i = a nx + b.  (4x4 / pad 1: 2 x 2 taps in every phase; 3x3 / pad 0: 4, 2, 2 and 1.)
//   MODE 2: weight gradient.  Rows r = tap Kc + ci (Kc = Cin), columns co, k = output pixel q; A = x at the pixel of (q, tap),
//           B = dy [Q][Cout].
// k is split into fixed ranges, one per blockIdx.z (>> 2 with parity phases).  The partial tile of a split goes to out (S = 1,
// MODE 0 or 1; MODE 0: + bias, LeakyReLU, + res) or to ws[split], which dconv_finish / dconv_wgrad_finish add in order (the
// 10 x 10 and 5 x 5 layers have too few output tiles to fill the GPU otherwise).
// ---------------------------------------------------------------------------------------------------------------
constexpr int TM = 64, TN = 64, TK = 16, LDK = TK + 4;

struct GemmGeo {
    int N, H, W, Ho, Wo;   // input H x W, output Ho x Wo
    int Kc, Nc;            // channels per tap of k, columns (MODE 0: Cin, Cout; 1: Cout, Cin; 2: Cin, Cout)
    int cps, S;            // chunks of 16 k per split, splits
};

template <int KS, int ST, int PAD, int MODE>
__global__ __launch_bounds__(256) void dconv_gemm_kernel(const float *__restrict__ src, const float *__restrict__ wsrc, const float *__restrict__ bias,
                                                         const float *__restrict__ res, float *__restrict__ out, float *__restrict__ ws, const GemmGeo g,
                                                         float slope, int act)
{
    static_assert(ST == 1 || ST == 2, "stride 1 or 2");
    constexpr int TW = KS * KS;
    constexpr bool PH = MODE == 1 && ST == 2;   // parity phases
    __shared__ __attribute__((aligned(16))) float As[TM][LDK];
    __shared__ __attribute__((aligned(16))) float Bs[TN][LDK];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ph = PH ? (int)(blockIdx.z & 3) : 0;
    const int split = PH ? (int)(blockIdx.z >> 2) : (int)blockIdx.z;
    const int py = ph >> 1, px = ph & 1;
    const int ky0 = (py + PAD) & 1, kx0 = (px + PAD) & 1;
    // taps of the phase per axis (an even KS has KS / 2 in either parity: a constant)
    const int ny = KS % 2 ? (KS - ky0 + 1) / 2 : KS / 2, nx = KS % 2 ? (KS - kx0 + 1) / 2 : KS / 2;
    const int T = PH ? ny * nx : TW;   // taps per row of this GEMM
    // the rows' grid
    const int Hr = MODE == 0 ? g.Ho : (PH ? (g.H - py + 1) >> 1 : g.H);
    const int Wr = MODE == 0 ? g.Wo : (PH ? (g.W - px + 1) >> 1 : g.W);
    const long M = MODE == 2 ? (long)T * g.Kc : (long)g.N * Hr * Wr;
    const long m0 = (long)blockIdx.x * TM;
    if (m0 >= M) return;   // (block-uniform: a small parity phase)
    const int n0 = blockIdx.y * TN;
    const long K = MODE == 2 ? (long)g.N * g.Ho * g.Wo : (long)T * g.Kc;
    const long KC = (K + TK - 1) / TK;
    const long cb = (long)split * g.cps, ce = min(KC, cb + g.cps);

    // loader coordinates.  MODE 0/1: thread = (row tid >> 2, k-quad tid & 3) of A and (column tid >> 2, k-quad) of B, float4 along k.
    // MODE 2: thread = (k tid >> 4, 4 rows / columns from 4 (tid & 15)), float4 along the rows (channels).
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
            const int ti = MODE == 1 && TW == 1 ? 0 : (int)(k / g.Kc);   // (the 1x1 input gradient reads its own pixel: a constant tap)
            const int c = (int)(k - (long)ti * g.Kc);
            int sy, sx, rt;   // the source pixel, the tap's index in the packed weight
            if (PH) {
                const int a = (int)((unsigned)ti / (unsigned)nx), b = ti - nx * a;
                sy = ly + ((py + PAD - ky0) >> 1) - a, sx = lx + ((px + PAD - kx0) >> 1) - b, rt = (ky0 + 2 * a) * KS + kx0 + 2 * b;
            } else {
                const int ky = ti / KS, kx = ti - KS * ky;
                sy = MODE == 0 ? ly * ST + ky - PAD : ly + PAD - ky, sx = MODE == 0 ? lx * ST + kx - PAD : lx + PAD - kx;
                rt = ti;
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
            const int iy = oy * ST + ky - PAD, ix = ox * ST + kx - PAD;
            // (without padding no tap lies above or left of the input: two compares fewer in front of the load, 2 - 5 % of this pass)
            const bool in = PAD == 0 ? lrow && iy < g.H && ix < g.W : lrow && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
            if (in) va = *reinterpret_cast<const float4 *>(src + ((n * g.H + iy) * g.W + ix) * g.Kc + lci);
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
__global__ __launch_bounds__(256) void dconv_finish_kernel(const float *__restrict__ ws, const float *__restrict__ bias, const float *__restrict__ res,
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
__global__ __launch_bounds__(256) void dconv_wgrad_finish_kernel(const float *__restrict__ ws, float *__restrict__ dw, int S, int Cin, int CinR,
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
typedef void (*GemmLaunch)(dim3 grid, hipStream_t st, const float *src, const float *w, const float *bias, const float *res, float *out, float *ws,
                           const GemmGeo &g, float slope, int act);

// a layer a file accepts: its geometry and the launchers of its three GEMMs (by MODE)
struct ConvLayer {
    int ks, st, pad;
    GemmLaunch gemm[3];
};

template <int KS, int ST, int PAD, int MODE>
void launch_gemm(dim3 grid, hipStream_t st, const float *src, const float *w, const float *bias, const float *res, float *out, float *ws,
                 const GemmGeo &g, float slope, int act)
{
    hipLaunchKernelGGL((dconv_gemm_kernel<KS, ST, PAD, MODE>), grid, dim3(256), 0, st, src, w, bias, res, out, ws, g, slope, act);
}

template <int KS, int ST, int PAD>
constexpr ConvLayer conv_layer()
{
    return {KS, ST, PAD, {launch_gemm<KS, ST, PAD, 0>, launch_gemm<KS, ST, PAD, 1>, launch_gemm<KS, ST, PAD, 2>}};
}

// the layer of kernel size ks in a file's table, or null
template <int NL>
const ConvLayer *find_layer(const ConvLayer (&layers)[NL], int ks)
{
    for (const ConvLayer &l : layers)
        if (l.ks == ks) return &l;
    return nullptr;
}

int conv_out(int n, const ConvLayer &L) { return (n + 2 * L.pad - L.ks) / L.st + 1; }

int check_channels(const char *what, int Cin, int Cout)
{
    if (Cin <= 0 || Cin % 4) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: Cin=%d (a multiple of 4)", what, Cin);
    if (Cout <= 0 || Cout % 16) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: Cout=%d (a multiple of 16)", what, Cout);
    return MREFSR_OK;
}

// splits of k: ~512 blocks in all, at least 8 chunks of 16 per split
void splits(long tiles, long KC, int &cps, int &S)
{
    long s = (512 + tiles - 1) / tiles;
    const long smax = KC / 8;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    cps = (int)((KC + s - 1) / s);
    S = (int)((KC + cps - 1) / cps);
}

// the GEMM's geometry and grid of MODE (0, 1) for a layer; S and cps from splits (stride 2, MODE 1: the largest phase, of
// ceil(ks / 2)^2 taps, sizes the grid and the splits)
GemmGeo conv_geo(const ConvLayer &L, int mode, int N, int H, int W, int Cin, int Cout, dim3 &grid)
{
    GemmGeo g = {N, H, W, conv_out(H, L), conv_out(W, L), mode == 1 ? Cout : Cin, mode == 1 ? Cin : Cout, 1, 1};
    const int tp = (L.ks + 1) / 2;
    long rows, K;
    int phases = 1;
    if (mode == 0) rows = (long)N * g.Ho * g.Wo, K = (long)L.ks * L.ks * Cin;
    else if (L.st == 2) rows = (long)N * ((H + 1) / 2) * ((W + 1) / 2), K = (long)tp * tp * Cout, phases = 4;
    else rows = (long)N * H * W, K = (long)L.ks * L.ks * Cout;
    const long mt = (rows + TM - 1) / TM, nt = (g.Nc + TN - 1) / TN;
    splits(mt * nt * phases, (K + TK - 1) / TK, g.cps, g.S);
    grid = dim3((unsigned)mt, (unsigned)nt, (unsigned)(g.S * phases));
    return g;
}

GemmGeo conv_geo_wgrad(const ConvLayer &L, int N, int H, int W, int Cin, int Cout, dim3 &grid)
{
    GemmGeo g = {N, H, W, conv_out(H, L), conv_out(W, L), Cin, Cout, 1, 1};
    const long R = (long)L.ks * L.ks * Cin, Q = (long)N * g.Ho * g.Wo;
    const long mt = (R + TM - 1) / TM, nt = (Cout + TN - 1) / TN;
    splits(mt * nt, (Q + TK - 1) / TK, g.cps, g.S);
    grid = dim3((unsigned)mt, (unsigned)nt, (unsigned)g.S);
    return g;
}

// The drivers behind the exported entry points, which name themselves in `what` and have checked the layer's sizes and channels.
// L = find_layer(the file's table, ks): null for a kernel size the file does not have
int conv_pack_weight(const char *what, const ConvLayer *L, const float *w, float *wpk, int Cout, int CinR, int Cin, int ks, int dgrad,
                     mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(w && wpk, "%s: null pointer", what);
    MREFSR_REQUIRE(Cout > 0 && CinR > 0 && CinR <= Cin && L, "%s: Cout=%d CinR=%d Cin=%d ks=%d", what, Cout, CinR, Cin, ks);
    const long total = (long)ks * ks * Cin * Cout;
    hipLaunchKernelGGL(dconv_pack_weight_kernel, dim3(grid_of((total + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)stream, w, wpk, Cout, CinR, Cin,
                       ks * ks, dgrad ? 1 : 0);
    return mrefsr::check_launch(what);
}

int64_t conv_workspace_bytes(const ConvLayer &L, int N, int H, int W, int Cin, int Cout, int dgrad)
{
    dim3 grid;
    const GemmGeo g = conv_geo(L, dgrad ? 1 : 0, N, H, W, Cin, Cout, grid);
    const long pix = dgrad ? (long)N * H * W : (long)N * g.Ho * g.Wo;
    return g.S > 1 ? (int64_t)g.S * pix * g.Nc * 4 : 0;
}

// mode 0: the forward, src = x, out = y + bias, LeakyReLU (act), + res; mode 1: the input gradient, src = dy, out = dx
int conv_run(const char *what, const ConvLayer &L, int mode, const float *src, const float *wpk, const float *bias, const float *res, float *out, int N,
             int H, int W, int Cin, int Cout, int act, float slope, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    dim3 grid;
    const GemmGeo g = conv_geo(L, mode, N, H, W, Cin, Cout, grid);
    const int64_t need = conv_workspace_bytes(L, N, H, W, Cin, Cout, mode);
    MREFSR_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "%s: workspace of %ld bytes < %ld", what, (long)workspace_bytes, (long)need);
    hipStream_t st = (hipStream_t)stream;
    L.gemm[mode](grid, st, src, wpk, bias, res, out, (float *)workspace, g, slope, act ? 1 : 0);
    if (g.S > 1) {
        const long total = (mode ? (long)N * H * W : (long)N * g.Ho * g.Wo) * g.Nc;
        hipLaunchKernelGGL(dconv_finish_kernel, dim3(grid_of((total + 255) / 256, 8192)), dim3(256), 0, st, (const float *)workspace, bias, res, out,
                           total, g.S, g.Nc, slope, act ? 1 : 0);
    }
    return mrefsr::check_launch(what);
}

int64_t conv_wgrad_workspace_bytes(const ConvLayer &L, int N, int H, int W, int Cin, int Cout)
{
    dim3 grid;
    const GemmGeo g = conv_geo_wgrad(L, N, H, W, Cin, Cout, grid);
    return (int64_t)g.S * L.ks * L.ks * Cin * Cout * 4;
}

int conv_wgrad(const char *what, const ConvLayer &L, const float *x, const float *dy, float *dw, int N, int H, int W, int Cin, int CinR, int Cout,
               void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(CinR > 0 && CinR <= Cin, "%s: CinR=%d Cin=%d", what, CinR, Cin);
    const int64_t need = conv_wgrad_workspace_bytes(L, N, H, W, Cin, Cout);
    MREFSR_REQUIRE(workspace_bytes >= need, "%s: workspace of %ld bytes < %ld", what, (long)workspace_bytes, (long)need);
    dim3 grid;
    const GemmGeo g = conv_geo_wgrad(L, N, H, W, Cin, Cout, grid);
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    L.gemm[2](grid, st, x, dy, nullptr, nullptr, nullptr, ws, g, 0.f, 0);
    const long total = (long)Cout * CinR * L.ks * L.ks;
    hipLaunchKernelGGL(dconv_wgrad_finish_kernel, dim3(grid_of((total + 255) / 256, 4096)), dim3(256), 0, st, ws, dw, g.S, Cin, CinR, Cout,
                       L.ks * L.ks);
    return mrefsr::check_launch(what);
}

}  // namespace
