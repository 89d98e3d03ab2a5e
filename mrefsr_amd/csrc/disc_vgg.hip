// VGGStyleDiscriminator of the adversarial training step (basicsr/archs/discriminator_arch.py:47-125, input_size 160; trained by
// MultiRefRestorationModel.optimize_parameters and differentiated twice by gradient_penalty_loss, basicsr/models/losses.py:370-404):
// the kernels of mrefsr_amd/archs/nhwc_vggdisc.py that csrc/disc.hip does not have.  BatchNorm + LeakyReLU and the image packing are
// disc.hip's entry points, used as they are.
//   vconv_pack_weight       torch's [Cout][CinR][KS][KS] -> [Cout][T][Cin] (forward) or [Cin][T][Cout] (input gradient), T = KS * KS
//   vconv_gemm<KS, MODE>    KS = 3 (stride 1) or 4 (stride 2), pad 1, as an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32
//                           products) with the operand tiles staged in LDS:
//                             MODE 0  forward (rows = output pixels, k = (tap, cin)) + bias + LeakyReLU (optional epilogue)
//                             MODE 1  input gradient (rows = input pixels; a 4x4 / stride-2 layer runs as four output-parity phases,
//                                     each a gather over exactly 2 x 2 taps)
//                             MODE 2  weight gradient (rows = (tap, cin), columns = cout, k = output pixels)
//                           a fixed split of k into blockIdx.z ranges whose partial tiles vconv_finish / vconv_wgrad_finish add in
//                           order (the 10 x 10 and 5 x 5 layers have too few output tiles to fill the GPU otherwise)
//   lrelu_mask              g lrelu'(y), the mask from the output's sign (backward and double backward of conv0_0's LeakyReLU)
//   lin_*                   the head: NCHW flatten of f [N][HW][C] -> Linear(C HW, J) -> LeakyReLU -> Linear(J, 1): forward,
//                           backward, double backward (linear1's weight is read in torch's [J][C HW] layout, feature c HW + p)
// No float atomics anywhere: two runs give the same bits.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

inline int grid_of(long work, int cap) { return (int)(work < 1 ? 1 : (work < cap ? work : cap)); }

__device__ inline float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// ---------------------------------------------------------------------------------------------------------------
// weight packing: w [Cout][CinR][KS][KS] -> dgrad 0: [Cout][T][Cin], 1: [Cin][T][Cout]; channels CinR..Cin-1 are 0
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vconv_pack_weight_kernel(const float *__restrict__ w, float *__restrict__ out, int Cout, int CinR, int Cin,
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
// The convolution GEMM.  Block = 4 waves = a 64 x 64 output tile (wave (wm, wn) = rows 32 wm.., columns 32 wn..: 2 x 2 MFMA tiles).
// k runs in chunks of 16: each thread loads one float4 of A and one of B per chunk into registers (the next chunk's loads are in
// flight while the current one is multiplied), the block stores them to LDS as As[row][k] / Bs[col][k] (row pitch 20 floats:
// the 16-lane groups of ds_read_b128 hit distinct 16-byte slots), and each lane reads As[row][4 q ..] / Bs[col][4 q ..] for its
// k-quad q = lane >> 4 and feeds element e to the e-th MFMA: the MFMA's k index 4 q + e is the same for A and B.
//   MODE 0: rows m = (n, oy, ox) of [N][Ho][Wo]; k = tap Kc + c (Kc = Cin, a multiple of 4; K padded to 16 with zeros); A = x at
//           (oy s + ky - 1, ox s + kx - 1); B^T = wpk [Cout][T][Cin].
//   MODE 1: phase (py, px) = blockIdx.z & 3 for KS = 4 (input rows iy = 2 yy + py), one phase for KS = 3; k = i Kc + c (Kc = Cout)
//           over the phase's taps: KS = 4: i = 2 a + b, (ky, kx) = (1 - py + 2 a, 1 - px + 2 b), source (yy + py - a, xx + px - b);
//           KS = 3: (ky, kx) = (i / 3, i % 3), source (iy + 1 - ky, ix + 1 - kx).  B^T = wpk_d [Cin][T][Cout].
//   MODE 2: rows r = tap Kc + ci (Kc = Cin), columns co, k = output pixel q; A = x at the pixel of (q, tap), B = dy [Q][Cout].
// The partial tile of split blockIdx.z (>> 2 for MODE 1, KS = 4) goes to out (S = 1: + bias, LeakyReLU) or to ws[split].
// ---------------------------------------------------------------------------------------------------------------
constexpr int TM = 64, TN = 64, TK = 16, LDK = TK + 4;

struct VGeo {
    int N, H, W, Ho, Wo;   // input H x W, output Ho x Wo
    int Kc, Nc;            // channels per tap of k, columns (MODE 0: Cin, Cout; 1: Cout, Cin; 2: Cin, Cout)
    int cps, S;            // chunks of 16 k per split, splits
};

template <int KS, int MODE>
__global__ __launch_bounds__(256) void vconv_gemm_kernel(const float *__restrict__ src, const float *__restrict__ wsrc, const float *__restrict__ bias,
                                                         float *__restrict__ out, float *__restrict__ ws, const VGeo g, float slope, int act)
{
    constexpr int S_ = KS == 4 ? 2 : 1;                       // stride
    constexpr int T = MODE == 1 ? (KS == 4 ? 4 : 9) : KS * KS;  // taps per row of this GEMM
    __shared__ __attribute__((aligned(16))) float As[TM][LDK];
    __shared__ __attribute__((aligned(16))) float Bs[TN][LDK];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ph = MODE == 1 && KS == 4 ? (int)(blockIdx.z & 3) : 0;
    const int split = MODE == 1 && KS == 4 ? (int)(blockIdx.z >> 2) : (int)blockIdx.z;
    const int py = ph >> 1, px = ph & 1;
    // the rows' grid
    const int Hr = MODE == 0 ? g.Ho : (MODE == 1 ? (KS == 4 ? (g.H - py + 1) >> 1 : g.H) : 0);
    const int Wr = MODE == 0 ? g.Wo : (MODE == 1 ? (KS == 4 ? (g.W - px + 1) >> 1 : g.W) : 0);
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
            const int ti = (int)(k / g.Kc), c = (int)(k - (long)ti * g.Kc);
            int sy, sx, rt;
            if (MODE == 0) {
                const int ky = ti / KS, kx = ti - KS * (ti / KS);
                sy = ly * S_ + ky - 1, sx = lx * S_ + kx - 1, rt = ti;
            } else if (KS == 4) {
                const int a = ti >> 1, b = ti & 1;
                sy = ly + py - a, sx = lx + px - b, rt = (1 - py + 2 * a) * 4 + (1 - px + 2 * b);
            } else {
                const int ky = ti / 3, kx = ti - 3 * (ti / 3);
                sy = ly + 1 - ky, sx = lx + 1 - kx, rt = ti;
            }
            const int Hs = MODE == 0 ? g.H : g.Ho, Ws = MODE == 0 ? g.W : g.Wo;
            if (lrow && sy >= 0 && sy < Hs && sx >= 0 && sx < Ws)
                va = *reinterpret_cast<const float4 *>(src + (((long)ln * Hs + sy) * Ws + sx) * g.Kc + c);
            if (bok) {
                const int Tw = KS * KS;
                vb = *reinterpret_cast<const float4 *>(wsrc + ((long)bcol * Tw + rt) * g.Kc + c);
            }
        } else {
            const long q = ch * TK + (tid >> 4);
            if (q >= K) return;
            const int ox = (int)(q % g.Wo);
            const long t2 = q / g.Wo;
            const int oy = (int)(t2 % g.Ho);
            const long n = t2 / g.Ho;
            const int ky = ltap / KS, kx = ltap - KS * (ltap / KS);
            const int iy = oy * S_ + ky - 1, ix = ox * S_ + kx - 1;
            if (lrow && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)
                va = *reinterpret_cast<const float4 *>(src + ((n * g.H + iy) * g.W + ix) * g.Kc + lci);
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
            if (MODE == 1) {
                const int xx = (int)(m % Wr);
                const long q = m / Wr;
                const int yy = (int)(q % Hr);
                const long nn = q / Hr;
                const int iy = KS == 4 ? 2 * yy + py : yy, ix = KS == 4 ? 2 * xx + px : xx;
                orow = (nn * g.H + iy) * g.W + ix;
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
                    out[orow * g.Nc + col] = v;
                }
            }
        }
}

// out[i] = sum_s ws[s][i] in order (+ bias, LeakyReLU)
__global__ __launch_bounds__(256) void vconv_finish_kernel(const float *__restrict__ ws, const float *__restrict__ bias, float *__restrict__ out,
                                                           long total, int S, int Nc, float slope, int act)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int s = 0; s < S; ++s) v += ws[(long)s * total + i];
        if (bias) v += bias[i % Nc];
        out[i] = act ? lrelu(v, slope) : v;
    }
}

// dw [Cout][CinR][T] = sum_s ws[s][t Cin + ci][co] in order
__global__ __launch_bounds__(256) void vconv_wgrad_finish_kernel(const float *__restrict__ ws, float *__restrict__ dw, int S, int Cin, int CinR,
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

// g lrelu'(y): out[i] = g[i] (y[i] > 0) + slope g[i] (y[i] <= 0)
__global__ __launch_bounds__(256) void lrelu_mask_kernel(const float *__restrict__ g, const float *__restrict__ y, float *__restrict__ out, long total,
                                                         float slope)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
        out[i] = y[i] > 0.f ? g[i] : g[i] * slope;
}

// ---------------------------------------------------------------------------------------------------------------
// Head.  f [N][HW][C] channels-last, read in the NCHW flatten order of the reference's view(B, -1): feature k = c HW + p sits at
// f[n][p][c].  W1 [J][K] (K = C HW), b1 [J], W2 [J], b2 [1].  h = W1 f + b1 (saved), out = b2 + sum_j W2 lrelu(h).
// Backward from gs = d / d out: GH[n][j] = gs[n] W2[j] lrelu'(h[n][j]); gf = W1^T GH; dW1 = GH (x) f; db1 = sum_n GH;
// dW2[j] = sum_n gs[n] lrelu(h[n][j]); db2 = sum_n gs.  Double backward for an upstream ggf of gf alone: V = W1 ggf;
// d gs[n] = sum_j W2[j] lrelu'(h) V; dW1 = GH (x) ggf; dW2[j] = sum_n gs[n] lrelu'(h[n][j]) V[n][j]; d f, d b1, d b2 = 0.
// ---------------------------------------------------------------------------------------------------------------
__device__ inline float block_sum_256(float v, float *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__device__ inline long feat_index(long k, int HW, int C) { return (k % HW) * C + k / HW; }   // NCHW feature k -> [HW][C] offset

// one block per j: rows[n][j] = sum_k W1[j][k] F[n][k] (+ b1[j]), per thread over k = tid + 256 i, then a fixed tree
__global__ __launch_bounds__(256) void lin_rows_kernel(const float *__restrict__ F, const float *__restrict__ w1, const float *__restrict__ b1,
                                                       float *__restrict__ rows, int N, int HW, int C, int J)
{
    __shared__ float red[256];
    const int j = blockIdx.x;
    const long K = (long)HW * C;
    const float *wr = w1 + (long)j * K;
    for (int n = 0; n < N; ++n) {
        const float *fn = F + (long)n * K;
        float part = 0.f;
        for (long k = threadIdx.x; k < K; k += 256) part += wr[k] * fn[feat_index(k, HW, C)];
        const float s = block_sum_256(part, red);
        if (threadIdx.x == 0) rows[(long)n * J + j] = b1 ? s + b1[j] : s;
    }
}

// one thread per image: MODE 0: out[n] = b2 + sum_j W2 lrelu(h); 1: d gs[n] = sum_j W2 lrelu'(h) V
template <int MODE>
__global__ __launch_bounds__(64) void lin_out_kernel(const float *__restrict__ h, const float *__restrict__ V, const float *__restrict__ w2,
                                                     const float *__restrict__ b2, float *__restrict__ out, int N, int J, float slope)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float acc = 0.f;
    for (int j = 0; j < J; ++j) {
        const float hv = h[(long)n * J + j];
        acc += MODE == 0 ? w2[j] * lrelu(hv, slope) : w2[j] * (hv > 0.f ? 1.f : slope) * V[(long)n * J + j];
    }
    out[n] = MODE == 0 ? acc + b2[0] : acc;
}

// one thread per (n, k): gf[n][p][c] = sum_j W1[j][k] GH[n][j]
__global__ __launch_bounds__(256) void lin_gf_kernel(const float *__restrict__ gs, const float *__restrict__ h, const float *__restrict__ w1,
                                                     const float *__restrict__ w2, float *__restrict__ gf, int N, int HW, int C, int J, float slope)
{
    const long K = (long)HW * C, total = (long)N * K;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int n = (int)(i / K);
        const long k = i - (long)n * K;
        const float gsn = gs[n];
        float acc = 0.f;
        for (int j = 0; j < J; ++j) {
            const float gh = gsn * w2[j] * (h[(long)n * J + j] > 0.f ? 1.f : slope);
            acc += w1[(long)j * K + k] * gh;
        }
        gf[(long)n * K + feat_index(k, HW, C)] = acc;
    }
}

// one thread per (j, k): dW1[j][k] = sum_n GH[n][j] F[n][k]; the k = 0 threads: MODE 0: db1[j] = sum_n GH, dW2[j] = sum_n gs lrelu(h),
// db2 = sum_n gs; MODE 1 (F = ggf): dW2[j] = sum_n gs lrelu'(h) V
template <int MODE>
__global__ __launch_bounds__(256) void lin_params_kernel(const float *__restrict__ gs, const float *__restrict__ h, const float *__restrict__ V,
                                                         const float *__restrict__ F, const float *__restrict__ w2, float *__restrict__ dw1,
                                                         float *__restrict__ db1, float *__restrict__ dw2, float *__restrict__ db2, int N, int HW,
                                                         int C, int J, float slope)
{
    const long K = (long)HW * C, total = (long)J * K;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i / K);
        const long k = i - (long)j * K;
        if (dw1) {
            const long fo = feat_index(k, HW, C);
            float acc = 0.f;
            for (int n = 0; n < N; ++n) {
                const float gh = gs[n] * w2[j] * (h[(long)n * J + j] > 0.f ? 1.f : slope);
                acc += gh * F[(long)n * K + fo];
            }
            dw1[i] = acc;
        }
        if (k == 0) {
            float sb = 0.f, sw = 0.f;
            for (int n = 0; n < N; ++n) {
                const float hv = h[(long)n * J + j], m = hv > 0.f ? 1.f : slope;
                sb += gs[n] * w2[j] * m;
                sw += MODE == 0 ? gs[n] * lrelu(hv, slope) : gs[n] * m * V[(long)n * J + j];
            }
            if (MODE == 0 && db1) db1[j] = sb;
            if (dw2) dw2[j] = sw;
            if (MODE == 0 && j == 0 && db2) {
                float s2 = 0.f;
                for (int n = 0; n < N; ++n) s2 += gs[n];
                *db2 = s2;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------- host side
int vout(int n, int ks) { return ks == 4 ? n / 2 : n; }

// splits of k: ~512 blocks in all, at least 8 chunks of 16 per split
void vsplits(long tiles, long KC, int &cps, int &S)
{
    long s = (512 + tiles - 1) / tiles;
    const long smax = KC / 8;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    cps = (int)((KC + s - 1) / s);
    S = (int)((KC + cps - 1) / cps);
}

int check_vconv(const char *what, int N, int H, int W, int Cin, int Cout, int ks)
{
    if (ks != 3 && ks != 4) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: kernel size %d (3: stride 1, 4: stride 2; pad 1)", what, ks);
    if (N <= 0 || H < (ks == 4 ? 2 : 1) || W < (ks == 4 ? 2 : 1))
        return mrefsr::fail(MREFSR_E_INVALID, "%s: N=%d H=%d W=%d", what, N, H, W);
    if (Cin <= 0 || Cin % 4) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: Cin=%d (a multiple of 4)", what, Cin);
    if (Cout <= 0 || Cout % 16) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: Cout=%d (a multiple of 16)", what, Cout);
    return MREFSR_OK;
}

// the GEMM's geometry and grid of MODE (0, 1) for a layer; S and cps from vsplits
VGeo vgeo(int mode, int N, int H, int W, int Cin, int Cout, int ks, dim3 &grid)
{
    VGeo g = {N, H, W, vout(H, ks), vout(W, ks), mode == 1 ? Cout : Cin, mode == 1 ? Cin : Cout, 1, 1};
    long rows, K;
    int phases = 1;
    if (mode == 0) rows = (long)N * g.Ho * g.Wo, K = (long)ks * ks * Cin;
    else if (ks == 4) rows = (long)N * ((H + 1) / 2) * ((W + 1) / 2), K = 4L * Cout, phases = 4;   // (the largest phase sizes the grid)
    else rows = (long)N * H * W, K = 9L * Cout;
    const long mt = (rows + TM - 1) / TM, nt = (g.Nc + TN - 1) / TN;
    vsplits(mt * nt * phases, (K + TK - 1) / TK, g.cps, g.S);
    grid = dim3((unsigned)mt, (unsigned)nt, (unsigned)(g.S * phases));
    return g;
}

VGeo vgeo_wgrad(int N, int H, int W, int Cin, int Cout, int ks, dim3 &grid)
{
    VGeo g = {N, H, W, vout(H, ks), vout(W, ks), Cin, Cout, 1, 1};
    const long R = (long)ks * ks * Cin, Q = (long)N * g.Ho * g.Wo;
    const long mt = (R + TM - 1) / TM, nt = (Cout + TN - 1) / TN;
    vsplits(mt * nt, (Q + TK - 1) / TK, g.cps, g.S);
    grid = dim3((unsigned)mt, (unsigned)nt, (unsigned)g.S);
    return g;
}

template <int MODE>
void launch_gemm(int ks, dim3 grid, hipStream_t st, const float *src, const float *w, const float *bias, float *out, float *ws, const VGeo &g,
                 float slope, int act)
{
    if (ks == 4) hipLaunchKernelGGL((vconv_gemm_kernel<4, MODE>), grid, dim3(256), 0, st, src, w, bias, out, ws, g, slope, act);
    else hipLaunchKernelGGL((vconv_gemm_kernel<3, MODE>), grid, dim3(256), 0, st, src, w, bias, out, ws, g, slope, act);
}

}  // namespace

MREFSR_EXPORT int mrefsr_disc_vconv_pack_weight_f32(const float *w, float *wpk, int Cout, int CinR, int Cin, int ks, int dgrad, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(w && wpk, "disc_vconv_pack_weight: null pointer");
    MREFSR_REQUIRE(Cout > 0 && CinR > 0 && CinR <= Cin && (ks == 3 || ks == 4), "disc_vconv_pack_weight: Cout=%d CinR=%d Cin=%d ks=%d", Cout, CinR,
                   Cin, ks);
    const long total = (long)ks * ks * Cin * Cout;
    hipLaunchKernelGGL(vconv_pack_weight_kernel, dim3(grid_of((total + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)stream, w, wpk, Cout, CinR, Cin,
                       ks * ks, dgrad ? 1 : 0);
    return mrefsr::check_launch("disc_vconv_pack_weight");
}

MREFSR_EXPORT int64_t mrefsr_disc_vconv_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks, int dgrad)
{
    if (check_vconv("disc_vconv_workspace_bytes", N, H, W, Cin, Cout, ks)) return -1;
    dim3 grid;
    const VGeo g = vgeo(dgrad ? 1 : 0, N, H, W, Cin, Cout, ks, grid);
    const long pix = dgrad ? (long)N * H * W : (long)N * g.Ho * g.Wo;
    return g.S > 1 ? (int64_t)g.S * pix * g.Nc * 4 : 0;
}

MREFSR_EXPORT int mrefsr_disc_vconv_f32(const float *x, const float *wpk, const float *bias, float *y, int N, int H, int W, int Cin, int Cout, int ks,
                                        int act, float slope, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && wpk && y, "disc_vconv: null pointer");
    int rc = check_vconv("disc_vconv", N, H, W, Cin, Cout, ks);
    if (rc) return rc;
    dim3 grid;
    const VGeo g = vgeo(0, N, H, W, Cin, Cout, ks, grid);
    const int64_t need = mrefsr_disc_vconv_workspace_bytes(N, H, W, Cin, Cout, ks, 0);
    MREFSR_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "disc_vconv: workspace of %ld bytes < %ld", (long)workspace_bytes, (long)need);
    hipStream_t st = (hipStream_t)stream;
    launch_gemm<0>(ks, grid, st, x, wpk, bias, y, (float *)workspace, g, slope, act ? 1 : 0);
    if (g.S > 1) {
        const long total = (long)N * g.Ho * g.Wo * Cout;
        hipLaunchKernelGGL(vconv_finish_kernel, dim3(grid_of((total + 255) / 256, 8192)), dim3(256), 0, st, (const float *)workspace, bias, y, total,
                           g.S, Cout, slope, act ? 1 : 0);
    }
    return mrefsr::check_launch("disc_vconv");
}

MREFSR_EXPORT int mrefsr_disc_vconv_dgrad_f32(const float *dy, const float *wpk_d, float *dx, int N, int H, int W, int Cin, int Cout, int ks,
                                              void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(dy && wpk_d && dx, "disc_vconv_dgrad: null pointer");
    int rc = check_vconv("disc_vconv_dgrad", N, H, W, Cin, Cout, ks);
    if (rc) return rc;
    dim3 grid;
    const VGeo g = vgeo(1, N, H, W, Cin, Cout, ks, grid);
    const int64_t need = mrefsr_disc_vconv_workspace_bytes(N, H, W, Cin, Cout, ks, 1);
    MREFSR_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "disc_vconv_dgrad: workspace of %ld bytes < %ld", (long)workspace_bytes,
                   (long)need);
    hipStream_t st = (hipStream_t)stream;
    launch_gemm<1>(ks, grid, st, dy, wpk_d, nullptr, dx, (float *)workspace, g, 0.f, 0);
    if (g.S > 1) {
        const long total = (long)N * H * W * Cin;
        hipLaunchKernelGGL(vconv_finish_kernel, dim3(grid_of((total + 255) / 256, 8192)), dim3(256), 0, st, (const float *)workspace, nullptr, dx, total,
                           g.S, Cin, 0.f, 0);
    }
    return mrefsr::check_launch("disc_vconv_dgrad");
}

MREFSR_EXPORT int64_t mrefsr_disc_vconv_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks)
{
    if (check_vconv("disc_vconv_wgrad_workspace_bytes", N, H, W, Cin, Cout, ks)) return -1;
    dim3 grid;
    const VGeo g = vgeo_wgrad(N, H, W, Cin, Cout, ks, grid);
    return (int64_t)g.S * ks * ks * Cin * Cout * 4;
}

MREFSR_EXPORT int mrefsr_disc_vconv_wgrad_f32(const float *x, const float *dy, float *dw, int N, int H, int W, int Cin, int CinR, int Cout, int ks,
                                              void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && dy && dw && workspace, "disc_vconv_wgrad: null pointer");
    int rc = check_vconv("disc_vconv_wgrad", N, H, W, Cin, Cout, ks);
    if (rc) return rc;
    MREFSR_REQUIRE(CinR > 0 && CinR <= Cin, "disc_vconv_wgrad: CinR=%d Cin=%d", CinR, Cin);
    const int64_t need = mrefsr_disc_vconv_wgrad_workspace_bytes(N, H, W, Cin, Cout, ks);
    MREFSR_REQUIRE(workspace_bytes >= need, "disc_vconv_wgrad: workspace of %ld bytes < %ld", (long)workspace_bytes, (long)need);
    dim3 grid;
    const VGeo g = vgeo_wgrad(N, H, W, Cin, Cout, ks, grid);
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    launch_gemm<2>(ks, grid, st, x, dy, nullptr, nullptr, ws, g, 0.f, 0);
    const long total = (long)Cout * CinR * ks * ks;
    hipLaunchKernelGGL(vconv_wgrad_finish_kernel, dim3(grid_of((total + 255) / 256, 4096)), dim3(256), 0, st, ws, dw, g.S, Cin, CinR, Cout, ks * ks);
    return mrefsr::check_launch("disc_vconv_wgrad");
}

MREFSR_EXPORT int mrefsr_disc_lrelu_mask_f32(const float *g, const float *y, float *out, int64_t n, float slope, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(g && y && out, "disc_lrelu_mask: null pointer");
    MREFSR_REQUIRE(n > 0, "disc_lrelu_mask: n=%ld", (long)n);
    hipLaunchKernelGGL(lrelu_mask_kernel, dim3(grid_of((n + 255) / 256, 16384)), dim3(256), 0, (hipStream_t)stream, g, y, out, (long)n, slope);
    return mrefsr::check_launch("disc_lrelu_mask");
}

static int check_lin(const char *what, int N, int HW, int C, int J)
{
    if (N <= 0 || HW <= 0 || C <= 0 || J <= 0) return mrefsr::fail(MREFSR_E_INVALID, "%s: N=%d HW=%d C=%d J=%d", what, N, HW, C, J);
    return MREFSR_OK;
}

MREFSR_EXPORT int64_t mrefsr_disc_linear_head_workspace_bytes(int N, int J)
{
    if (N <= 0 || J <= 0) return -1;
    return (int64_t)N * J * 4;   // V [N][J]
}

MREFSR_EXPORT int mrefsr_disc_linear_head_fwd_f32(const float *f, const float *w1, const float *b1, const float *w2, const float *b2, float *out,
                                                  float *hidden, int N, int HW, int C, int J, float slope, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(f && w1 && b1 && w2 && b2 && out && hidden, "disc_linear_head_fwd: null pointer");
    int rc = check_lin("disc_linear_head_fwd", N, HW, C, J);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lin_rows_kernel, dim3(J), dim3(256), 0, st, f, w1, b1, hidden, N, HW, C, J);
    hipLaunchKernelGGL(lin_out_kernel<0>, dim3((N + 63) / 64), dim3(64), 0, st, hidden, nullptr, w2, b2, out, N, J, slope);
    return mrefsr::check_launch("disc_linear_head_fwd");
}

MREFSR_EXPORT int mrefsr_disc_linear_head_bwd_f32(const float *gs, const float *hidden, const float *f, const float *w1, const float *w2, float *gf,
                                                  float *gw1, float *gb1, float *gw2, float *gb2, int N, int HW, int C, int J, float slope,
                                                  mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(gs && hidden && w1 && w2, "disc_linear_head_bwd: null pointer");
    MREFSR_REQUIRE(f || !gw1, "disc_linear_head_bwd: gw1 needs f");
    int rc = check_lin("disc_linear_head_bwd", N, HW, C, J);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long K = (long)HW * C;
    if (gf) hipLaunchKernelGGL(lin_gf_kernel, dim3(grid_of((N * K + 255) / 256, 8192)), dim3(256), 0, st, gs, hidden, w1, w2, gf, N, HW, C, J, slope);
    if (gw1 || gb1 || gw2 || gb2)
        hipLaunchKernelGGL(lin_params_kernel<0>, dim3(grid_of((J * K + 255) / 256, 8192)), dim3(256), 0, st, gs, hidden, nullptr, f, w2, gw1, gb1, gw2,
                           gb2, N, HW, C, J, slope);
    return mrefsr::check_launch("disc_linear_head_bwd");
}

MREFSR_EXPORT int mrefsr_disc_linear_head_dbl_f32(const float *ggf, const float *gs, const float *hidden, const float *w1, const float *w2, float *d_gs,
                                                  float *d_w1, float *d_w2, int N, int HW, int C, int J, float slope, void *workspace,
                                                  int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(ggf && gs && hidden && w1 && w2 && workspace, "disc_linear_head_dbl: null pointer");
    int rc = check_lin("disc_linear_head_dbl", N, HW, C, J);
    if (rc) return rc;
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_disc_linear_head_workspace_bytes(N, J), "disc_linear_head_dbl: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float *V = (float *)workspace;
    const long K = (long)HW * C;
    if (d_gs || d_w2) hipLaunchKernelGGL(lin_rows_kernel, dim3(J), dim3(256), 0, st, ggf, w1, nullptr, V, N, HW, C, J);
    if (d_gs) hipLaunchKernelGGL(lin_out_kernel<1>, dim3((N + 63) / 64), dim3(64), 0, st, hidden, V, w2, nullptr, d_gs, N, J, slope);
    if (d_w1 || d_w2)
        hipLaunchKernelGGL(lin_params_kernel<1>, dim3(grid_of((J * K + 255) / 256, 8192)), dim3(256), 0, st, gs, hidden, V, ggf, w2, d_w1, nullptr,
                           d_w2, nullptr, N, HW, C, J, slope);
    return mrefsr::check_launch("disc_linear_head_dbl");
}
