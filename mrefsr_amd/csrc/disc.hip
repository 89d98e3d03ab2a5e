// ImageDiscriminator of the adversarial training step (basicsr/archs/discriminator_arch.py:10-45, trained by
// MultiRefRestorationModel.optimize_parameters, multi_ref_restoration_model.py:219-278, and differentiated twice by
// gradient_penalty_loss, basicsr/models/losses.py:370-404): the kernels of mrefsr_amd/archs/nhwc_disc.py.
//   pack_image / unpack_image   [B][3][H][W] <-> [B][H][W][4] (channel 3 = 0) and its gradient
//   conv_pack_weight            [Cout][Cin][3][3] -> the GEMM layouts of the forward ([9][Cin][Cout]) and input gradient ([9][Cout][Cin])
//   conv_gemm                   3x3 / pad 1 / stride 1 or 2 as an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32 products):
//                               forward (rows = output pixels) and input gradient (rows = input pixels, one launch per output
//                               parity phase of a stride-2 layer: a gather over its 1-2 taps per dimension, no scatter)
//   conv_wgrad / _finish        weight gradient: split over the pixels into partial tiles, added in a fixed order
//   chan_stats / chan_sums      per-channel (count, mean, M2) and sums of the BatchNorm passes: fixed-order partials in double
//   bn_*                        BatchNorm2d (training mode) + LeakyReLU: forward, backward, double backward
//   head_*                      AdaptiveAvgPool2d(1) -> 1x1 conv + bias -> LeakyReLU -> 1x1 conv + bias -> Sigmoid: forward,
//                               backward, double backward (a few MFLOP: one block per image, then one thread per weight)
// No float atomics anywhere: two runs give the same bits.
#include "disc_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// image packing: img [B][3][H][W] -> x4 [B][H][W][4] (channel 3 = 0); the gradient takes channels 0..2 back
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_image_kernel(const float *__restrict__ img, float4 *__restrict__ x4, long HW, long total)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / HW, p = i - b * HW;
        const float *s = img + b * 3 * HW + p;
        x4[i] = make_float4(s[0], s[HW], s[2 * HW], 0.f);
    }
}

__global__ __launch_bounds__(256) void unpack_image_kernel(const float4 *__restrict__ g4, float *__restrict__ img, long HW, long total)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / HW, p = i - b * HW;
        const float4 v = g4[i];
        float *d = img + b * 3 * HW + p;
        d[0] = v.x, d[HW] = v.y, d[2 * HW] = v.z;
    }
}

// w [Cout][CinR][3][3] -> dgrad = 0: [9][Cin][Cout], 1: [9][Cout][Cin]; channels CinR..Cin-1 (the image's padding channel) are 0
__global__ __launch_bounds__(256) void conv_pack_weight_kernel(const float *__restrict__ w, float *__restrict__ out, int Cout, int CinR, int Cin,
                                                               int dgrad)
{
    const long total = 9L * Cin * Cout;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int ci, co;
        const int t = (int)(i / ((long)Cin * Cout));
        const int r = (int)(i - (long)t * Cin * Cout);
        if (dgrad) co = r / Cin, ci = r - co * Cin;
        else ci = r / Cout, co = r - ci * Cout;
        out[i] = ci < CinR ? w[((long)co * CinR + ci) * 9 + t] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 3x3 convolution, pad 1, as an implicit GEMM  out[row][col] = sum_{tap, k} src[pixel(row, tap)][k] * wpk[tap][k][col].
//   MODE 0 (forward):        row = output pixel (n, oy, ox) of [N][Ho][Wo]; src = x [N][H][W][Kc = Cin]; source pixel
//                            (oy s + ky - 1, ox s + kx - 1); + bias; out [N][Ho][Wo][Nc = Cout].
//   MODE 1 (input gradient): row = input pixel (n, iy, ix) of the phase (py, px) = blockIdx.z (stride 2: iy = 2 i + py); src = dy
//                            [N][Ho][Wo][Kc = Cout]; a tap contributes when (iy + 1 - ky) is a multiple of s: source pixel
//                            ((iy + 1 - ky) / s, (ix + 1 - kx) / s).  For a stride-2 phase that is 1 (py = 0: ky = 1) or 2 (py = 1:
//                            ky = 0, 2) taps per dimension; out = dx [N][H][W][Nc = Cin].
// Wave = 32 rows x 16 NB columns: 2 x NB accumulators of v_mfma_f32_16x16x4_f32 (A: lane l = row l & 15, k l >> 4; B: k l >> 4,
// column l & 15; D: row 4 (l >> 4) + r, column l & 15).  VEC (Kc % 16 == 0): a lane reads a float4 of 4 consecutive channels and
// feeds element e to the e-th MFMA of a 16-channel step; otherwise (Kc % 4 == 0) one channel per MFMA.  The sum over k of one
// output element is done by one wave in a fixed order.  Block = 4 waves = 128 consecutive rows.
// ---------------------------------------------------------------------------------------------------------------
struct ConvGeo {
    int N, H, W, Ho, Wo, s;   // input H x W, output Ho x Wo, stride
    int Kc, Nc;               // GEMM k channels per tap, columns
};

template <int MODE, int NB, bool VEC>
__global__ __launch_bounds__(256) void conv_gemm_kernel(const float *__restrict__ src, const float *__restrict__ wpk, const float *__restrict__ bias,
                                                        float *__restrict__ out, const ConvGeo g)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane >> 4, cl = lane & 15;
    const int py = MODE == 1 && g.s == 2 ? (int)(blockIdx.z >> 1) : 0, px = MODE == 1 && g.s == 2 ? (int)(blockIdx.z & 1) : 0;
    // the rows' grid: output pixels (MODE 0) or the input pixels of this phase (MODE 1)
    const int Hr = MODE == 0 ? g.Ho : (g.s == 2 ? (g.H - py + 1) >> 1 : g.H);
    const int Wr = MODE == 0 ? g.Wo : (g.s == 2 ? (g.W - px + 1) >> 1 : g.W);
    const long M = (long)g.N * Hr * Wr;
    const long m0 = ((long)blockIdx.x * 4 + wave) * 32;
    if (m0 >= M || Hr <= 0 || Wr <= 0) return;
    const int n0 = blockIdx.y * 16 * NB;
    const int Hs = MODE == 0 ? g.H : g.Ho, Ws = MODE == 0 ? g.W : g.Wo;   // source map
    // the two rows this lane feeds into the A operand
    int rn[2], ry[2], rx[2];
    bool rok[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const long m = m0 + 16 * a + cl;
        rok[a] = m < M;
        const long mm = rok[a] ? m : 0;
        const int xx = (int)(mm % Wr);
        const long q = mm / Wr;
        const int yy = (int)(q % Hr);
        rn[a] = (int)(q / Hr);
        if (MODE == 0) ry[a] = yy, rx[a] = xx;
        else ry[a] = g.s == 2 ? 2 * yy + py : yy, rx[a] = g.s == 2 ? 2 * xx + px : xx;   // the input pixel
    }
    f32x4 acc[2][NB];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int Kc = g.Kc, Nc = g.Nc;
    bool cok[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) cok[b] = n0 + 16 * b + cl < Nc;
    for (int ky = 0; ky < 3; ++ky) {
        if (MODE == 1 && g.s == 2 && ((py + 1 - ky) & 1)) continue;   // (block-uniform: this phase has no such tap)
        for (int kx = 0; kx < 3; ++kx) {
            if (MODE == 1 && g.s == 2 && ((px + 1 - kx) & 1)) continue;
            long soff[2];
            bool sok[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                int sy, sx;
                if (MODE == 0) sy = ry[a] * g.s + ky - 1, sx = rx[a] * g.s + kx - 1;
                else if (g.s == 2) sy = (ry[a] + 1 - ky) >> 1, sx = (rx[a] + 1 - kx) >> 1;   // (even numerators: exact halves)
                else sy = ry[a] + 1 - ky, sx = rx[a] + 1 - kx;
                sok[a] = rok[a] && sy >= 0 && sy < Hs && sx >= 0 && sx < Ws;
                soff[a] = sok[a] ? (((long)rn[a] * Hs + sy) * Ws + sx) * Kc : 0;
            }
            const float *wt = wpk + (long)(ky * 3 + kx) * Kc * Nc;
            if (VEC) {
                for (int c0 = 0; c0 < Kc; c0 += 16) {
                    const int kc = c0 + 4 * kl;
                    float ae[2][4];
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        const float4 v = sok[a] ? *reinterpret_cast<const float4 *>(src + soff[a] + kc) : make_float4(0.f, 0.f, 0.f, 0.f);
                        ae[a][0] = v.x, ae[a][1] = v.y, ae[a][2] = v.z, ae[a][3] = v.w;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float bv[NB];
#pragma unroll
                        for (int b = 0; b < NB; ++b) bv[b] = cok[b] ? wt[(long)(kc + e) * Nc + n0 + 16 * b + cl] : 0.f;
#pragma unroll
                        for (int a = 0; a < 2; ++a)
#pragma unroll
                            for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(ae[a][e], bv[b], acc[a][b], 0, 0, 0);
                    }
                }
            } else {
                for (int c0 = 0; c0 < Kc; c0 += 4) {
                    const int kc = c0 + kl;
                    float av[2], bv[NB];
#pragma unroll
                    for (int a = 0; a < 2; ++a) av[a] = sok[a] ? src[soff[a] + kc] : 0.f;
#pragma unroll
                    for (int b = 0; b < NB; ++b) bv[b] = cok[b] ? wt[(long)kc * Nc + n0 + 16 * b + cl] : 0.f;
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
                }
            }
        }
    }
    // store: row m0 + 16 a + 4 kl + r, column n0 + 16 b + cl
    const int Ho_ = MODE == 0 ? g.Ho : g.H, Wo_ = MODE == 0 ? g.Wo : g.W;   // the output map
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long m = m0 + 16 * a + 4 * kl + r;
            if (m >= M) continue;
            const int xx = (int)(m % Wr);
            const long q = m / Wr;
            const int yy = (int)(q % Hr);
            const int nn = (int)(q / Hr);
            const int oy = MODE == 1 && g.s == 2 ? 2 * yy + py : yy, ox = MODE == 1 && g.s == 2 ? 2 * xx + px : xx;
            float *dst = out + (((long)nn * Ho_ + oy) * Wo_ + ox) * Nc;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int col = n0 + 16 * b + cl;
                if (col < Nc) dst[col] = MODE == 0 && bias ? acc[a][b][r] + bias[col] : acc[a][b][r];
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------
// Weight gradient  dW[tap][ci][co] = sum_q x[pixel(q, tap)][ci] * dy[q][co]  over the output pixels q, as a GEMM with rows
// (tap, ci) = tap * Cin + ci, columns co, k = q.  One wave = 32 rows x 16 NB columns over the pixel range of split blockIdx.z,
// k-ordered; its partial tile goes to ws[split][row][co].  conv_wgrad_finish adds the splits in order and writes torch's
// layout [Cout][CinR][3][3].
// ---------------------------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(64) void conv_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ ws,
                                                        const ConvGeo g, int chunk)
{
    const int lane = threadIdx.x, kl = lane >> 4, cl = lane & 15;
    const int Cin = g.Kc, Cout = g.Nc, R = 9 * Cin;
    const int r0 = blockIdx.x * 32, n0 = blockIdx.y * 16 * NB, split = blockIdx.z;
    const long Q = (long)g.N * g.Ho * g.Wo;
    const long qb = (long)split * chunk, qe = min(Q, qb + chunk);
    int rky[2], rkx[2], rci[2];
    bool rok[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int r = r0 + 16 * a + cl;
        rok[a] = r < R;
        const int t = rok[a] ? r / Cin : 0;
        rky[a] = t / 3, rkx[a] = t - 3 * (t / 3), rci[a] = rok[a] ? r - t * Cin : 0;
    }
    bool cok[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) cok[b] = n0 + 16 * b + cl < Cout;
    f32x4 acc[2][NB];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long k = qb; k < qe; k += 4) {
        const long q = k + kl;
        const bool qok = q < qe;
        const long qq = qok ? q : qb;
        const int ox = (int)(qq % g.Wo);
        const long t2 = qq / g.Wo;
        const int oy = (int)(t2 % g.Ho);
        const long n = t2 / g.Ho;
        float av[2], bv[NB];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int iy = oy * g.s + rky[a] - 1, ix = ox * g.s + rkx[a] - 1;
            const bool ok = qok && rok[a] && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
            av[a] = ok ? x[((n * g.H + iy) * g.W + ix) * Cin + rci[a]] : 0.f;
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) bv[b] = qok && cok[b] ? dy[qq * Cout + n0 + 16 * b + cl] : 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
    float *o = ws + (long)split * R * Cout;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + 16 * a + 4 * kl + r;
            if (row >= R) continue;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int col = n0 + 16 * b + cl;
                if (col < Cout) o[(long)row * Cout + col] = acc[a][b][r];
            }
        }
}

__global__ __launch_bounds__(256) void conv_wgrad_finish_kernel(const float *__restrict__ ws, float *__restrict__ dw, int S, int Cin, int CinR,
                                                                int Cout)
{
    const long total = (long)Cout * CinR * 9;
    const long R = 9L * Cin;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int t = (int)(i % 9);
        const long r = i / 9;
        const int ci = (int)(r % CinR);
        const int co = (int)(r / CinR);
        const long src = ((long)t * Cin + ci) * Cout + co;
        float acc = 0.f;
        for (int s = 0; s < S; ++s) acc += ws[(long)s * R * Cout + src];
        dw[i] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Per-channel reductions over [P][C] (P = N H W pixels).  Block (split s, 64 channels): 4 rows of 64 threads, thread (rl, c)
// takes pixels p = pb + rl + 4 j of the split's range; the 4 rows are merged in order, partial[s][q][c].
//   chan_stats: Welford (count, mean, M2) of x, merged with Chan's formula (double).
//   chan_sums:  sums (double) of up to 5 quantities of g = gy * lrelu'(y) (mask from the output sign) or of gy itself:
//               MODE 0: gy (bias gradient); 1: g, g xh; 2: g, g xh, a, a xh, a g  (xh = (x - mean) invstd, a = ggx)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void chan_stats_kernel(const float *__restrict__ x, double *__restrict__ part, long P, int C, int chunk)
{
    __shared__ double sh[3][4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cl, s = blockIdx.x;
    const long pb = (long)s * chunk, pe = min(P, pb + chunk);
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
    if (c < C)
        for (long p = pb + rl; p < pe; p += 4) {
            const double v = x[p * C + c];
            cnt += 1.0;
            const double d = v - mean;
            mean += d / cnt;
            m2 += d * (v - mean);
        }
    sh[0][rl][cl] = cnt, sh[1][rl][cl] = mean, sh[2][rl][cl] = m2;
    __syncthreads();
    if (rl == 0 && c < C) {
        for (int k = 1; k < 4; ++k) {
            const double nb = sh[0][k][cl];
            if (nb == 0.0) continue;
            const double mb = sh[1][k][cl], tot = cnt + nb, d = mb - mean;
            mean += d * (nb / tot);
            m2 += sh[2][k][cl] + d * d * (cnt * nb / tot);
            cnt = tot;
        }
        const long gs = gridDim.x;
        part[(0 * gs + s) * (long)C + c] = cnt;   // layout [q][split][C]
        part[(1 * gs + s) * (long)C + c] = mean;
        part[(2 * gs + s) * (long)C + c] = m2;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void chan_sums_kernel(const float *__restrict__ gy, const float *__restrict__ y, const float *__restrict__ x,
                                                        const float *__restrict__ a, const float *__restrict__ mean, const float *__restrict__ invstd,
                                                        double *__restrict__ part, long P, int C, int chunk, float slope)
{
    constexpr int NQ = MODE == 0 ? 1 : (MODE == 1 ? 2 : 5);
    __shared__ double sh[NQ][4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cl, s = blockIdx.x;
    const long pb = (long)s * chunk, pe = min(P, pb + chunk);
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    if (c < C) {
        const float mu = MODE ? mean[c] : 0.f, r = MODE ? invstd[c] : 0.f;
        for (long p = pb + rl; p < pe; p += 4) {
            const long i = p * C + c;
            float g = gy[i];
            if (MODE == 0) {
                acc[0] += g;
                continue;
            }
            if (!(y[i] > 0.f)) g *= slope;
            const float xh = (x[i] - mu) * r;
            acc[0] += g;
            acc[1] += (double)g * xh;
            if (MODE == 2) {
                const float av = a[i];
                acc[2] += av;
                acc[3] += (double)av * xh;
                acc[4] += (double)av * g;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) sh[q][rl][cl] = acc[q];
    __syncthreads();
    if (rl == 0 && c < C) {
        const long gs = gridDim.x;
#pragma unroll
        for (int q = 0; q < NQ; ++q) part[((long)q * gs + s) * C + c] = ((sh[q][0][cl] + sh[q][1][cl]) + sh[q][2][cl]) + sh[q][3][cl];
    }
}

// merge of the BatchNorm statistics: mean, invstd = 1 / sqrt(var + eps) (biased var), and torch's running-statistics update
// (running = (1 - momentum) running + momentum stat, var unbiased by n / (n - 1)); num_batches_tracked += 1
__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const double *__restrict__ part, int S, int C, float eps, float momentum,
                                                              float *__restrict__ mean_out, float *__restrict__ invstd_out,
                                                              float *__restrict__ run_mean, float *__restrict__ run_var, int64_t *__restrict__ nbt)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && nbt) *nbt += 1;
    if (c >= C) return;
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
    for (int s = 0; s < S; ++s) {
        const double nb = part[(0L * S + s) * C + c];
        if (nb == 0.0) continue;
        const double mb = part[(1L * S + s) * C + c], tot = cnt + nb, d = mb - mean;
        mean += d * (nb / tot);
        m2 += part[(2L * S + s) * C + c] + d * d * (cnt * nb / tot);
        cnt = tot;
    }
    const double var = m2 / cnt;
    mean_out[c] = (float)mean;
    invstd_out[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (run_mean) run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mean;
    if (run_var) run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)(m2 / (cnt - 1.0));
}

// sums[q][c] = sum over the splits, in order; MODE 0: db = sums[0]; MODE 1: dgamma = sum g xh, dbeta = sum g;
// MODE 2: d gamma = invstd (A - Q P) with A = sum a g - (sum g / n) sum a, P = sum a xh, Q = sum g xh / n
template <int MODE>
__global__ __launch_bounds__(256) void chan_sums_finish_kernel(const double *__restrict__ part, int S, int C, long P, double *__restrict__ sums,
                                                               const float *__restrict__ invstd, float *__restrict__ o0, float *__restrict__ o1)
{
    constexpr int NQ = MODE == 0 ? 1 : (MODE == 1 ? 2 : 5);
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double acc = 0.0;
        for (int s = 0; s < S; ++s) acc += part[((long)q * S + s) * C + c];
        v[q] = acc;
        sums[(long)q * C + c] = acc;
    }
    if (MODE == 0 && o0) o0[c] = (float)v[0];
    if (MODE == 1) {
        if (o0) o0[c] = (float)v[1];
        if (o1) o1[c] = (float)v[0];
    }
    if (MODE == 2 && o0) {
        const double n = (double)P, A = v[4] - v[0] / n * v[2], Pp = v[3], Q = v[1] / n;
        o0[c] = (float)((double)invstd[c] * (A - Q * Pp));
    }
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float *__restrict__ x, const float *__restrict__ mean, const float *__restrict__ invstd,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ y,
                                                       long total, int C, float slope)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        y[i] = lrelu((x[i] - mean[c]) * invstd[c] * gamma[c] + beta[c], slope);
    }
}

// gx = gamma invstd (g - sum g / n - xh sum g xh / n),  g = gy lrelu'(y)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float *__restrict__ gy, const float *__restrict__ y, const float *__restrict__ x,
                                                           const float *__restrict__ mean, const float *__restrict__ invstd,
                                                           const float *__restrict__ gamma, const double *__restrict__ sums, float *__restrict__ gx,
                                                           long total, int C, double inv_n, float slope)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        float g = gy[i];
        if (!(y[i] > 0.f)) g *= slope;
        const float r = invstd[c], xh = (x[i] - mean[c]) * r;
        const float gm = (float)(sums[c] * inv_n), gxm = (float)(sums[C + c] * inv_n);
        gx[i] = gamma[c] * r * (g - gm - xh * gxm);
    }
}

// double backward (a = ggx, b = ggamma, c = gbeta per channel; n pixels per channel; P, Q, A as in chan_sums_finish):
//   d gy = lrelu'(y) (gamma r (a - sum a / n - xh P / n) + b xh + c)
//   d x  = -gamma r^2 xh (A - Q P) / n - gamma r^2 (Q (a - sum a / n - xh P / n) + (P / n) (g - sum g / n - xh Q)) + b r (g - sum g / n - xh Q)
__global__ __launch_bounds__(256) void bn_dbl_apply_kernel(const float *__restrict__ a, const float *__restrict__ ggamma, const float *__restrict__ gbeta,
                                                           const float *__restrict__ gy, const float *__restrict__ y, const float *__restrict__ x,
                                                           const float *__restrict__ mean, const float *__restrict__ invstd,
                                                           const float *__restrict__ gamma, const double *__restrict__ sums, float *__restrict__ d_gy,
                                                           float *__restrict__ d_x, long total, int C, double n, float slope)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const float m = y[i] > 0.f ? 1.f : slope;
        const float g = gy[i] * m;
        const float r = invstd[c], xh = (x[i] - mean[c]) * r, gm = gamma[c];
        const double Sg = sums[c], Sgx = sums[C + c], Sa = sums[2 * C + c], Sax = sums[3 * C + c], Sag = sums[4 * C + c];
        const float am = (float)(Sa / n), Pn = (float)(Sax / n), Q = (float)(Sgx / n), gmean = (float)(Sg / n);
        const float AQP = (float)((Sag - Sg / n * Sa - Sgx / n * Sax) / n);   // (A - Q P) / n
        const float b = ggamma ? ggamma[c] : 0.f, cc = gbeta ? gbeta[c] : 0.f;
        const float av = a[i];
        const float a_c = av - am - xh * Pn, g_c = g - gmean - xh * Q;
        if (d_gy) d_gy[i] = m * (gm * r * a_c + b * xh + cc);
        if (d_x) d_x[i] = -gm * r * r * (xh * AQP + Q * a_c + Pn * g_c) + b * r * g_c;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Head.  f [N][HW][C]; W1 [J][C] (+ b1), W2 [J] (+ b2).  Saved: pooled P [N][C], pre-activation H [N][J], output s [N].
// Forward (block per image): P = sum_q f / HW (q in order), H = b1 + W1 P (c in order), o = b2 + sum_j W2 lrelu(H) (per-thread j
// order, then a fixed tree), s = sigmoid(o).
// ---------------------------------------------------------------------------------------------------------------
#define HEAD_MAXC 2048
#define HEAD_MAXJ 4096

__global__ __launch_bounds__(256) void head_fwd_kernel(const float *__restrict__ f, const float *__restrict__ w1, const float *__restrict__ b1,
                                                       const float *__restrict__ w2, const float *__restrict__ b2, float *__restrict__ out,
                                                       float *__restrict__ Pp, float *__restrict__ Hh, int HW, int C, int J, float slope)
{
    __shared__ float sp[HEAD_MAXC];
    __shared__ float red[256];
    const int n = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = 0.f;
        for (int q = 0; q < HW; ++q) acc += f[((long)n * HW + q) * C + c];
        acc = acc / (float)HW;
        sp[c] = acc;
        Pp[(long)n * C + c] = acc;
    }
    __syncthreads();
    float part = 0.f;
    for (int j = threadIdx.x; j < J; j += 256) {
        const float *wr = w1 + (long)j * C;
        float h = 0.f;
        for (int c = 0; c < C; ++c) h += wr[c] * sp[c];
        h += b1[j];
        Hh[(long)n * J + j] = h;
        part += w2[j] * lrelu(h, slope);
    }
    const float o = mrefsr::block_sum<256>(red, part) + b2[0];
    if (threadIdx.x == 0) out[n] = 1.f / (1.f + expf(-o));
}

// backward, per image: go = gs s (1 - s), GH[n][j] = go W2[j] lrelu'(H), gf[n][q][c] = (sum_j W1[j][c] GH[n][j]) / HW
__global__ __launch_bounds__(256) void head_bwd_kernel(const float *__restrict__ gs, const float *__restrict__ s, const float *__restrict__ Hh,
                                                       const float *__restrict__ w1, const float *__restrict__ w2, float *__restrict__ gf,
                                                       float *__restrict__ GH, float *__restrict__ GO, int HW, int C, int J, float slope)
{
    __shared__ float sh[HEAD_MAXJ];
    const int n = blockIdx.x;
    const float sv = s[n], go = gs[n] * (sv * (1.f - sv));
    if (threadIdx.x == 0) GO[n] = go;
    for (int j = threadIdx.x; j < J; j += 256) {
        const float gh = go * w2[j] * (Hh[(long)n * J + j] > 0.f ? 1.f : slope);
        sh[j] = gh;
        GH[(long)n * J + j] = gh;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = 0.f;
        for (int j = 0; j < J; ++j) acc += w1[(long)j * C + c] * sh[j];
        acc = acc / (float)HW;
        for (int q = 0; q < HW; ++q) gf[((long)n * HW + q) * C + c] = acc;
    }
}

// double backward, per image (ggf = d L / d gf; u = sum_j W2 lrelu'(H) V with V = W1 ggp, ggp = sum_q ggf / HW):
//   d gs = s (1 - s) u;  e = gs s (1 - s) (1 - 2 s) u  (= d L / d o);  DH = e W2 lrelu'(H);  d f = (W1^T DH) / HW;
//   GH = go W2 lrelu'(H) (the backward's, for the W1 term GH x ggp)
__global__ __launch_bounds__(256) void head_dbl_kernel(const float *__restrict__ ggf, const float *__restrict__ gs, const float *__restrict__ s,
                                                       const float *__restrict__ Hh, const float *__restrict__ w1, const float *__restrict__ w2,
                                                       float *__restrict__ d_gs, float *__restrict__ d_f, float *__restrict__ DH,
                                                       float *__restrict__ GH, float *__restrict__ V, float *__restrict__ GGP,
                                                       float *__restrict__ E, float *__restrict__ GO, int HW, int C, int J, float slope)
{
    __shared__ float sp[HEAD_MAXC];
    __shared__ float sh[HEAD_MAXJ];
    __shared__ float red[256];
    const int n = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = 0.f;
        for (int q = 0; q < HW; ++q) acc += ggf[((long)n * HW + q) * C + c];
        acc = acc / (float)HW;
        sp[c] = acc;
        GGP[(long)n * C + c] = acc;
    }
    __syncthreads();
    float part = 0.f;
    for (int j = threadIdx.x; j < J; j += 256) {
        const float *wr = w1 + (long)j * C;
        float v = 0.f;
        for (int c = 0; c < C; ++c) v += wr[c] * sp[c];
        V[(long)n * J + j] = v;
        part += w2[j] * (Hh[(long)n * J + j] > 0.f ? 1.f : slope) * v;
    }
    const float u = mrefsr::block_sum<256>(red, part);
    const float sv = s[n], ds = sv * (1.f - sv), go = gs[n] * ds, e = go * (1.f - 2.f * sv) * u;
    if (threadIdx.x == 0) {
        if (d_gs) d_gs[n] = ds * u;
        E[n] = e;
        GO[n] = go;
    }
    for (int j = threadIdx.x; j < J; j += 256) {
        const float mw = w2[j] * (Hh[(long)n * J + j] > 0.f ? 1.f : slope);
        sh[j] = e * mw;
        DH[(long)n * J + j] = e * mw;
        GH[(long)n * J + j] = go * mw;
    }
    __syncthreads();
    if (d_f)
        for (int c = threadIdx.x; c < C; c += 256) {
            float acc = 0.f;
            for (int j = 0; j < J; ++j) acc += w1[(long)j * C + c] * sh[j];
            acc = acc / (float)HW;
            for (int q = 0; q < HW; ++q) d_f[((long)n * HW + q) * C + c] = acc;
        }
}

// parameter gradients of the head, one thread per W1 element (n in order):
//   dW1[j][c] = sum_n X[n][j] Pp[n][c] (+ X2[n][j] P2[n][c]);  db1[j] = sum_n X[n][j]
//   dW2[j] = sum_n y1[n] lrelu(H[n][j]) (+ y2[n] lrelu'(H[n][j]) V[n][j]);  db2 = sum_n y1[n]
__global__ __launch_bounds__(256) void head_params_kernel(const float *__restrict__ X, const float *__restrict__ Pp, const float *__restrict__ X2,
                                                          const float *__restrict__ P2, const float *__restrict__ y1, const float *__restrict__ y2,
                                                          const float *__restrict__ Hh, const float *__restrict__ V, float *__restrict__ dw1,
                                                          float *__restrict__ db1, float *__restrict__ dw2, float *__restrict__ db2, int N, int C,
                                                          int J, float slope)
{
    const long total = (long)J * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i / C), c = (int)(i - (long)j * C);
        if (dw1) {
            float acc = 0.f;
            for (int n = 0; n < N; ++n) {
                acc += X[(long)n * J + j] * Pp[(long)n * C + c];
                if (X2) acc += X2[(long)n * J + j] * P2[(long)n * C + c];
            }
            dw1[i] = acc;
        }
        if (c == 0) {
            float sb = 0.f, sw = 0.f;
            for (int n = 0; n < N; ++n) {
                const float h = Hh[(long)n * J + j];
                sb += X[(long)n * J + j];
                sw += y1[n] * lrelu(h, slope);
                if (y2) sw += y2[n] * (h > 0.f ? 1.f : slope) * V[(long)n * J + j];
            }
            if (db1) db1[j] = sb;
            if (dw2) dw2[j] = sw;
            if (j == 0 && db2) {
                float s2 = 0.f;
                for (int n = 0; n < N; ++n) s2 += y1[n];
                *db2 = s2;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------- host side
int conv_splits_of(long rows, int per)
{
    // splits of the per-channel reductions: >= 256 pixels each, ~256 blocks in all
    long s = (rows + 255) / 256;
    if (s > per) s = per;
    return (int)(s < 1 ? 1 : s);
}

int chan_splits(long P, int C)
{
    const int cb = (C + 63) / 64;
    return conv_splits_of(P, (256 + cb - 1) / cb);
}

int wgrad_splits(int N, int Ho, int Wo, int Cin, int Cout)
{
    const long Q = (long)N * Ho * Wo;
    const int NB = Cout % 32 == 0 ? 2 : 1;
    const long tiles = (long)((9 * Cin + 31) / 32) * ((Cout + 16 * NB - 1) / (16 * NB));
    long s = (1024 + tiles - 1) / tiles;   // ~1024 waves in flight
    const long smax = (Q + 255) / 256;      // >= 256 pixels per split
    if (s > smax) s = smax;
    return (int)(s < 1 ? 1 : s);
}

int out_size(int n, int s) { return s == 2 ? (n + 1) / 2 : n; }

int check_conv(const char *what, int N, int H, int W, int Cin, int Cout, int stride)
{
    if (N <= 0 || H <= 0 || W <= 0)
        return mrefsr::fail(MREFSR_E_INVALID, "%s: N=%d H=%d W=%d", what, N, H, W);
    if (stride != 1 && stride != 2) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: stride %d (1 or 2)", what, stride);
    if (Cin <= 0 || Cin % 4 || !(Cin == 4 || Cin % 16 == 0))
        return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: Cin=%d (4, the packed image, or a multiple of 16)", what, Cin);
    if (Cout <= 0 || Cout % 16) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: Cout=%d (a multiple of 16)", what, Cout);
    return MREFSR_OK;
}

}  // namespace

MREFSR_EXPORT int mrefsr_disc_pack_image_f32(const float *img, float *x4, int B, int H, int W, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(img && x4, "disc_pack_image: null pointer");
    MREFSR_REQUIRE(B > 0 && H > 0 && W > 0, "disc_pack_image: B=%d H=%d W=%d", B, H, W);
    const long HW = (long)H * W, total = B * HW;
    hipLaunchKernelGGL(pack_image_kernel, dim3(grid_of((total + 255) / 256, 16384)), dim3(256), 0, (hipStream_t)stream, img,
                       reinterpret_cast<float4 *>(x4), HW, total);
    return mrefsr::check_launch("disc_pack_image");
}

MREFSR_EXPORT int mrefsr_disc_unpack_image_f32(const float *g4, float *img, int B, int H, int W, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(img && g4, "disc_unpack_image: null pointer");
    MREFSR_REQUIRE(B > 0 && H > 0 && W > 0, "disc_unpack_image: B=%d H=%d W=%d", B, H, W);
    const long HW = (long)H * W, total = B * HW;
    hipLaunchKernelGGL(unpack_image_kernel, dim3(grid_of((total + 255) / 256, 16384)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(g4), img, HW, total);
    return mrefsr::check_launch("disc_unpack_image");
}

MREFSR_EXPORT int mrefsr_disc_conv_pack_weight_f32(const float *w, float *wpk, int Cout, int CinR, int Cin, int dgrad, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(w && wpk, "disc_conv_pack_weight: null pointer");
    MREFSR_REQUIRE(Cout > 0 && CinR > 0 && CinR <= Cin, "disc_conv_pack_weight: Cout=%d CinR=%d Cin=%d", Cout, CinR, Cin);
    const long total = 9L * Cin * Cout;
    hipLaunchKernelGGL(conv_pack_weight_kernel, dim3(grid_of((total + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)stream, w, wpk, Cout, CinR,
                       Cin, dgrad ? 1 : 0);
    return mrefsr::check_launch("disc_conv_pack_weight");
}

MREFSR_EXPORT int mrefsr_disc_conv3x3_f32(const float *x, const float *wpk, const float *bias, float *y, int N, int H, int W, int Cin, int Cout,
                                          int stride, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && wpk && y, "disc_conv3x3: null pointer");
    int rc = check_conv("disc_conv3x3", N, H, W, Cin, Cout, stride);
    if (rc) return rc;
    const ConvGeo g = {N, H, W, out_size(H, stride), out_size(W, stride), stride, Cin, Cout};
    const long M = (long)N * g.Ho * g.Wo;
    const int NB = Cout % 32 == 0 ? 2 : 1;
    const dim3 grid((unsigned)((M + 127) / 128), (unsigned)(Cout / (16 * NB)), 1);
    hipStream_t st = (hipStream_t)stream;
    if (Cin % 16 == 0) {
        if (NB == 2) hipLaunchKernelGGL((conv_gemm_kernel<0, 2, true>), grid, dim3(256), 0, st, x, wpk, bias, y, g);
        else hipLaunchKernelGGL((conv_gemm_kernel<0, 1, true>), grid, dim3(256), 0, st, x, wpk, bias, y, g);
    } else {
        if (NB == 2) hipLaunchKernelGGL((conv_gemm_kernel<0, 2, false>), grid, dim3(256), 0, st, x, wpk, bias, y, g);
        else hipLaunchKernelGGL((conv_gemm_kernel<0, 1, false>), grid, dim3(256), 0, st, x, wpk, bias, y, g);
    }
    return mrefsr::check_launch("disc_conv3x3");
}

MREFSR_EXPORT int mrefsr_disc_conv3x3_dgrad_f32(const float *dy, const float *wpk_d, float *dx, int N, int H, int W, int Cin, int Cout, int stride,
                                                mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(dy && wpk_d && dx, "disc_conv3x3_dgrad: null pointer");
    int rc = check_conv("disc_conv3x3_dgrad", N, H, W, Cin, Cout, stride);
    if (rc) return rc;
    const ConvGeo g = {N, H, W, out_size(H, stride), out_size(W, stride), stride, Cout, Cin};
    const long M = (long)N * (stride == 2 ? (long)((H + 1) / 2) * ((W + 1) / 2) : (long)H * W);
    const int NB = Cin % 32 == 0 ? 2 : 1;   // (Cin = 4: one 16-column group, 4 of them used)
    const dim3 grid((unsigned)((M + 127) / 128), (unsigned)((Cin + 16 * NB - 1) / (16 * NB)), stride == 2 ? 4 : 1);
    // (every output element belongs to exactly one phase; the largest phase (py = px = 0) sizes the grid, the others return early)
    hipStream_t st = (hipStream_t)stream;
    if (NB == 2) hipLaunchKernelGGL((conv_gemm_kernel<1, 2, true>), grid, dim3(256), 0, st, dy, wpk_d, nullptr, dx, g);
    else hipLaunchKernelGGL((conv_gemm_kernel<1, 1, true>), grid, dim3(256), 0, st, dy, wpk_d, nullptr, dx, g);
    return mrefsr::check_launch("disc_conv3x3_dgrad");
}

MREFSR_EXPORT int64_t mrefsr_disc_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int stride)
{
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (stride != 1 && stride != 2)) return -1;
    return (int64_t)wgrad_splits(N, out_size(H, stride), out_size(W, stride), Cin, Cout) * 9 * Cin * Cout * 4;
}

MREFSR_EXPORT int mrefsr_disc_conv3x3_wgrad_f32(const float *x, const float *dy, float *dw, int N, int H, int W, int Cin, int CinR, int Cout,
                                                int stride, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && dy && dw && workspace, "disc_conv3x3_wgrad: null pointer");
    int rc = check_conv("disc_conv3x3_wgrad", N, H, W, Cin, Cout, stride);
    if (rc) return rc;
    MREFSR_REQUIRE(CinR > 0 && CinR <= Cin, "disc_conv3x3_wgrad: CinR=%d Cin=%d", CinR, Cin);
    const int64_t need = mrefsr_disc_conv3x3_wgrad_workspace_bytes(N, H, W, Cin, Cout, stride);
    MREFSR_REQUIRE(workspace_bytes >= need, "disc_conv3x3_wgrad: workspace of %ld bytes < %ld", (long)workspace_bytes, (long)need);
    const ConvGeo g = {N, H, W, out_size(H, stride), out_size(W, stride), stride, Cin, Cout};
    const int S = wgrad_splits(N, g.Ho, g.Wo, Cin, Cout);
    const long Q = (long)N * g.Ho * g.Wo;
    const int chunk = (int)(((Q + S - 1) / S + 3) / 4 * 4);
    const int S_used = (int)((Q + chunk - 1) / chunk);
    const int NB = Cout % 32 == 0 ? 2 : 1;
    const dim3 grid((unsigned)((9 * Cin + 31) / 32), (unsigned)(Cout / (16 * NB)), (unsigned)S_used);
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    if (NB == 2) hipLaunchKernelGGL(conv_wgrad_kernel<2>, grid, dim3(64), 0, st, x, dy, ws, g, chunk);
    else hipLaunchKernelGGL(conv_wgrad_kernel<1>, grid, dim3(64), 0, st, x, dy, ws, g, chunk);
    const long total = (long)Cout * CinR * 9;
    hipLaunchKernelGGL(conv_wgrad_finish_kernel, dim3(grid_of((total + 255) / 256, 4096)), dim3(256), 0, st, ws, dw, S_used, Cin, CinR, Cout);
    return mrefsr::check_launch("disc_conv3x3_wgrad");
}

MREFSR_EXPORT int64_t mrefsr_disc_chan_workspace_bytes(int64_t P, int C)
{
    if (P <= 0 || C <= 0) return -1;
    return (int64_t)chan_splits(P, C) * 5 * C * 8 + 5L * C * 8;   // partials + the merged sums
}

MREFSR_EXPORT int mrefsr_disc_bias_grad_f32(const float *dy, float *db, int64_t P, int C, void *workspace, int64_t workspace_bytes,
                                            mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(dy && db && workspace, "disc_bias_grad: null pointer");
    MREFSR_REQUIRE(P > 0 && C > 0, "disc_bias_grad: P=%ld C=%d", (long)P, C);
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_disc_chan_workspace_bytes(P, C), "disc_bias_grad: workspace too small");
    const int S = chan_splits(P, C), chunk = (int)((P + S - 1) / S);
    double *part = (double *)workspace, *sums = part + (long)S * 5 * C;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(chan_sums_kernel<0>, dim3(S, (C + 63) / 64), dim3(256), 0, st, dy, nullptr, nullptr, nullptr, nullptr, nullptr, part, (long)P,
                       C, chunk, 0.f);
    hipLaunchKernelGGL(chan_sums_finish_kernel<0>, dim3((C + 255) / 256), dim3(256), 0, st, part, S, C, (long)P, sums, nullptr, db, nullptr);
    return mrefsr::check_launch("disc_bias_grad");
}

MREFSR_EXPORT int mrefsr_disc_bn_lrelu_f32(const float *x, const float *gamma, const float *beta, float *y, float *mean, float *invstd,
                                           float *run_mean, float *run_var, int64_t *num_batches_tracked, int64_t P, int C, float eps, float momentum,
                                           float slope, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && gamma && beta && y && mean && invstd && workspace, "disc_bn_lrelu: null pointer");
    MREFSR_REQUIRE(P > 1 && C > 0 && C % 16 == 0, "disc_bn_lrelu: P=%ld C=%d (more than one value per channel, C a multiple of 16)", (long)P, C);
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_disc_chan_workspace_bytes(P, C), "disc_bn_lrelu: workspace too small");
    const int S = chan_splits(P, C), chunk = (int)((P + S - 1) / S);
    double *part = (double *)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(chan_stats_kernel, dim3(S, (C + 63) / 64), dim3(256), 0, st, x, part, (long)P, C, chunk);
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, st, part, S, C, eps, momentum, mean, invstd, run_mean, run_var,
                       num_batches_tracked);
    const long total = (long)P * C;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_of((total + 255) / 256, 16384)), dim3(256), 0, st, x, mean, invstd, gamma, beta, y, total, C, slope);
    return mrefsr::check_launch("disc_bn_lrelu");
}

MREFSR_EXPORT int mrefsr_disc_bn_lrelu_bwd_f32(const float *gy, const float *y, const float *x, const float *mean, const float *invstd,
                                               const float *gamma, float *gx, float *ggamma, float *gbeta, int64_t P, int C, float slope,
                                               void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(gy && y && x && mean && invstd && gamma && workspace, "disc_bn_lrelu_bwd: null pointer");
    MREFSR_REQUIRE(P > 1 && C > 0 && C % 16 == 0, "disc_bn_lrelu_bwd: P=%ld C=%d", (long)P, C);
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_disc_chan_workspace_bytes(P, C), "disc_bn_lrelu_bwd: workspace too small");
    const int S = chan_splits(P, C), chunk = (int)((P + S - 1) / S);
    double *part = (double *)workspace, *sums = part + (long)S * 5 * C;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(chan_sums_kernel<1>, dim3(S, (C + 63) / 64), dim3(256), 0, st, gy, y, x, nullptr, mean, invstd, part, (long)P, C, chunk, slope);
    hipLaunchKernelGGL(chan_sums_finish_kernel<1>, dim3((C + 255) / 256), dim3(256), 0, st, part, S, C, (long)P, sums, invstd, ggamma, gbeta);
    if (gx) {
        const long total = (long)P * C;
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_of((total + 255) / 256, 16384)), dim3(256), 0, st, gy, y, x, mean, invstd, gamma, sums, gx,
                           total, C, 1.0 / (double)P, slope);
    }
    return mrefsr::check_launch("disc_bn_lrelu_bwd");
}

MREFSR_EXPORT int mrefsr_disc_bn_lrelu_dbl_f32(const float *ggx, const float *ggamma, const float *gbeta, const float *gy, const float *y,
                                               const float *x, const float *mean, const float *invstd, const float *gamma, float *d_gy, float *d_x,
                                               float *d_gamma, int64_t P, int C, float slope, void *workspace, int64_t workspace_bytes,
                                               mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(ggx && gy && y && x && mean && invstd && gamma && workspace, "disc_bn_lrelu_dbl: null pointer");
    MREFSR_REQUIRE(P > 1 && C > 0 && C % 16 == 0, "disc_bn_lrelu_dbl: P=%ld C=%d", (long)P, C);
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_disc_chan_workspace_bytes(P, C), "disc_bn_lrelu_dbl: workspace too small");
    const int S = chan_splits(P, C), chunk = (int)((P + S - 1) / S);
    double *part = (double *)workspace, *sums = part + (long)S * 5 * C;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(chan_sums_kernel<2>, dim3(S, (C + 63) / 64), dim3(256), 0, st, gy, y, x, ggx, mean, invstd, part, (long)P, C, chunk, slope);
    hipLaunchKernelGGL(chan_sums_finish_kernel<2>, dim3((C + 255) / 256), dim3(256), 0, st, part, S, C, (long)P, sums, invstd, d_gamma, nullptr);
    const long total = (long)P * C;
    hipLaunchKernelGGL(bn_dbl_apply_kernel, dim3(grid_of((total + 255) / 256, 16384)), dim3(256), 0, st, ggx, ggamma, gbeta, gy, y, x, mean, invstd,
                       gamma, sums, d_gy, d_x, total, C, (double)P, slope);
    return mrefsr::check_launch("disc_bn_lrelu_dbl");
}

MREFSR_EXPORT int64_t mrefsr_disc_head_workspace_bytes(int N, int C, int J)
{
    if (N <= 0 || C <= 0 || J <= 0) return -1;
    return ((int64_t)N * (3L * J + C) + 2L * N) * 4;   // GH, DH, V [N][J], GGP [N][C], E, GO [N]
}

static int check_head(const char *what, int N, int HW, int C, int J)
{
    if (N <= 0 || HW <= 0) return mrefsr::fail(MREFSR_E_INVALID, "%s: N=%d HW=%d", what, N, HW);
    if (C <= 0 || C > HEAD_MAXC || C % 16 || J <= 0 || J > HEAD_MAXJ)
        return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: C=%d J=%d (C a multiple of 16 up to %d, J up to %d)", what, C, J, HEAD_MAXC, HEAD_MAXJ);
    return MREFSR_OK;
}

MREFSR_EXPORT int mrefsr_disc_head_fwd_f32(const float *f, const float *w1, const float *b1, const float *w2, const float *b2, float *out, float *pooled,
                                           float *hidden, int N, int HW, int C, int J, float slope, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(f && w1 && b1 && w2 && b2 && out && pooled && hidden, "disc_head_fwd: null pointer");
    int rc = check_head("disc_head_fwd", N, HW, C, J);
    if (rc) return rc;
    hipLaunchKernelGGL(head_fwd_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, f, w1, b1, w2, b2, out, pooled, hidden, HW, C, J, slope);
    return mrefsr::check_launch("disc_head_fwd");
}

MREFSR_EXPORT int mrefsr_disc_head_bwd_f32(const float *gs, const float *s, const float *pooled, const float *hidden, const float *w1, const float *w2,
                                           float *gf, float *gw1, float *gb1, float *gw2, float *gb2, int N, int HW, int C, int J, float slope,
                                           void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(gs && s && pooled && hidden && w1 && w2 && gf && workspace, "disc_head_bwd: null pointer");
    int rc = check_head("disc_head_bwd", N, HW, C, J);
    if (rc) return rc;
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_disc_head_workspace_bytes(N, C, J), "disc_head_bwd: workspace too small");
    float *GH = (float *)workspace, *GO = GH + 3L * N * J + (long)N * C + N;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(head_bwd_kernel, dim3(N), dim3(256), 0, st, gs, s, hidden, w1, w2, gf, GH, GO, HW, C, J, slope);
    if (gw1 || gb1 || gw2 || gb2) {
        const long total = (long)J * C;
        hipLaunchKernelGGL(head_params_kernel, dim3(grid_of((total + 255) / 256, 8192)), dim3(256), 0, st, GH, pooled, nullptr, nullptr, GO, nullptr,
                           hidden, nullptr, gw1, gb1, gw2, gb2, N, C, J, slope);
    }
    return mrefsr::check_launch("disc_head_bwd");
}

MREFSR_EXPORT int mrefsr_disc_head_dbl_f32(const float *ggf, const float *gs, const float *s, const float *pooled, const float *hidden, const float *w1,
                                           const float *w2, float *d_gs, float *d_f, float *d_w1, float *d_b1, float *d_w2, float *d_b2, int N, int HW,
                                           int C, int J, float slope, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(ggf && gs && s && pooled && hidden && w1 && w2 && workspace, "disc_head_dbl: null pointer");
    int rc = check_head("disc_head_dbl", N, HW, C, J);
    if (rc) return rc;
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_disc_head_workspace_bytes(N, C, J), "disc_head_dbl: workspace too small");
    float *GH = (float *)workspace, *DH = GH + (long)N * J, *V = DH + (long)N * J, *GGP = V + (long)N * J, *E = GGP + (long)N * C, *GO = E + N;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(head_dbl_kernel, dim3(N), dim3(256), 0, st, ggf, gs, s, hidden, w1, w2, d_gs, d_f, DH, GH, V, GGP, E, GO, HW, C, J, slope);
    if (d_w1 || d_b1 || d_w2 || d_b2) {
        const long total = (long)J * C;
        hipLaunchKernelGGL(head_params_kernel, dim3(grid_of((total + 255) / 256, 8192)), dim3(256), 0, st, DH, pooled, GH, GGP, E, GO, hidden, V, d_w1,
                           d_b1, d_w2, d_b2, N, C, J, slope);
    }
    return mrefsr::check_launch("disc_head_dbl");
}
