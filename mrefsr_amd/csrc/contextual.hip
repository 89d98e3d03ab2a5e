// Contextual loss of the training step (Mechrez et al., ECCV 2018; losses.ContextualLoss, train.contextual_opt): what
// the VGG19 node of mrefsr_amd/archs/nhwc_train.py (_VggContextual) runs per tap.  x (features of the output) and y (of the target),
// both NHWC [B][N][C] fp32, N = h w; i runs over positions of x, j over positions of y.
//   cx_mean          mu[b][c] = mean_p y[b][p][c], fixed order
//   cx_normalise     xn = (x - mu) / max(|x - mu|, 1e-12) per position, the same for yn; 1 / max(..) of x kept for the backward
//   cx_dist          d[b][i][j] = 1 - <xn_i, yn_j> on v_mfma_f32_16x16x4_f32, operands straight from the NHWC rows -> scratch [B][N][ld]
//   cx_row           per row i: m = min_j d (lowest j on ties), Z = sum_j w,  w = exp((1 - d / (m + 1e-5)) / h)
//   cx_col           per column j: max_i w / Z[i] (lowest i on ties) and its row
//   cx_finish        CX[b] = mean_j of the column maxima (fixed order), tap loss = mean_b -log(CX[b] + 1e-5), the running total
// backward (d is recomputed: the scratch of the forward call is dead):
//   cx_dist          again
//   cx_rowgrad       per row i: the scatter sums over the columns that selected i, then d[i][:] -> E[i][:] = d loss / d S[i][:] in place
//   cx_grad_gemm     dxn = E yn, the second MFMA product
//   cx_grad_finish   dx (+)= (dxn - xn <xn, dxn>) / max(|x - mu|, 1e-12), + max |dx| for the fp16-split dgrad
// One N x N fp32 matrix per sample is materialised (N <= MREFSR_CX_MAX_N): exp((1 - d / (m + eps)) / h) needs the row minimum first
// and has no online rescaling, and the column maximum needs Z; with d in scratch (41 MB at B = 4, N = 1600: it stays in the 256 MB
// of MALL) the three statistics passes are memory-bound sweeps and the product runs once per direction.
// Every sum has a fixed order; no float atomics; nothing is read back.
//
// CoBi (Zhang et al., "Zoom to Learn, Learn to Zoom", ICCV 2019): the *_sp entry points take the tap's grid h x w and weight_sp = ws
// in [0, 1), and cx_dist stores d = (1 - ws) (1 - <xn_i, yn_j>) + ws ((r_i - r_j)^2 + (c_i - c_j)^2) / (h^2 + w^2), i = r_i w + c_i;
// every later pass runs on that d as it stands; the norms and the product of such a call are taken in double (cx_normalise<true>,
// cx_dist<true> on the f64 MFMA).  The spatial term is a constant: the backward is the closed form above on the
// combined d with coef (1 - ws).  ws = 0 launches the kernels of the plain entry points.  What feeds such taps:
//   cx_patches       image NCHW [B][3][H][W] -> the size x size RGB patches at a stride as NHWC features [B][oh ow][Cpad], the
//                    channels in F.unfold's (c, dy, dx) order, zeros past 3 size^2; its adjoint in gather form (no atomics)
//   cx_subsample     NHWC tap [B][h][w][C] -> the positions (r s, c s); its adjoint scatters into the tap's gradient buffer
#include "common.h"
#include <type_traits>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr float CX_EPS = 1e-5f;
constexpr float CX_NORM_FLOOR = 1e-12f;

// the contextual weight of one distance: me = m + eps of the row, h = band_width.  The one expression every pass evaluates, so
// that the column pass and the backward see the bits the row pass summed
__device__ __forceinline__ float cx_weight(float d, float me, float h) { return expf((1.0f - d / me) / h); }

// mu[b][c]: block = 16 channels x 64 position groups (16 blocks of 400-step loops took 100 us at C = 256, N = 1600); group g adds the
// positions g, g + 64, ... in double, thread (0, c) the 64 groups in ascending order
__global__ __launch_bounds__(1024) void cx_mean_kernel(const float *__restrict__ y, float *__restrict__ mu, int N, int C)
{
    __shared__ double part[64][16];
    const int b = blockIdx.y, t = threadIdx.x & 15, c = blockIdx.x * 16 + t, g = threadIdx.x >> 4;
    const float *yb = y + (long)b * N * C + c;
    double s = 0.0;
    for (int p = g; p < N; p += 64) s += (double)yb[(long)p * C];
    part[g][t] = s;
    __syncthreads();
    if (g == 0) {
        for (int k = 1; k < 64; ++k) s += part[k][t];
        mu[(long)b * C + c] = (float)(s / (double)N);
    }
}

// one wave per position: rows [0, BN) are x, rows [BN, 2 BN) are y.  C <= 512: at most two float4 per lane.
// HI (the CoBi entry points): the squares are added, the root taken and the elements divided in double, each element rounded once.
// With the spatial term the row minima of repetitive texture are 1e-3 and less, and an fp32 norm -- a common factor 1 + 1e-7 on
// every distance of a row or a column -- then carries the loss to 1e-6; HI = false is the plain kernel, bit for bit
template <bool HI>
__global__ __launch_bounds__(256) void cx_normalise_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ mu,
                                                           float *__restrict__ xn, float *__restrict__ yn, float *__restrict__ rnorm, long BN,
                                                           int N, int C)
{
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= 2 * BN) return;   // (whole waves leave: no barrier below)
    const bool is_x = row < BN;
    const long r = is_x ? row : row - BN;
    const int C4 = C >> 2;
    const float4 *src = reinterpret_cast<const float4 *>((is_x ? x : y) + r * C);
    const float4 *m4 = reinterpret_cast<const float4 *>(mu + (r / N) * C);
    float4 *dst = reinterpret_cast<float4 *>((is_x ? xn : yn) + r * C);
    float4 v[2];
    float ss = 0.f;
    double sd = 0.0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int k = lane + 64 * q;
        v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < C4) {
            const float4 a = src[k], u = m4[k];
            v[q] = make_float4(a.x - u.x, a.y - u.y, a.z - u.z, a.w - u.w);
            if constexpr (HI)
                sd += (double)v[q].x * v[q].x + (double)v[q].y * v[q].y + (double)v[q].z * v[q].z + (double)v[q].w * v[q].w;
            else
                ss += v[q].x * v[q].x + v[q].y * v[q].y + v[q].z * v[q].z + v[q].w * v[q].w;
        }
    }
    if constexpr (HI) {
        sd = __shfl(mrefsr::wave_sum(sd), 0, 64);
        const double root = sqrt(sd);
        const bool floored = root < (double)CX_NORM_FLOOR;
        const double den = floored ? (double)CX_NORM_FLOOR : root;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = lane + 64 * q;
            if (k < C4)
                dst[k] = make_float4((float)(v[q].x / den), (float)(v[q].y / den), (float)(v[q].z / den), (float)(v[q].w / den));
        }
        if (is_x && lane == 0) rnorm[r] = floored ? 1.0f / CX_NORM_FLOOR : (float)(1.0 / den);   // (the floor as cx_grad_finish tests it)
    } else {
        ss = __shfl(mrefsr::wave_sum(ss), 0, 64);
        const float den = fmaxf(sqrtf(ss), CX_NORM_FLOOR);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = lane + 64 * q;
            if (k < C4) dst[k] = make_float4(v[q].x / den, v[q].y / den, v[q].z / den, v[q].w / den);
        }
        if (is_x && lane == 0) rnorm[r] = 1.0f / den;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// d = 1 - xn yn^T on the f32 matrix pipe.  Block = 4 waves = one 64 x 64 tile of d[b]; wave w: the 32 x 32 quarter (w >> 1, w & 1),
// 2 x 2 accumulators.  A[m][k] = xn[i0 + m][c], B[k][n] = yn[j0 + n][c]: a lane holds a float4 of row (l & 15), channels
// k0 + 4 (l >> 4) .. + 3 of both maps and feeds element e to the e-th MFMA of the 16-channel step, so the MFMA's local k = l >> 4 is
// channel k0 + 4 (l >> 4) + e on both sides (gram_bwd_kernel's operand trick).  Rows past N load zeros and are not stored.
// D: column (j) = lane & 15, row (i) = 4 (lane >> 4) + r.
// ---------------------------------------------------------------------------------------------------------------
// SP (CoBi): the same tiling on v_mfma_f64_16x16x4_f64 -- the operands converted lane by lane, A / B laid out as in the f32 form,
// D: column (j) = lane & 15, row (i) = (lane >> 4) + 4 r -- and an epilogue that stores oms (1 - <xn_i, yn_j>) + ws d_sp[i][j],
// formed in double and rounded once (oms = 1 - ws; gw: the grid's width; diag = h^2 + w^2).  Why double: an f32 accumulator near 1
// is good to 6e-8, which is 1e-4 of a row minimum of 1e-3 and less -- what the spatial term leaves of repetitive texture -- and the
// loss then carries 1e-6.  A thread owns the 8 rows i0 + 16 a + (l >> 4) + 4 r and the 2 columns j0 + 16 q + (l & 15): their (r, c)
// come from one integer division by gw each, before the stores.  SP = false is the plain kernel, bit for bit
template <bool SP>
__global__ __launch_bounds__(256) void cx_dist_kernel(const float *__restrict__ xn, const float *__restrict__ yn, float *__restrict__ d, int N,
                                                      int C, int ld, int gw, double oms, double ws, double diag)
{
    using acc_t = std::conditional_t<SP, f64x4, f32x4>;
    const int b = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane >> 4, cl = lane & 15;
    const int i0 = blockIdx.y * 64 + (wave >> 1) * 32, j0 = blockIdx.x * 64 + (wave & 1) * 32;
    const float *xb = xn + (long)b * N * C, *yb = yn + (long)b * N * C;
    const float4 *xr[2], *yr[2];
    bool xok[2], yok[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int i = i0 + 16 * a + cl, j = j0 + 16 * a + cl;
        xok[a] = i < N, yok[a] = j < N;
        xr[a] = reinterpret_cast<const float4 *>(xb + (long)(xok[a] ? i : 0) * C) + kl;
        yr[a] = reinterpret_cast<const float4 *>(yb + (long)(yok[a] ? j : 0) * C) + kl;
    }
    acc_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[a][q] = acc_t{0, 0, 0, 0};
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k4 = 0; k4 < C / 4; k4 += 4) {
        float4 av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) av[a] = xok[a] ? xr[a][k4] : zero, bv[a] = yok[a] ? yr[a][k4] : zero;
        const float ae[2][4] = {{av[0].x, av[0].y, av[0].z, av[0].w}, {av[1].x, av[1].y, av[1].z, av[1].w}};
        const float be[2][4] = {{bv[0].x, bv[0].y, bv[0].z, bv[0].w}, {bv[1].x, bv[1].y, bv[1].z, bv[1].w}};
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    if constexpr (SP)
                        acc[a][q] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)ae[a][e], (double)be[q][e], acc[a][q], 0, 0, 0);
                    else
                        acc[a][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ae[a][e], be[q][e], acc[a][q], 0, 0, 0);
                }
    }
    float *db = d + (long)b * N * ld;
    if constexpr (SP) {
        int ir[2][4], ic[2][4], jr[2], jc[2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + 16 * a + kl + 4 * r;
                ir[a][r] = i / gw, ic[a][r] = i - ir[a][r] * gw;
            }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = j0 + 16 * q + cl;
            jr[q] = j / gw, jc[q] = j - jr[q] * gw;
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int j = j0 + 16 * q + cl;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = i0 + 16 * a + kl + 4 * r;
                    const int dr = ir[a][r] - jr[q], dc = ic[a][r] - jc[q];
                    if (i < N && j < N) db[(long)i * ld + j] = (float)(oms * (1.0 - acc[a][q][r]) + ws * ((double)(dr * dr + dc * dc) / diag));
                }
            }
    } else {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int j = j0 + 16 * q + cl;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = i0 + 16 * a + 4 * kl + r;
                    if (i < N && j < N) db[(long)i * ld + j] = 1.0f - acc[a][q][r];
                }
            }
    }
}

// one wave per row i of d[b]: the minimum with the lowest j on ties, then Z in double over the lane's columns j = l, l + 64, ... and
// the wave's shuffle tree.  rowf: [2][BN] = m, Z
__global__ __launch_bounds__(256) void cx_row_kernel(const float *__restrict__ d, float *__restrict__ rowf, int *__restrict__ jmin, long BN,
                                                     int N, int ld, float h)
{
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= BN) return;
    const float *dr = d + row * ld;
    float best = INFINITY;
    int bj = 0x7fffffff;
    for (int j = lane; j < N; j += 64) {
        const float v = dr[j];
        if (v < best) best = v, bj = j;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (ov < best || (ov == best && oj < bj)) best = ov, bj = oj;
    }
    const float me = best + CX_EPS;
    double z = 0.0;
    for (int j = lane; j < N; j += 64) z += (double)cx_weight(dr[j], me, h);
    z = mrefsr::wave_sum(z);
    if (lane == 0) {
        rowf[row] = best;
        rowf[BN + row] = (float)z;
        jmin[row] = bj == 0x7fffffff ? 0 : bj;   // (a row of NaNs: any index inside the map)
    }
}

// block = 32 columns x 32 row groups; group g scans the rows [g R, (g + 1) R), R = ceil(N / 32), a later row replaces the maximum
// only when strictly greater; thread (0, j) merges the groups in ascending order by the same rule: the lowest i wins a tie.
// (64 columns x 4 groups -- 100 blocks of 400-step loops at N = 1600 -- took 151 us.)  cxmax: [BN], the maximum of w / Z
__global__ __launch_bounds__(1024) void cx_col_kernel(const float *__restrict__ d, const float *__restrict__ rowf, float *__restrict__ cxmax,
                                                      int *__restrict__ imax, long BN, int N, int ld, float h)
{
    __shared__ float sv[32][32];
    __shared__ int si[32][32];
    const int b = blockIdx.y, t = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int j = blockIdx.x * 32 + t;
    const int R = (N + 31) / 32, ib = g * R, ie = min(N, ib + R);
    const float *db = d + (long)b * N * ld;
    const float *mrow = rowf + (long)b * N, *zrow = rowf + BN + (long)b * N;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if (j < N) {
        for (int i = ib; i < ie; ++i) {
            const float v = db[(long)i * ld + j];
            const float cx = cx_weight(v, mrow[i] + CX_EPS, h) / zrow[i];
            if (cx > best) best = cx, bi = i;
        }
    }
    sv[g][t] = best, si[g][t] = bi;
    __syncthreads();
    if (g == 0 && j < N) {
        for (int k = 1; k < 32; ++k)
            if (sv[k][t] > best) best = sv[k][t], bi = si[k][t];
        const long o = (long)b * N + j;
        cxmax[o] = bi == 0x7fffffff ? 0.f : best;
        imax[o] = bi == 0x7fffffff ? 0 : bi;
    }
}

// one block: CX[b] = (sum_j of the column maxima, thread-strided in double, then the block's tree) / N; thread 0 the mean of
// -log(CX[b] + eps) over b in order, and the running weighted total of the taps
__global__ __launch_bounds__(256) void cx_finish_kernel(const float *__restrict__ cxmax, float *__restrict__ cx, float *__restrict__ tap_loss,
                                                        float *__restrict__ run, float *__restrict__ total, int B, int N, float weight,
                                                        float loss_weight, int first)
{
    __shared__ double red[256];
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        double s = 0.0;
        for (int j = threadIdx.x; j < N; j += 256) s += (double)cxmax[(long)b * N + j];
        s = mrefsr::block_sum<256>(red, s);
        const float c = (float)(s / (double)N);
        if (threadIdx.x == 0) cx[b] = c;
        acc += -log((double)c + (double)CX_EPS);
    }
    if (threadIdx.x == 0) {
        const float l = (float)(acc / (double)B);
        tap_loss[0] = l;
        const float r = __fadd_rn(first ? 0.f : run[0], __fmul_rn(l, weight));
        run[0] = r;
        total[0] = __fmul_rn(r, loss_weight);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Backward, one block per row i of sample b.  a = -gup coef / (B N (CX[b] + eps)) is d loss / d cx at every selected element.
//   P = a sum_{j: imax[j] = i} cxmax[j]   (= T[i] / Z[i])
//   GW[i][j] = G[i][j] w[i][j] = [imax[j] = i] a cxmax[j] - P w[i][j] / Z[i]
//   U = sum_j GW[i][j] d[i][j]
//   E[i][j] = -dd[i][j] = GW[i][j] / (h me) - [j = jmin[i]] U / (h me^2),  me = m[i] + eps
// The scatter over j is this block's own scan of imax in a fixed order (thread-strided in double, the block's tree).  U is the sum
// of the very GW values that E is made of (they pass through the row: a thread reads back what it wrote), not Q - P WD / Z from row
// sums of the forward: the rounding errors of GW then reach the gradient through U and through E with opposite signs, and the
// fp32 error of the result is that of torch's autograd (3e-5 -> 2e-6 of the gradient's norm).  d[i][:] is replaced by E[i][:], the
// columns N .. ld - 1 by zeros (cx_grad_gemm reads whole float4s of a row).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cx_rowgrad_kernel(float *__restrict__ d, const float *__restrict__ rowf, const int *__restrict__ jmin,
                                                         const float *__restrict__ cxmax, const int *__restrict__ imax,
                                                         const float *__restrict__ cx, const float *__restrict__ gup, float coef, long BN, int B,
                                                         int N, int ld, float h)
{
    __shared__ double red[256];
    const long row = blockIdx.x;
    const int b = (int)(row / N), i = (int)(row - (long)b * N);
    const float *cmax = cxmax + (long)b * N;
    const int *im = imax + (long)b * N;
    const float up = gup ? gup[0] : 1.0f;
    const float a = -(up * coef) / ((float)B * (float)N * (cx[b] + CX_EPS));
    double ps = 0.0;
    for (int j = threadIdx.x; j < N; j += 256)
        if (im[j] == i) ps += (double)cmax[j];
    ps = mrefsr::block_sum<256>(red, ps);
    const float me = rowf[row] + CX_EPS, z = rowf[BN + row];
    const float pz = a * (float)ps / z;
    float *dr = d + row * ld;
    double us = 0.0;
    for (int j = threadIdx.x; j < N; j += 256) {
        const float v = dr[j];
        const float gw = (im[j] == i ? a * cmax[j] : 0.f) - pz * cx_weight(v, me, h);
        us += (double)gw * (double)v;
        dr[j] = gw;
    }
    us = mrefsr::block_sum<256>(red, us);
    const float inv = 1.0f / (h * me);
    const float um = (float)us * inv / me;
    const int jm = jmin[row];
    for (int j = threadIdx.x; j < ld; j += 256) dr[j] = j < N ? dr[j] * inv - (j == jm ? um : 0.f) : 0.f;
}

// dxn[b][i][c] = sum_j E[i][j] yn[j][c].  Block = 4 waves = 64 rows i x 64 channels; wave: 16 rows x 64 channels, four accumulators.
// A[m][k] = E[i0 + m][j]: a float4 of row (l & 15), columns jj + 4 (l >> 4) .. + 3 (E's rows are ld long, ld a multiple of 16, zero
// past N), element e to the e-th MFMA; B[k][n] = yn[jj + 4 (l >> 4) + e][c0 + 16 q + n], zero for j >= N.
// D: column (c) = lane & 15, row (i) = 4 (lane >> 4) + r.
__global__ __launch_bounds__(256) void cx_grad_gemm_kernel(const float *__restrict__ e, const float *__restrict__ yn, float *__restrict__ dxn,
                                                           int N, int C, int ld)
{
    const int b = blockIdx.z, c0 = blockIdx.y * 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane >> 4, cl = lane & 15;
    const int i0 = (blockIdx.x * 4 + wave) * 16;
    const int ia = i0 + cl;
    const bool iok = ia < N;
    const float4 *er = reinterpret_cast<const float4 *>(e + ((long)b * N + (iok ? ia : 0)) * ld) + kl;
    const float *yb = yn + (long)b * N * C + c0 + cl;
    f32x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int jj = 0; jj < ld; jj += 16) {
        const float4 ev = iok ? er[jj >> 2] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float ee[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = jj + 4 * kl + k;
            const bool jok = j < N;
            const float *yr = yb + (long)(jok ? j : 0) * C;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float bv = jok ? yr[16 * q] : 0.f;
                acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ee[k], bv, acc[q], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * kl + r;
            if (i < N) dxn[((long)b * N + i) * C + c0 + 16 * q + cl] = acc[q][r];
        }
}

// one wave per position of x: through the normalisation, dx = (dxn - xn <xn, dxn>) rnorm (a position at the norm floor: dxn rnorm);
// the centring subtracts a constant of y, so this is d loss / d x.  Written or added into g, max |g| published.
__global__ __launch_bounds__(256) void cx_grad_finish_kernel(const float *__restrict__ dxn, const float *__restrict__ xn,
                                                             const float *__restrict__ rnorm, float *__restrict__ g, long BN, int C,
                                                             int accumulate, unsigned int *__restrict__ amax_bits)
{
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    float amx = 0.f;
    if (row < BN) {
        const int C4 = C >> 2;
        const float4 *dv = reinterpret_cast<const float4 *>(dxn + row * C), *xv = reinterpret_cast<const float4 *>(xn + row * C);
        float4 *gv = reinterpret_cast<float4 *>(g + row * C);
        float4 dq[2], xq[2];
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = lane + 64 * q;
            dq[q] = xq[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < C4) {
                dq[q] = dv[k], xq[q] = xv[k];
                t += dq[q].x * xq[q].x + dq[q].y * xq[q].y + dq[q].z * xq[q].z + dq[q].w * xq[q].w;
            }
        }
        t = __shfl(mrefsr::wave_sum(t), 0, 64);
        const float rn = rnorm[row];
        if (rn >= 1.0f / CX_NORM_FLOOR) t = 0.f;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = lane + 64 * q;
            if (k < C4) {
                float4 v = make_float4((dq[q].x - xq[q].x * t) * rn, (dq[q].y - xq[q].y * t) * rn, (dq[q].z - xq[q].z * t) * rn,
                                       (dq[q].w - xq[q].w * t) * rn);
                if (accumulate) {
                    const float4 o = gv[k];
                    v.x += o.x, v.y += o.y, v.z += o.z, v.w += o.w;
                }
                gv[k] = v;
                amx = fmaxf(amx, mrefsr::amax4(v));
            }
        }
    }
    if (amax_bits) mrefsr::publish_amax<true>(amax_bits, amx);   // (one wave per position: thousands of waves on one word)
}

// ---------------------------------------------------------------------------------------------------------------
// RGB patches as features (CoBi_RGB).  One thread per float4 of out [B][oh ow][Cpad]: channel k = (c size + dy) size + dx of patch
// (pr, pc) is img[b][c][pr stride + dy][pc stride + dx] (norm: (v + 1) * 0.5 first), zero for k >= 3 size^2
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cx_patches_kernel(const float *__restrict__ img, float *__restrict__ out, long total4, int H, int W,
                                                         int size, int stride, int oh, int ow, int Cpad, int norm)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total4) return;
    const int C4 = Cpad >> 2, k4 = (int)(t % C4);
    const long pos = t / C4;
    const int pc = (int)(pos % ow), pr = (int)((pos / ow) % oh);
    const long b = pos / ((long)oh * ow);
    const int ss = size * size, K = 3 * ss;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = 4 * k4 + e;
        v[e] = 0.f;
        if (k < K) {
            const int c = k / ss, rem = k - c * ss, dy = rem / size, dx = rem - dy * size;
            const float a = img[((b * 3 + c) * H + pr * stride + dy) * W + pc * stride + dx];
            v[e] = norm ? (a + 1.0f) * 0.5f : a;
        }
    }
    reinterpret_cast<float4 *>(out)[t] = make_float4(v[0], v[1], v[2], v[3]);
}

// the adjoint in gather form, one thread per image element (b, c, y, x): the patches (pr, pc) with pr stride <= y < pr stride + size
// and the same in x, at most ceil(size / stride)^2 of them, added in ascending (pr, pc) order; times scale; written or added
__global__ __launch_bounds__(256) void cx_patches_bwd_kernel(const float *__restrict__ g, float *__restrict__ dimg, long total, int H, int W,
                                                             int size, int stride, int oh, int ow, int Cpad, float scale, int accumulate)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int x = (int)(t % W), y = (int)((t / W) % H);
    const long bc = t / ((long)H * W);
    const int c = (int)(bc % 3);
    const long b = bc / 3;
    const int r0 = y < size ? 0 : (y - size + stride) / stride, r1 = min(oh - 1, y / stride);
    const int c0 = x < size ? 0 : (x - size + stride) / stride, c1 = min(ow - 1, x / stride);
    const float *gb = g + b * oh * ow * Cpad + c * size * size;
    float s = 0.f;
    for (int pr = r0; pr <= r1; ++pr) {
        const int dy = y - pr * stride;
        for (int pc = c0; pc <= c1; ++pc) s += gb[((long)pr * ow + pc) * Cpad + dy * size + (x - pc * stride)];
    }
    s *= scale;
    dimg[t] = accumulate ? dimg[t] + s : s;
}

// the positions (r s, c s) of a tap [B][h][w][C] -> [B][hs][ws][C], one thread per float4
__global__ __launch_bounds__(256) void cx_subsample_kernel(const float *__restrict__ f, float *__restrict__ out, long total4, int h, int w, int C4,
                                                           int s, int hs, int ws)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total4) return;
    const int k = (int)(t % C4);
    const long pos = t / C4;
    const int c = (int)(pos % ws), r = (int)((pos / ws) % hs);
    const long b = pos / ((long)hs * ws);
    reinterpret_cast<float4 *>(out)[t] = reinterpret_cast<const float4 *>(f)[((b * h + (long)r * s) * w + (long)c * s) * C4 + k];
}

// its adjoint over the float4s of the tap's gradient buffer g [B][h][w][C], CX_SUB_ITEMS per thread a block's width apart (one
// float4 per thread had 12800 waves peek at the one amax word: 63 us for the 13 MB of a relu2_2 buffer): a sampled position gets
// (accumulate ? g : 0) + gs, any other keeps its value (accumulate) or is zeroed; max |g| of the whole buffer is published as
// cx_grad_finish does
constexpr int CX_SUB_ITEMS = 8;
__global__ __launch_bounds__(256) void cx_subsample_bwd_kernel(const float *__restrict__ gs, float *__restrict__ g, long total4, int h, int w,
                                                               int C4, int s, int hs, int ws, int accumulate,
                                                               unsigned int *__restrict__ amax_bits)
{
    float amx = 0.f;
#pragma unroll
    for (int it = 0; it < CX_SUB_ITEMS; ++it) {
        const long t = ((long)blockIdx.x * CX_SUB_ITEMS + it) * 256 + threadIdx.x;
        if (t >= total4) break;
        const int k = (int)(t % C4);
        const long pos = t / C4;
        const int c = (int)(pos % w), r = (int)((pos / w) % h);
        const long b = pos / ((long)h * w);
        float4 *gp = reinterpret_cast<float4 *>(g) + t;
        float4 v = accumulate ? *gp : make_float4(0.f, 0.f, 0.f, 0.f);
        const bool hit = r % s == 0 && c % s == 0;
        if (hit) {
            const float4 a = reinterpret_cast<const float4 *>(gs)[((b * hs + r / s) * ws + c / s) * C4 + k];
            v.x += a.x, v.y += a.y, v.z += a.z, v.w += a.w;
        }
        if (hit || !accumulate) *gp = v;
        amx = fmaxf(amx, mrefsr::amax4(v));
    }
    if (amax_bits) mrefsr::publish_amax<true>(amax_bits, amx);
}

inline int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }
inline int cx_ld(int N) { return (N + 15) / 16 * 16; }
inline bool cx_shape_ok(int B, int N, int C)
{
    return B >= 1 && B <= 65535 && N >= 2 && N <= MREFSR_CX_MAX_N && (C == 64 || C == 128 || C == 256 || C == 512);
}
// scratch: mu [B][C] | d [B][N][ld] | (backward) dxn [B][N][C]
inline int64_t cx_off_d(int B, int C) { return align256((int64_t)B * C * 4); }
inline int64_t cx_off_dxn(int B, int N, int C) { return cx_off_d(B, C) + align256((int64_t)B * N * cx_ld(N) * 4); }

// null / non-positive sizes are invalid arguments; an N over the bound or another channel count is a shape the kernels do not take
#define CX_REQUIRE_SHAPE(what)                                                                                                       \
    do {                                                                                                                             \
        MREFSR_REQUIRE(B >= 1 && B <= 65535 && N >= 2 && C > 0, "%s: B=%d N=%d C=%d (1 <= B <= 65535, N >= 2)", what, B, N, C);       \
        if (!cx_shape_ok(B, N, C))                                                                                                   \
            return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: N=%d C=%d (N <= %d: one N x N matrix per sample is materialised; C of "    \
                                "64, 128, 256, 512)", what, N, C, MREFSR_CX_MAX_N);                                                   \
    } while (0)

// the grid of a *_sp call: h, w >= 1 or the arguments are invalid; h w over the bound is a shape the kernels do not take (N = h w
// is formed only below it: no overflow)
#define CX_REQUIRE_GRID(what)                                                                                                        \
    do {                                                                                                                             \
        MREFSR_REQUIRE(h >= 1 && w >= 1, "%s: a grid of %d x %d positions", what, h, w);                                              \
        if ((int64_t)h * w > MREFSR_CX_MAX_N)                                                                                        \
            return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: a grid of %d x %d positions (h w <= %d: one N x N matrix per sample is "   \
                                "materialised)", what, h, w, MREFSR_CX_MAX_N);                                                        \
        MREFSR_REQUIRE(weight_sp >= 0.f && weight_sp < 1.f, "%s: weight_sp=%g (a number in [0, 1))", what, (double)weight_sp);        \
    } while (0)

// the spatial term of a call: gw = 0 is the plain distance
struct CxSpatial {
    int gh, gw;
    float ws;
};

void launch_dist(const float *xn, const float *yn, float *d, int B, int N, int C, CxSpatial sp, hipStream_t st)
{
    const int T = (N + 63) / 64;
    if (sp.gw > 0 && sp.ws > 0.f)
        hipLaunchKernelGGL(cx_dist_kernel<true>, dim3(T, T, B), dim3(256), 0, st, xn, yn, d, N, C, cx_ld(N), sp.gw, 1.0 - (double)sp.ws,
                           (double)sp.ws, (double)(sp.gh * sp.gh + sp.gw * sp.gw));
    else
        hipLaunchKernelGGL(cx_dist_kernel<false>, dim3(T, T, B), dim3(256), 0, st, xn, yn, d, N, C, cx_ld(N), 0, 1.0, 0.0, 1.0);
}

int cx_forward(const char *what, const float *x, const float *y, int B, int N, int C, float band_width, CxSpatial sp, float *xn, float *yn,
               float *rnorm, float *rowf, int32_t *jmin, float *cxmax, int32_t *imax, float *cx, float *tap_loss, float weight,
               float loss_weight, int first, float *run, float *total, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(band_width > 0.f && band_width < INFINITY, "%s: band_width=%g (a finite number > 0)", what, (double)band_width);
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_contextual_workspace_bytes(B, N, C, 0), "%s: workspace of %ld bytes < %ld", what,
                   (long)workspace_bytes, (long)mrefsr_contextual_workspace_bytes(B, N, C, 0));
    MREFSR_REQUIRE((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(xn) |
                    reinterpret_cast<uintptr_t>(yn) | reinterpret_cast<uintptr_t>(workspace)) % 16 == 0,
                   "%s: pointers must be 16-byte aligned", what);
    hipStream_t st = (hipStream_t)stream;
    const long BN = (long)B * N;
    const int ld = cx_ld(N);
    float *mu = (float *)workspace, *d = (float *)((char *)workspace + cx_off_d(B, C));
    hipLaunchKernelGGL(cx_mean_kernel, dim3(C / 16, B), dim3(1024), 0, st, y, mu, N, C);
    if (sp.gw > 0 && sp.ws > 0.f)
        hipLaunchKernelGGL(cx_normalise_kernel<true>, dim3((unsigned)((2 * BN + 3) / 4)), dim3(256), 0, st, x, y, (const float *)mu, xn, yn, rnorm,
                           BN, N, C);
    else
        hipLaunchKernelGGL(cx_normalise_kernel<false>, dim3((unsigned)((2 * BN + 3) / 4)), dim3(256), 0, st, x, y, (const float *)mu, xn, yn, rnorm,
                           BN, N, C);
    launch_dist(xn, yn, d, B, N, C, sp, st);
    hipLaunchKernelGGL(cx_row_kernel, dim3((unsigned)((BN + 3) / 4)), dim3(256), 0, st, (const float *)d, rowf, jmin, BN, N, ld, band_width);
    hipLaunchKernelGGL(cx_col_kernel, dim3((N + 31) / 32, B), dim3(1024), 0, st, (const float *)d, (const float *)rowf, cxmax, imax, BN, N, ld,
                       band_width);
    hipLaunchKernelGGL(cx_finish_kernel, dim3(1), dim3(256), 0, st, (const float *)cxmax, cx, tap_loss, run, total, B, N, weight, loss_weight,
                       first ? 1 : 0);
    return mrefsr::check_launch(what);
}

// (the spatial term is a constant of d: every backward quantity is linear in a, so the factor 1 - ws of d d / d <xn_i, yn_j> rides on coef)
int cx_backward(const char *what, const float *xn, const float *yn, const float *rnorm, int B, int N, int C, float band_width, CxSpatial sp,
                const float *rowf, const int32_t *jmin, const float *cxmax, const int32_t *imax, const float *cx, const float *gup, float coef,
                float *dx, int accumulate, float *amax, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(band_width > 0.f && band_width < INFINITY, "%s: band_width=%g (a finite number > 0)", what, (double)band_width);
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_contextual_workspace_bytes(B, N, C, 1), "%s: workspace of %ld bytes < %ld", what,
                   (long)workspace_bytes, (long)mrefsr_contextual_workspace_bytes(B, N, C, 1));
    MREFSR_REQUIRE((reinterpret_cast<uintptr_t>(xn) | reinterpret_cast<uintptr_t>(yn) | reinterpret_cast<uintptr_t>(dx) |
                    reinterpret_cast<uintptr_t>(workspace)) % 16 == 0,
                   "%s: pointers must be 16-byte aligned", what);
    hipStream_t st = (hipStream_t)stream;
    const long BN = (long)B * N;
    const int ld = cx_ld(N);
    float *d = (float *)((char *)workspace + cx_off_d(B, C)), *dxn = (float *)((char *)workspace + cx_off_dxn(B, N, C));
    if (sp.gw > 0 && sp.ws > 0.f) coef *= (float)(1.0 - (double)sp.ws);
    launch_dist(xn, yn, d, B, N, C, sp, st);
    hipLaunchKernelGGL(cx_rowgrad_kernel, dim3((unsigned)BN), dim3(256), 0, st, d, rowf, jmin, cxmax, imax, cx, gup, coef, BN, B, N, ld,
                       band_width);
    hipLaunchKernelGGL(cx_grad_gemm_kernel, dim3((N + 63) / 64, C / 64, B), dim3(256), 0, st, (const float *)d, yn, dxn, N, C, ld);
    hipLaunchKernelGGL(cx_grad_finish_kernel, dim3((unsigned)((BN + 3) / 4)), dim3(256), 0, st, (const float *)dxn, xn, rnorm, dx, BN, C,
                       accumulate ? 1 : 0, reinterpret_cast<unsigned int *>(amax));
    return mrefsr::check_launch(what);
}

inline int cx_patch_channels(int size) { const int k = 3 * size * size; return k <= 64 ? 64 : k <= 128 ? 128 : k <= 256 ? 256 : 512; }

// image, patch and stride of a cx_patches call: -> MREFSR_OK with oh, ow set
int cx_patch_geometry(const char *what, int B, int H, int W, int size, int stride, int Cpad, int *oh, int *ow)
{
    MREFSR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && size >= 1 && stride >= 1, "%s: B=%d H=%d W=%d size=%d stride=%d", what, B, H, W, size, stride);
    if (size > 13)
        return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: size=%d (3 size^2 <= 512 channels: size <= 13)", what, size);
    MREFSR_REQUIRE(size <= H && size <= W, "%s: a patch of %d x %d in an image of %d x %d", what, size, size, H, W);
    MREFSR_REQUIRE(Cpad == cx_patch_channels(size), "%s: Cpad=%d (size %d: %d)", what, Cpad, size, cx_patch_channels(size));
    MREFSR_REQUIRE((int64_t)B * 3 * H * W < ((int64_t)1 << 31), "%s: an image batch of %d x 3 x %d x %d", what, B, H, W);
    *oh = (H - size) / stride + 1, *ow = (W - size) / stride + 1;
    return MREFSR_OK;
}

int cx_subsample_geometry(const char *what, int B, int h, int w, int C, int s)
{
    MREFSR_REQUIRE(B >= 1 && h >= 1 && w >= 1 && C >= 4 && C % 4 == 0 && s >= 1, "%s: B=%d h=%d w=%d C=%d (a multiple of 4) s=%d", what, B, h,
                   w, C, s);
    MREFSR_REQUIRE((int64_t)B * h * w * C < ((int64_t)1 << 33), "%s: a tap of %d x %d x %d x %d", what, B, h, w, C);
    return MREFSR_OK;
}

}  // namespace

MREFSR_EXPORT int64_t mrefsr_contextual_workspace_bytes(int B, int N, int C, int backward)
{
    if (B < 1 || B > 65535 || N < 2 || C <= 0) return MREFSR_E_INVALID;
    if (!cx_shape_ok(B, N, C)) return MREFSR_E_UNSUPPORTED;
    return backward ? cx_off_dxn(B, N, C) + align256((int64_t)B * N * C * 4) : cx_off_dxn(B, N, C);
}

MREFSR_EXPORT int mrefsr_contextual_fwd_f32(const float *x, const float *y, int B, int N, int C, float band_width, float *xn, float *yn,
                                            float *rnorm, float *rowf, int32_t *jmin, float *cxmax, int32_t *imax, float *cx, float *tap_loss,
                                            float weight, float loss_weight, int first, float *run, float *total, void *workspace,
                                            int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && y && xn && yn && rnorm && rowf && jmin && cxmax && imax && cx && tap_loss && run && total && workspace,
                   "contextual_fwd: null pointer");
    CX_REQUIRE_SHAPE("contextual_fwd");
    return cx_forward("contextual_fwd", x, y, B, N, C, band_width, CxSpatial{0, 0, 0.f}, xn, yn, rnorm, rowf, jmin, cxmax, imax, cx, tap_loss,
                      weight, loss_weight, first, run, total, workspace, workspace_bytes, stream);
}

MREFSR_EXPORT int mrefsr_contextual_bwd_f32(const float *xn, const float *yn, const float *rnorm, int B, int N, int C, float band_width,
                                            const float *rowf, const int32_t *jmin, const float *cxmax, const int32_t *imax, const float *cx,
                                            const float *gup, float coef, float *dx, int accumulate, float *amax, void *workspace,
                                            int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(xn && yn && rnorm && rowf && jmin && cxmax && imax && cx && dx && workspace, "contextual_bwd: null pointer");
    CX_REQUIRE_SHAPE("contextual_bwd");
    return cx_backward("contextual_bwd", xn, yn, rnorm, B, N, C, band_width, CxSpatial{0, 0, 0.f}, rowf, jmin, cxmax, imax, cx, gup, coef, dx,
                       accumulate, amax, workspace, workspace_bytes, stream);
}

MREFSR_EXPORT int mrefsr_contextual_fwd_sp_f32(const float *x, const float *y, int B, int h, int w, int C, float band_width, float weight_sp,
                                               float *xn, float *yn, float *rnorm, float *rowf, int32_t *jmin, float *cxmax, int32_t *imax,
                                               float *cx, float *tap_loss, float weight, float loss_weight, int first, float *run, float *total,
                                               void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && y && xn && yn && rnorm && rowf && jmin && cxmax && imax && cx && tap_loss && run && total && workspace,
                   "contextual_fwd_sp: null pointer");
    CX_REQUIRE_GRID("contextual_fwd_sp");
    const int N = h * w;
    CX_REQUIRE_SHAPE("contextual_fwd_sp");
    return cx_forward("contextual_fwd_sp", x, y, B, N, C, band_width, CxSpatial{h, w, weight_sp}, xn, yn, rnorm, rowf, jmin, cxmax, imax, cx,
                      tap_loss, weight, loss_weight, first, run, total, workspace, workspace_bytes, stream);
}

MREFSR_EXPORT int mrefsr_contextual_bwd_sp_f32(const float *xn, const float *yn, const float *rnorm, int B, int h, int w, int C,
                                               float band_width, float weight_sp, const float *rowf, const int32_t *jmin, const float *cxmax,
                                               const int32_t *imax, const float *cx, const float *gup, float coef, float *dx, int accumulate,
                                               float *amax, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(xn && yn && rnorm && rowf && jmin && cxmax && imax && cx && dx && workspace, "contextual_bwd_sp: null pointer");
    CX_REQUIRE_GRID("contextual_bwd_sp");
    const int N = h * w;
    CX_REQUIRE_SHAPE("contextual_bwd_sp");
    return cx_backward("contextual_bwd_sp", xn, yn, rnorm, B, N, C, band_width, CxSpatial{h, w, weight_sp}, rowf, jmin, cxmax, imax, cx, gup,
                       coef, dx, accumulate, amax, workspace, workspace_bytes, stream);
}

MREFSR_EXPORT int mrefsr_cx_patch_channels(int size)
{
    if (size < 1) return MREFSR_E_INVALID;
    return size > 13 ? MREFSR_E_UNSUPPORTED : cx_patch_channels(size);
}

MREFSR_EXPORT int mrefsr_cx_patches_f32(const float *img, int B, int H, int W, int size, int stride, int norm, float *out, int Cpad,
                                        mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(img && out, "cx_patches: null pointer");
    int oh, ow;
    if (const int e = cx_patch_geometry("cx_patches", B, H, W, size, stride, Cpad, &oh, &ow)) return e;
    MREFSR_REQUIRE(reinterpret_cast<uintptr_t>(out) % 16 == 0, "cx_patches: out must be 16-byte aligned");
    const long total4 = (long)B * oh * ow * (Cpad / 4);
    hipLaunchKernelGGL(cx_patches_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, out, total4, H, W, size,
                       stride, oh, ow, Cpad, norm ? 1 : 0);
    return mrefsr::check_launch("cx_patches");
}

MREFSR_EXPORT int mrefsr_cx_patches_bwd_f32(const float *g, int B, int H, int W, int size, int stride, int Cpad, float scale, float *dimg,
                                            int accumulate, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(g && dimg, "cx_patches_bwd: null pointer");
    int oh, ow;
    if (const int e = cx_patch_geometry("cx_patches_bwd", B, H, W, size, stride, Cpad, &oh, &ow)) return e;
    const long total = (long)B * 3 * H * W;
    hipLaunchKernelGGL(cx_patches_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, dimg, total, H, W, size,
                       stride, oh, ow, Cpad, scale, accumulate ? 1 : 0);
    return mrefsr::check_launch("cx_patches_bwd");
}

MREFSR_EXPORT int mrefsr_cx_subsample_f32(const float *f, int B, int h, int w, int C, int s, float *out, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(f && out, "cx_subsample: null pointer");
    if (const int e = cx_subsample_geometry("cx_subsample", B, h, w, C, s)) return e;
    MREFSR_REQUIRE((reinterpret_cast<uintptr_t>(f) | reinterpret_cast<uintptr_t>(out)) % 16 == 0, "cx_subsample: pointers must be 16-byte aligned");
    const int hs = (h + s - 1) / s, ws = (w + s - 1) / s;
    const long total4 = (long)B * hs * ws * (C / 4);
    hipLaunchKernelGGL(cx_subsample_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f, out, total4, h, w, C / 4,
                       s, hs, ws);
    return mrefsr::check_launch("cx_subsample");
}

MREFSR_EXPORT int mrefsr_cx_subsample_bwd_f32(const float *gs, int B, int h, int w, int C, int s, float *g, int accumulate, float *amax,
                                              mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(gs && g, "cx_subsample_bwd: null pointer");
    if (const int e = cx_subsample_geometry("cx_subsample_bwd", B, h, w, C, s)) return e;
    MREFSR_REQUIRE((reinterpret_cast<uintptr_t>(gs) | reinterpret_cast<uintptr_t>(g)) % 16 == 0,
                   "cx_subsample_bwd: pointers must be 16-byte aligned");
    const int hs = (h + s - 1) / s, ws = (w + s - 1) / s;
    const long total4 = (long)B * h * w * (C / 4);
    hipLaunchKernelGGL(cx_subsample_bwd_kernel, dim3((unsigned)((total4 + 256 * CX_SUB_ITEMS - 1) / (256 * CX_SUB_ITEMS))), dim3(256), 0, (hipStream_t)stream, gs, g, total4, h, w,
                       C / 4, s, hs, ws, accumulate ? 1 : 0, reinterpret_cast<unsigned int *>(amax));
    return mrefsr::check_launch("cx_subsample_bwd");
}
