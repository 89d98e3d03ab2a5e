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
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

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

// one wave per position: rows [0, BN) are x, rows [BN, 2 BN) are y.  C <= 512: at most two float4 per lane
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
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int k = lane + 64 * q;
        v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < C4) {
            const float4 a = src[k], u = m4[k];
            v[q] = make_float4(a.x - u.x, a.y - u.y, a.z - u.z, a.w - u.w);
            ss += v[q].x * v[q].x + v[q].y * v[q].y + v[q].z * v[q].z + v[q].w * v[q].w;
        }
    }
    ss = __shfl(mrefsr::wave_sum(ss), 0, 64);
    const float den = fmaxf(sqrtf(ss), CX_NORM_FLOOR);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int k = lane + 64 * q;
        if (k < C4) dst[k] = make_float4(v[q].x / den, v[q].y / den, v[q].z / den, v[q].w / den);
    }
    if (is_x && lane == 0) rnorm[r] = 1.0f / den;
}

// ---------------------------------------------------------------------------------------------------------------
// d = 1 - xn yn^T on the f32 matrix pipe.  Block = 4 waves = one 64 x 64 tile of d[b]; wave w: the 32 x 32 quarter (w >> 1, w & 1),
// 2 x 2 accumulators.  A[m][k] = xn[i0 + m][c], B[k][n] = yn[j0 + n][c]: a lane holds a float4 of row (l & 15), channels
// k0 + 4 (l >> 4) .. + 3 of both maps and feeds element e to the e-th MFMA of the 16-channel step, so the MFMA's local k = l >> 4 is
// channel k0 + 4 (l >> 4) + e on both sides (gram_bwd_kernel's operand trick).  Rows past N load zeros and are not stored.
// D: column (j) = lane & 15, row (i) = 4 (lane >> 4) + r.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cx_dist_kernel(const float *__restrict__ xn, const float *__restrict__ yn, float *__restrict__ d, int N,
                                                      int C, int ld)
{
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
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[a][q] = f32x4{0.f, 0.f, 0.f, 0.f};
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
                for (int q = 0; q < 2; ++q) acc[a][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ae[a][e], be[q][e], acc[a][q], 0, 0, 0);
    }
    float *db = d + (long)b * N * ld;
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
                amx = fmaxf(amx, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
            }
        }
    }
    if (amax_bits) mrefsr::publish_amax<true>(amax_bits, amx);   // (one wave per position: thousands of waves on one word)
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
        MREFSR_REQUIRE(B >= 1 && B <= 65535 && N >= 2 && C > 0, what ": B=%d N=%d C=%d (1 <= B <= 65535, N >= 2)", B, N, C);          \
        if (!cx_shape_ok(B, N, C))                                                                                                   \
            return mrefsr::fail(MREFSR_E_UNSUPPORTED, what ": N=%d C=%d (N <= %d: one N x N matrix per sample is materialised; C of " \
                                "64, 128, 256, 512)", N, C, MREFSR_CX_MAX_N);                                                         \
    } while (0)

void launch_dist(const float *xn, const float *yn, float *d, int B, int N, int C, hipStream_t st)
{
    const int T = (N + 63) / 64;
    hipLaunchKernelGGL(cx_dist_kernel, dim3(T, T, B), dim3(256), 0, st, xn, yn, d, N, C, cx_ld(N));
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
    MREFSR_REQUIRE(band_width > 0.f && band_width < INFINITY, "contextual_fwd: band_width=%g (a finite number > 0)", (double)band_width);
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_contextual_workspace_bytes(B, N, C, 0), "contextual_fwd: workspace of %ld bytes < %ld",
                   (long)workspace_bytes, (long)mrefsr_contextual_workspace_bytes(B, N, C, 0));
    MREFSR_REQUIRE((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(xn) |
                    reinterpret_cast<uintptr_t>(yn) | reinterpret_cast<uintptr_t>(workspace)) % 16 == 0,
                   "contextual_fwd: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long BN = (long)B * N;
    const int ld = cx_ld(N);
    float *mu = (float *)workspace, *d = (float *)((char *)workspace + cx_off_d(B, C));
    hipLaunchKernelGGL(cx_mean_kernel, dim3(C / 16, B), dim3(1024), 0, st, y, mu, N, C);
    hipLaunchKernelGGL(cx_normalise_kernel, dim3((unsigned)((2 * BN + 3) / 4)), dim3(256), 0, st, x, y, (const float *)mu, xn, yn, rnorm, BN, N, C);
    launch_dist(xn, yn, d, B, N, C, st);
    hipLaunchKernelGGL(cx_row_kernel, dim3((unsigned)((BN + 3) / 4)), dim3(256), 0, st, (const float *)d, rowf, jmin, BN, N, ld, band_width);
    hipLaunchKernelGGL(cx_col_kernel, dim3((N + 31) / 32, B), dim3(1024), 0, st, (const float *)d, (const float *)rowf, cxmax, imax, BN, N, ld,
                       band_width);
    hipLaunchKernelGGL(cx_finish_kernel, dim3(1), dim3(256), 0, st, (const float *)cxmax, cx, tap_loss, run, total, B, N, weight, loss_weight,
                       first ? 1 : 0);
    return mrefsr::check_launch("contextual_fwd");
}

MREFSR_EXPORT int mrefsr_contextual_bwd_f32(const float *xn, const float *yn, const float *rnorm, int B, int N, int C, float band_width,
                                            const float *rowf, const int32_t *jmin, const float *cxmax, const int32_t *imax, const float *cx,
                                            const float *gup, float coef, float *dx, int accumulate, float *amax, void *workspace,
                                            int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(xn && yn && rnorm && rowf && jmin && cxmax && imax && cx && dx && workspace, "contextual_bwd: null pointer");
    CX_REQUIRE_SHAPE("contextual_bwd");
    MREFSR_REQUIRE(band_width > 0.f && band_width < INFINITY, "contextual_bwd: band_width=%g (a finite number > 0)", (double)band_width);
    MREFSR_REQUIRE(workspace_bytes >= mrefsr_contextual_workspace_bytes(B, N, C, 1), "contextual_bwd: workspace of %ld bytes < %ld",
                   (long)workspace_bytes, (long)mrefsr_contextual_workspace_bytes(B, N, C, 1));
    MREFSR_REQUIRE((reinterpret_cast<uintptr_t>(xn) | reinterpret_cast<uintptr_t>(yn) | reinterpret_cast<uintptr_t>(dx) |
                    reinterpret_cast<uintptr_t>(workspace)) % 16 == 0,
                   "contextual_bwd: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long BN = (long)B * N;
    const int ld = cx_ld(N);
    float *d = (float *)((char *)workspace + cx_off_d(B, C)), *dxn = (float *)((char *)workspace + cx_off_dxn(B, N, C));
    launch_dist(xn, yn, d, B, N, C, st);
    hipLaunchKernelGGL(cx_rowgrad_kernel, dim3((unsigned)BN), dim3(256), 0, st, d, rowf, jmin, cxmax, imax, cx, gup, coef, BN, B, N, ld,
                       band_width);
    hipLaunchKernelGGL(cx_grad_gemm_kernel, dim3((N + 63) / 64, C / 64, B), dim3(256), 0, st, (const float *)d, yn, dxn, N, C, ld);
    hipLaunchKernelGGL(cx_grad_finish_kernel, dim3((unsigned)((BN + 3) / 4)), dim3(256), 0, st, (const float *)dxn, xn, rnorm, dx, BN, C,
                       accumulate ? 1 : 0, reinterpret_cast<unsigned int *>(amax));
    return mrefsr::check_launch("contextual_bwd");
}
