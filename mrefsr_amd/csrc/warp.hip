// Homography views of image batches and the matcher's score against a known homography (mrefsr_amd/views.py; train.ref_augment,
// val.ref_perturb, val.match_probe).  No counterpart on the device in the reference: its view generator is cv2.warpPerspective on
// the host (image_pair_generation_perspective of ref_cufed_dataset.py / ref_megadepth_dataset.py).
//
// warp_persp: y[n][c][yo][xo] = interpolate(x[n][c], sx, sy) with (u, v, t) = S_n (xo, yo, 1), sx = u / t, sy = v / t -- S is the
// SAMPLING matrix, destination -> source, in integer pixel coordinates (pixel (x, y) is at (x, y)): cv2.warpPerspective's
// dst(x, y) = src(M^-1 (x, y, 1)) with S = M^-1.  The order of operations, all of it spelled out below (-ffp-contract=off, Makefile):
//   coordinates in double:  u = (S0 xo + S1 yo) + S2, likewise v and t; sx = u / t; fx = floor(sx); the fraction sx - fx is
//     rounded ONCE to fp32 (it may round to 1.0f: the weights below are then exactly those of the next pixel);
//   weights in fp32 from the fraction a, s = 1 - a (cubic convolution, A = -0.75, the kernel of OpenCV and torch.grid_sample):
//     w0 = ((-0.75 a) s) s        w1 = ((1.25 a - 2.25) a) a + 1        w2 = ((1.25 s - 2.25) s) s + 1        w3 = ((-0.75 a) a) s
//     (w1, w2: torch's Horner form; w0, w3: the factored form of the outer lobes, five roundings instead of Horner's
//     cancellation at 3).  a = 0 gives exactly [-0, 1, 0, -0], a = 1 exactly [-0, 0, 1, -0]; bilinear: [s, a];
//   the separable sum in fp32: per row  r_j = ((w0 v_j0 + w1 v_j1) + w2 v_j2) + w3 v_j3  along x, then the same chain over the
//     rows with the y weights; every product rounded before its add.  Taps outside the image are 0 (constant border).
// So, for finite inputs: the identity returns the input's bits (-0 comes back as +0), an integer translation returns shifted bits
// and exact zeros, a zero image stays zero.  The output is exactly 0 where t is not > 0, where a coordinate is not finite, and
// where no tap is inside the image.  |y - exact| <= 70 * 2^-24 * max |x| (bilinear: 7; DESIGN 3.24 counts the roundings).
//
// One thread per output pixel of a 32 x 8 tile; the coordinate, the taps' addresses and the weights are computed once and serve all
// C channels.  The grid is (tiles across, tiles down, N): the image, and with it S_n, is uniform per block.  No atomics, no readback.
//
// match_stats: the top-1 matcher's indices against the homography M_n that maps a query position to its true reference position in
// feature coordinates: per n the number of counted queries, the sum of their end-point errors and, per threshold, the number of
// them with an error <= the threshold.  Everything in double; one block per n, block_sum (reduce.h: the fixed halving tree).
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int TILE_X = 32, TILE_Y = 8;
constexpr int MAX_THR = 4;

// TAPS = 4: cubic convolution, taps ix - 1 .. ix + 2; TAPS = 2: bilinear, taps ix, ix + 1
template <int TAPS> __device__ __forceinline__ void weights_of(const float a, float *w)
{
    const float s = 1.0f - a;
    if (TAPS == 2) {
        w[0] = s;
        w[1] = a;
        return;
    }
    w[0] = ((-0.75f * a) * s) * s;
    w[1] = ((1.25f * a - 2.25f) * a) * a + 1.0f;
    w[2] = ((1.25f * s - 2.25f) * s) * s + 1.0f;
    w[3] = ((-0.75f * a) * a) * s;
}

template <int TAPS>
__global__ __launch_bounds__(THREADS) void warp_persp_kernel(const float *__restrict__ x, const double *__restrict__ S,
                                                             float *__restrict__ y, const int C, const int H, const int W,
                                                             const int Ho, const int Wo, const int clamp01)
{
    constexpr int FIRST = TAPS == 4 ? -1 : 0;
    const int n = (int)blockIdx.z;
    const int xo = (int)blockIdx.x * TILE_X + (int)(threadIdx.x & (TILE_X - 1));
    const int yo = (int)blockIdx.y * TILE_Y + (int)(threadIdx.x / TILE_X);
    if (xo >= Wo || yo >= Ho) return;
    const double *const s = S + 9 * (long long)n;
    const double dx = (double)xo, dy = (double)yo;
    const double u = (s[0] * dx + s[1] * dy) + s[2];
    const double v = (s[3] * dx + s[4] * dy) + s[5];
    const double t = (s[6] * dx + s[7] * dy) + s[8];
    const long long plane_in = (long long)H * W, plane_out = (long long)Ho * Wo;
    float *const out = y + (long long)n * C * plane_out + (long long)yo * Wo + xo;
    const double sx = u / t, sy = v / t;
    const double fx = floor(sx), fy = floor(sy);
    // a tap inside the image: FIRST + TAPS - 1 + fx >= 0 and FIRST + fx <= W - 1 (false for NaN and the infinities as well)
    const bool seen = t > 0.0 && fx >= (double)(1 - TAPS - FIRST) && fx <= (double)(W - 1 - FIRST) && fy >= (double)(1 - TAPS - FIRST) &&
                      fy <= (double)(H - 1 - FIRST);
    if (!seen) {
        for (int c = 0; c < C; ++c) out[c * plane_out] = 0.0f;
        return;
    }
    const int ix = (int)fx, iy = (int)fy;
    float wx[TAPS], wy[TAPS];
    weights_of<TAPS>((float)(sx - fx), wx);
    weights_of<TAPS>((float)(sy - fy), wy);
    int col[TAPS], row[TAPS];   // clamped into the image: every load below is inside the plane
    bool okx[TAPS], oky[TAPS];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
        const int cx = ix + FIRST + k, cy = iy + FIRST + k;
        okx[k] = cx >= 0 && cx < W;
        oky[k] = cy >= 0 && cy < H;
        col[k] = min(max(cx, 0), W - 1);
        row[k] = min(max(cy, 0), H - 1) * W;
    }
    const float *src = x + (long long)n * C * plane_in;
    for (int c = 0; c < C; ++c, src += plane_in) {
        float r[TAPS];
#pragma unroll
        for (int j = 0; j < TAPS; ++j) {
            float p[TAPS];
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                const float val = src[row[j] + col[k]];
                p[k] = wx[k] * (okx[k] && oky[j] ? val : 0.0f);
            }
            float acc = p[0] + p[1];
#pragma unroll
            for (int k = 2; k < TAPS; ++k) acc = acc + p[k];
            r[j] = acc;
        }
        float acc = wy[0] * r[0] + wy[1] * r[1];
#pragma unroll
        for (int j = 2; j < TAPS; ++j) acc = acc + wy[j] * r[j];
        if (clamp01) acc = fminf(fmaxf(acc, 0.0f), 1.0f);
        out[c * plane_out] = acc;
    }
}

struct Thresholds {
    double v[MAX_THR];
};

// max_idx [N][h-2][w-2]; M [N][9]; stats [N][2 + T]
__global__ __launch_bounds__(THREADS) void match_stats_kernel(const int64_t *__restrict__ max_idx, const double *__restrict__ M,
                                                              const Thresholds thr, double *__restrict__ stats, const int h, const int w,
                                                              const int y_hi, const int x_hi, const int margin, const int T)
{
    __shared__ double red[THREADS];
    const int n = blockIdx.x, pw = w - 2, total = (h - 2) * pw;
    const double *const m = M + 9 * (long long)n;
    const int64_t *const idx = max_idx + (long long)n * total;
    const double lo = (double)margin, xh = (double)(x_hi - margin), yh = (double)(y_hi - margin);
    double cnt = 0.0, err = 0.0, hit[MAX_THR] = {0.0, 0.0, 0.0, 0.0};
    for (int q = threadIdx.x; q < total; q += THREADS) {
        const int qy = q / pw, qx = q % pw;
        const double cx = (double)(qx + 1), cy = (double)(qy + 1);   // the centre of the 3 x 3 query patch
        const double U = (m[0] * cx + m[1] * cy) + m[2];
        const double V = (m[3] * cx + m[4] * cy) + m[5];
        const double Z = (m[6] * cx + m[7] * cy) + m[8];
        if (!(Z > 0.0)) continue;
        const double tx = U / Z - 1.0, ty = V / Z - 1.0;   // the true top-left of the matching reference patch
        const bool counted = (double)qx >= lo && (double)qx <= xh && (double)qy >= lo && (double)qy <= yh && tx >= lo && tx <= xh &&
                             ty >= lo && ty <= yh;
        if (!counted) continue;
        const int64_t i = idx[q];
        const double ex = (double)(i % pw) - tx, ey = (double)(i / pw) - ty;
        const double e = sqrt(ex * ex + ey * ey);
        cnt += 1.0;
        err += e;
#pragma unroll
        for (int k = 0; k < MAX_THR; ++k)
            if (k < T && e <= thr.v[k]) hit[k] += 1.0;
    }
    cnt = mrefsr::block_sum<THREADS>(red, cnt);
    err = mrefsr::block_sum<THREADS>(red, err);
#pragma unroll
    for (int k = 0; k < MAX_THR; ++k)
        if (k < T) hit[k] = mrefsr::block_sum<THREADS>(red, hit[k]);
    if (threadIdx.x == 0) {
        double *const o = stats + (long long)n * (2 + T);
        o[0] = cnt;
        o[1] = err;
#pragma unroll
        for (int k = 0; k < MAX_THR; ++k)
            if (k < T) o[2 + k] = hit[k];
    }
}

}  // namespace

MREFSR_EXPORT int mrefsr_warp_persp_f32(const float *x, const double *S, float *y, int N, int C, int H, int W, int Ho, int Wo, int interp,
                                        int clamp, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && S && y && (const float *)y != x, "warp_persp: null pointer or y == x (x=%p S=%p y=%p)", (const void *)x,
                   (const void *)S, (const void *)y);
    MREFSR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "warp_persp: N=%d C=%d H=%d W=%d Ho=%d Wo=%d (all positive)", N, C, H,
                   W, Ho, Wo);
    MREFSR_REQUIRE(interp == 0 || interp == 1, "warp_persp: interp=%d (0 bilinear, 1 bicubic)", interp);
    MREFSR_REQUIRE(clamp == 0 || clamp == 1, "warp_persp: clamp=%d (0 or 1)", clamp);
    const int tiles_x = (Wo + TILE_X - 1) / TILE_X, tiles_y = (Ho + TILE_Y - 1) / TILE_Y;
    MREFSR_REQUIRE((long long)H * W <= ((long long)1 << 30) && (long long)Ho * Wo <= ((long long)1 << 30) && tiles_y <= 65535 && N <= 65535,
                   "warp_persp: %d images of %d x %d -> %d x %d (H W, Ho Wo <= 2^30, Ho <= 524280, N <= 65535)", N, H, W, Ho, Wo);
    const dim3 grid((unsigned int)tiles_x, (unsigned int)tiles_y, (unsigned int)N), block(THREADS);
    if (interp == 1)
        hipLaunchKernelGGL(warp_persp_kernel<4>, grid, block, 0, (hipStream_t)stream, x, S, y, C, H, W, Ho, Wo, clamp);
    else
        hipLaunchKernelGGL(warp_persp_kernel<2>, grid, block, 0, (hipStream_t)stream, x, S, y, C, H, W, Ho, Wo, clamp);
    return mrefsr::check_launch("warp_persp");
}

MREFSR_EXPORT int mrefsr_match_stats_f64(const int64_t *max_idx, const double *M, const double *thr, double *stats, int N, int h, int w,
                                         int y_hi, int x_hi, int margin, int T, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(max_idx && M && stats && (thr || T == 0), "match_stats: null pointer (max_idx=%p M=%p thr=%p stats=%p)", (const void *)max_idx,
                   (const void *)M, (const void *)thr, (const void *)stats);
    MREFSR_REQUIRE(N > 0 && h >= 3 && w >= 3 && (long long)(h - 2) * (w - 2) <= ((long long)1 << 30),
                   "match_stats: N=%d h=%d w=%d (N positive, h, w >= 3, (h - 2) (w - 2) <= 2^30)", N, h, w);
    MREFSR_REQUIRE(T >= 0 && T <= MAX_THR, "match_stats: T=%d thresholds (0..%d)", T, MAX_THR);
    MREFSR_REQUIRE(margin >= 0 && y_hi >= 0 && y_hi <= h - 3 && x_hi >= 0 && x_hi <= w - 3,
                   "match_stats: margin=%d (>= 0) y_hi=%d (0..h-3) x_hi=%d (0..w-3)", margin, y_hi, x_hi);
    Thresholds t;
    for (int k = 0; k < MAX_THR; ++k) t.v[k] = k < T ? thr[k] : 0.0;   // (thr is HOST memory: T <= 4 doubles go as a kernel argument)
    hipLaunchKernelGGL(match_stats_kernel, dim3((unsigned int)N), dim3(THREADS), 0, (hipStream_t)stream, max_idx, M, t, stats, h, w, y_hi, x_hi,
                       margin, T);
    return mrefsr::check_launch("match_stats");
}
