// Colour correction of test() outputs towards the LQ image (val.color_fix; the "color fix" of StableSR, Wang et al., IJCV 2024, that
// DiffBIR, SUPIR and others reuse): x the output, s the colour source (the bicubic-upsampled LQ), both [B][C][H][W] fp32, every
// (b, c) plane on its own.  sizes: NULL, or [B][2] int32 (h_b, w_b) in device memory, 1 <= h_b <= H, 1 <= w_b <= W: the top-left
// h_b x w_b rectangle of sample b is the image -- statistics and filters see it alone, its border is the image border, and every
// pixel outside it keeps x's bits.  Neither form clamps its result; the inputs are only read.
//
// wavelet, levels L in 1..5:  out = high_L(x) + low_L(s) = x + low_L(s - x),  low_0(v) = v,  low_i(v) = low_{i-1}(v) filtered with
// [1,2,1]^T [1,2,1] / 16 at dilation r = 2^(i-1), the reads clamped to the rectangle at EVERY stage (replicate padding; not the same
// as one 63-tap kernel with folded indices).  One launch, one block of 512 threads per 64 x 64 tile of a plane.  D = s - x of the tile
// and a halo of HL = 2^L - 1 pixels (31 at L = 5) is staged in LDS, (64 + 2 HL) rows of 64 + 2 ceil4(HL) words (126 x 128 words =
// 63 KB at L = 5: two blocks per CU): the tile's first column sits on a 16-byte boundary of its LDS row, so with 16-byte global
// accesses a quad goes to LDS as one 16-byte write.  Positions outside the rectangle are never read (every read index is clamped in
// image coordinates first) and never staged.  Then the L stages in place, each a pass along x and a pass along y:
//     v' = 0.25f * (a + c) + 0.5f * b          a, c the neighbours at -r, +r (clamped), b the centre
// -- the products are exact, so TWO roundings per pass (a + c, then the sum; -ffp-contract=off, Makefile).  A thread computes its
// elements of a pass (of half a pass where it has more than 16) into registers, the block meets, it writes them back.  In both
// passes the lanes of a wave run along x (consecutive LDS words: no bank conflict by stride; a wave that wraps into the next row of
// a narrower region can meet itself two-way).  Stage i is computed on the tile grown by the later stages' dilations
// (rem_i = HL - (2^i - 1)) only, its pass along x on r more rows each side: 116 k instead of 159 k element updates per tile at
// L = 5.  Last,
//     out = low == 0 ? x : x + low             inside the rectangle (s bit-equal to x gives D = +0 everywhere: x's bits, -0 included)
//     out = x                                  outside it.
// ROUNDINGS: R(L) = 4 L + 1 fp32 roundings lie on the longest path in front of that last add -- the subtraction and 4 per stage --,
// each of a value no larger than max |s - x| (every stage is a convex combination with weights exact in fp32), so
//     |out - exact| <= R(L) 2^-24 max |s - x| + 2^-24 |exact|,        R(5) = 21
// (tests/test_color_fix_kernels_gpu.py carries the same R).
//
// adain:  out = (x - mu_x) (sigma_s / sigma_x) + mu_s,  mu the mean over the rectangle, sigma = sqrt(var + 1e-5) with the unbiased
// variance (calc_mean_std of StableSR); a rectangle of one pixel has none: the binding refuses it on the host.  Two launches.
// Statistics: block (j, plane) takes rows [j RB, (j + 1) RB) of the plane (RB = max(1, 4096 / W)) that lie in the rectangle; in
// double, two passes: the block's sum -> its mean, then the squares about that mean -> its M2, for x and for s, each by the halving
// tree of reduce.h; (count, mean_x, M2_x, mean_s, M2_s) go to the block's row of the workspace.  The block that draws the last
// ticket merges: thread t takes planes t, t + 256, ...; per plane, in ascending block order and two passes again,
//     mean = sum n_j mean_j / N,   M2 = sum M2_j + n_j (mean_j - mean)^2,   sigma = sqrt(M2 / (N - 1) + 1e-5)
// and writes (mu_x, sigma_s / sigma_x, mu_s) in double behind the partials.  Apply:  out = fl32(((double)x - mu_x) a + mu_s), the
// product rounded before the add in double, ONE rounding to fp32; outside the rectangle x's bits.  No float atomics, no readback, a
// ticket that resets itself, the same bits from call to call.
//
// Both kernels: 16-byte global accesses when the three pointers are 16-byte aligned and W % 4 == 0 (every row then starts on a
// 16-byte boundary), 4-byte accesses otherwise; the same arithmetic either way.
#include <math.h>

#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
// device-memory addresses: said so, they are accessed with global_* instead of flat_* instructions
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

constexpr int TILE = 64;
constexpr int WAVELET_THREADS = 512;

// the valid rectangle of sample b, clamped into the plane whatever the table says: no index below leaves the buffers
__device__ __forceinline__ void valid_rect(const int *__restrict__ sizes, const long long b, const int H, const int W, int &h, int &w)
{
    h = H, w = W;
    if (sizes) {
        h = min(max(sizes[2 * b], 1), H);
        w = min(max(sizes[2 * b + 1], 1), W);
    }
}

template <int L> struct Geo {
    static constexpr int HL = (1 << L) - 1;          // halo
    static constexpr int XO = (HL + 3) / 4 * 4;      // LDS column of the tile's first column
    static constexpr int ROWS = TILE + 2 * HL;
    static constexpr int PITCH = TILE + 2 * XO;      // words per LDS row
};

// One pass of one stage, in place: positions rows [R0, R0 + NR) x columns [C0, C0 + NC) of the LDS image (LDS coordinates; image
// coordinates = LDS coordinates + (iy0, ix0)) that lie inside the h x w rectangle get 0.25 (a + c) + 0.5 b, a and c at distance
// DIL along x (ALONG_X) or y with the index clamped into the rectangle.  The clamped index stays inside the region the pass before
// computed: that region is this one grown by DIL along the axis, and clamping moves an index towards the centre.
template <int PITCH, int R0, int NR, int C0, int NC, int DIL, bool ALONG_X>
__device__ __forceinline__ void filter_chunk(float *t, const int tid, const int iy0, const int ix0, const int h, const int w)
{
    constexpr int N = NR * NC, K = (N + WAVELET_THREADS - 1) / WAVELET_THREADS;
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int idx = tid + k * WAVELET_THREADS;
        const int ly = R0 + idx / NC, lx = C0 + idx % NC;
        const int gy = iy0 + ly, gx = ix0 + lx;
        v[k] = 0.f;
        if (idx < N && gy >= 0 && gy < h && gx >= 0 && gx < w) {
            float a, c;
            if (ALONG_X) {
                a = t[ly * PITCH + (max(gx - DIL, 0) - ix0)];
                c = t[ly * PITCH + (min(gx + DIL, w - 1) - ix0)];
            } else {
                a = t[(max(gy - DIL, 0) - iy0) * PITCH + lx];
                c = t[(min(gy + DIL, h - 1) - iy0) * PITCH + lx];
            }
            v[k] = 0.25f * (a + c) + 0.5f * t[ly * PITCH + lx];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int idx = tid + k * WAVELET_THREADS;
        const int ly = R0 + idx / NC, lx = C0 + idx % NC;
        const int gy = iy0 + ly, gx = ix0 + lx;
        if (idx < N && gy >= 0 && gy < h && gx >= 0 && gx < w) t[ly * PITCH + lx] = v[k];
    }
}

// A pass in chunks of at most CHUNK_ITEMS elements per thread (the registers a thread holds between the two halves of a chunk):
// rows of a pass along x, columns of a pass along y do not depend on each other, so a chunk of them is read, met on and written
// while the next chunk's reads may already run; one more barrier closes the pass.
constexpr int CHUNK_ITEMS = 16;

template <int PITCH, int R0, int NR, int C0, int NC, int DIL, bool ALONG_X>
__device__ __forceinline__ void filter_pass(float *t, const int tid, const int iy0, const int ix0, const int h, const int w)
{
    constexpr int PER = CHUNK_ITEMS * WAVELET_THREADS;
    constexpr int NCH = (NR * NC + PER - 1) / PER;
    if constexpr (NCH <= 1) {
        filter_chunk<PITCH, R0, NR, C0, NC, DIL, ALONG_X>(t, tid, iy0, ix0, h, w);
        __syncthreads();
    } else if constexpr (ALONG_X) {
        constexpr int RC = (NR + NCH - 1) / NCH;
        filter_chunk<PITCH, R0, RC, C0, NC, DIL, true>(t, tid, iy0, ix0, h, w);
        filter_pass<PITCH, R0 + RC, NR - RC, C0, NC, DIL, true>(t, tid, iy0, ix0, h, w);
    } else {
        constexpr int CC = (NC + NCH - 1) / NCH;
        filter_chunk<PITCH, R0, NR, C0, CC, DIL, false>(t, tid, iy0, ix0, h, w);
        filter_pass<PITCH, R0, NR, C0 + CC, NC - CC, DIL, false>(t, tid, iy0, ix0, h, w);
    }
}

// stage I of L (dilation 2^(I-1)) and the stages behind it
template <int L, int I>
__device__ __forceinline__ void stages(float *t, const int tid, const int iy0, const int ix0, const int h, const int w)
{
    if constexpr (I <= L) {
        typedef Geo<L> G;
        constexpr int DIL = 1 << (I - 1);
        constexpr int REM = G::HL - ((1 << I) - 1);   // the later stages' dilations
        filter_pass<G::PITCH, G::HL - REM - DIL, TILE + 2 * (REM + DIL), G::XO - REM, TILE + 2 * REM, DIL, true>(t, tid, iy0, ix0, h, w);
        filter_pass<G::PITCH, G::HL - REM, TILE + 2 * REM, G::XO - REM, TILE + 2 * REM, DIL, false>(t, tid, iy0, ix0, h, w);
        stages<L, I + 1>(t, tid, iy0, ix0, h, w);
    }
}

// blockIdx.x = (plane * tiles_y + tile_y) * tiles_x + tile_x.  Four waves per SIMD (128 VGPRs): the two blocks per CU that the LDS admits
template <int L, bool VEC>
__global__ __launch_bounds__(WAVELET_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void color_fix_wavelet_kernel(const float *__restrict__ x_, const float *__restrict__ s_,
                                                                            float *__restrict__ out_, const int C, const int H, const int W,
                                                                            const int *__restrict__ sizes)
{
    typedef Geo<L> G;
    __shared__ __attribute__((aligned(16))) float t[G::ROWS * G::PITCH];
    const int tid = threadIdx.x;
    const int tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE;
    const unsigned int blk = blockIdx.x;
    const int x0 = (int)(blk % tiles_x) * TILE, y0 = (int)((blk / tiles_x) % tiles_y) * TILE;
    const long long plane = blk / tiles_x / tiles_y;
    const long long hw = (long long)H * W;
    const gf32 *const x = (const gf32 *)x_ + plane * hw;
    const gf32 *const s = (const gf32 *)s_ + plane * hw;
    gf32 *const out = (gf32 *)out_ + plane * hw;
    int h, w;
    valid_rect(sizes, plane / C, H, W, h, w);
    const bool filtered = y0 < h && x0 < w;   // (the whole block alike) else the tile lies outside the rectangle: a copy of x
    const int iy0 = y0 - G::HL, ix0 = x0 - G::XO;   // image coordinates of LDS position (0, 0)

    if (filtered) {
        if (VEC) {
            constexpr int QUADS = G::PITCH / 4;
            for (int idx = tid; idx < G::ROWS * QUADS; idx += WAVELET_THREADS) {
                const int ly = idx / QUADS, lx = 4 * (idx % QUADS);
                const int gy = iy0 + ly, gx = ix0 + lx;
                // (gx and W are multiples of 4: a quad that starts inside the rectangle ends inside the row)
                if (gy < 0 || gy >= h || gx < 0 || gx >= w) continue;
                const f32x4 xv = *(const gf32x4 *)(x + (long long)gy * W + gx), sv = *(const gf32x4 *)(s + (long long)gy * W + gx);
                *(f32x4 *)(t + ly * G::PITCH + lx) = sv - xv;
            }
        } else {
            for (int idx = tid; idx < G::ROWS * G::PITCH; idx += WAVELET_THREADS) {
                const int ly = idx / G::PITCH, lx = idx % G::PITCH;
                const int gy = iy0 + ly, gx = ix0 + lx;
                if (gy < 0 || gy >= h || gx < 0 || gx >= w) continue;
                t[idx] = s[(long long)gy * W + gx] - x[(long long)gy * W + gx];
            }
        }
        __syncthreads();
        stages<L, 1>(t, tid, iy0, ix0, h, w);
    }

    if (VEC) {
        for (int idx = tid; idx < TILE * TILE / 4; idx += WAVELET_THREADS) {
            const int r = idx / (TILE / 4), c = 4 * (idx % (TILE / 4));
            const int gy = y0 + r, gx = x0 + c;
            if (gy >= H || gx >= W) continue;
            f32x4 v = *(const gf32x4 *)(x + (long long)gy * W + gx);
            if (filtered && gy < h) {
                const f32x4 low = *(const f32x4 *)(t + (G::HL + r) * G::PITCH + G::XO + c);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (gx + e < w && low[e] != 0.f) v[e] = v[e] + low[e];
            }
            *(gf32x4 *)(out + (long long)gy * W + gx) = v;
        }
    } else {
        for (int idx = tid; idx < TILE * TILE; idx += WAVELET_THREADS) {
            const int r = idx / TILE, c = idx % TILE;
            const int gy = y0 + r, gx = x0 + c;
            if (gy >= H || gx >= W) continue;
            float v = x[(long long)gy * W + gx];
            if (filtered && gy < h && gx < w) {
                const float low = t[(G::HL + r) * G::PITCH + G::XO + c];
                if (low != 0.f) v = v + low;
            }
            out[(long long)gy * W + gx] = v;
        }
    }
}

// ---- adain ------------------------------------------------------------------------------------------------------------------
constexpr int THREADS = 256;
constexpr int PART = 5;              // doubles per block: count, mean_x, M2_x, mean_s, M2_s
constexpr int STAT = 3;              // doubles per plane: mu_x, sigma_s / sigma_x, mu_s
constexpr int ROWS_ELEMS = 4096;     // elements of a block's rows, about
constexpr double EPS = 1e-5;
constexpr int INFLIGHT = 8;           // block rows of the workspace a merging thread loads before it adds them

__host__ __device__ inline int rows_per_block(const int W) { return W >= ROWS_ELEMS ? 1 : ROWS_ELEMS / W; }

__device__ __forceinline__ double load_partial(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// grid (blocks per plane, planes).  ws: [planes * gridDim.x][PART] partials, then [planes][STAT]
__global__ __launch_bounds__(THREADS) void color_fix_adain_stats_kernel(const float *__restrict__ x_, const float *__restrict__ s_, const int C,
                                                                        const int H, const int W, const int *__restrict__ sizes, double *ws,
                                                                        unsigned int *ticket)
{
    __shared__ double red[THREADS];
    __shared__ int last;
    const int tid = threadIdx.x;
    const long long plane = blockIdx.y, hw = (long long)H * W;
    const unsigned int per_plane = gridDim.x, nblocks = gridDim.x * gridDim.y;
    const float *const x = x_ + plane * hw, *const s = s_ + plane * hw;
    int h, w;
    valid_rect(sizes, plane / C, H, W, h, w);
    const int rb = rows_per_block(W);
    const int ya = min((int)blockIdx.x * rb, h), yb = min(ya + rb, h);
    const int n = (yb - ya) * w;     // <= 4096 + W elements; 0 for a block below the rectangle

    double sx = 0.0, ss = 0.0;
    for (int i = tid; i < n; i += THREADS) {
        const long long o = (long long)(ya + i / w) * W + i % w;
        sx += (double)x[o];
        ss += (double)s[o];
    }
    const double inv = n > 0 ? 1.0 / (double)n : 0.0;
    const double mx = mrefsr::block_sum<THREADS>(red, sx) * inv, ms = mrefsr::block_sum<THREADS>(red, ss) * inv;
    double qx = 0.0, qs = 0.0;
    for (int i = tid; i < n; i += THREADS) {
        const long long o = (long long)(ya + i / w) * W + i % w;
        const double dx = (double)x[o] - mx, ds = (double)s[o] - ms;
        qx += dx * dx;
        qs += ds * ds;
    }
    qx = mrefsr::block_sum<THREADS>(red, qx);
    qs = mrefsr::block_sum<THREADS>(red, qs);
    if (tid == 0) {
        double *row = ws + PART * ((long long)plane * per_plane + blockIdx.x);
        mrefsr::store_partial(row, (double)n);
        mrefsr::store_partial(row + 1, mx);
        mrefsr::store_partial(row + 2, qx);
        mrefsr::store_partial(row + 3, ms);
        mrefsr::store_partial(row + 4, qs);
    }
    if (!mrefsr::last_block_by_ticket(ticket, nblocks, &last)) return;

    double *const stats = ws + (long long)PART * nblocks;
    for (int p = tid; p < (int)gridDim.y; p += THREADS) {
        const double *rows = ws + (long long)PART * p * per_plane;
        // INFLIGHT rows loaded at a time and added in ascending block order (rows past the plane's last: count 0, nothing added)
        double cnt = 0.0, mean_x = 0.0, mean_s = 0.0;
        for (unsigned int j0 = 0; j0 < per_plane; j0 += INFLIGHT) {
            double nj[INFLIGHT], mxj[INFLIGHT], msj[INFLIGHT];
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                const bool in = j0 + u < per_plane;
                nj[u] = in ? load_partial(rows + PART * (j0 + u)) : 0.0;
                mxj[u] = in ? load_partial(rows + PART * (j0 + u) + 1) : 0.0;
                msj[u] = in ? load_partial(rows + PART * (j0 + u) + 3) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                cnt += nj[u];
                mean_x += nj[u] * mxj[u];
                mean_s += nj[u] * msj[u];
            }
        }
        mean_x /= cnt;
        mean_s /= cnt;
        double m2x = 0.0, m2s = 0.0;
        for (unsigned int j0 = 0; j0 < per_plane; j0 += INFLIGHT) {
            double nj[INFLIGHT], dx[INFLIGHT], ds[INFLIGHT], qx[INFLIGHT], qs[INFLIGHT];
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                const bool in = j0 + u < per_plane;
                nj[u] = in ? load_partial(rows + PART * (j0 + u)) : 0.0;
                dx[u] = in ? load_partial(rows + PART * (j0 + u) + 1) - mean_x : 0.0;
                qx[u] = in ? load_partial(rows + PART * (j0 + u) + 2) : 0.0;
                ds[u] = in ? load_partial(rows + PART * (j0 + u) + 3) - mean_s : 0.0;
                qs[u] = in ? load_partial(rows + PART * (j0 + u) + 4) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                m2x += qx[u] + nj[u] * (dx[u] * dx[u]);
                m2s += qs[u] + nj[u] * (ds[u] * ds[u]);
            }
        }
        const double sig_x = sqrt(m2x / (cnt - 1.0) + EPS), sig_s = sqrt(m2s / (cnt - 1.0) + EPS);
        stats[STAT * p] = mean_x;
        stats[STAT * p + 1] = sig_s / sig_x;
        stats[STAT * p + 2] = mean_s;
    }
}

__device__ __forceinline__ float adain_apply(const float v, const double mu_x, const double a, const double mu_s)
{
    return (float)(((double)v - mu_x) * a + mu_s);
}

// grid (blocks per plane, planes), grid-stride over the plane's elements (VEC: its quads)
template <bool VEC>
__global__ __launch_bounds__(THREADS) void color_fix_adain_apply_kernel(const float *__restrict__ x_, float *__restrict__ out_, const int C,
                                                                        const int H, const int W, const int *__restrict__ sizes,
                                                                        const double *__restrict__ stats)
{
    const long long plane = blockIdx.y, hw = (long long)H * W;
    const gf32 *const x = (const gf32 *)x_ + plane * hw;
    gf32 *const out = (gf32 *)out_ + plane * hw;
    int h, w;
    valid_rect(sizes, plane / C, H, W, h, w);
    const double mu_x = stats[STAT * plane], a = stats[STAT * plane + 1], mu_s = stats[STAT * plane + 2];
    const long long step = (long long)gridDim.x * THREADS, first = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (VEC) {
        const int wq = W / 4;
        for (long long q = first; q < hw / 4; q += step) {
            const int gy = (int)(q / wq), gx = 4 * (int)(q % wq);
            f32x4 v = *(const gf32x4 *)(x + 4 * q);
            if (gy < h) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (gx + e < w) v[e] = adain_apply(v[e], mu_x, a, mu_s);
            }
            *(gf32x4 *)(out + 4 * q) = v;
        }
    } else {
        for (long long i = first; i < hw; i += step) {
            const int gy = (int)(i / W), gx = (int)(i % W);
            const float v = x[i];
            out[i] = gy < h && gx < w ? adain_apply(v, mu_x, a, mu_s) : v;
        }
    }
}

bool aligned(const void *p, const size_t a) { return p && ((size_t)p & (a - 1)) == 0; }

// planes = B C in 1 .. 2^31 - 1, H, W >= 1, H W <= 2^30
bool shape_ok(const int B, const int C, const int H, const int W)
{
    return B > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W <= ((long long)1 << 30) && (long long)B * C <= 0x7fffffffll;
}

// blocks of the wavelet launch (one per tile and plane), or -1 when there are more than one launch takes
long long wavelet_blocks(const long long planes, const int H, const int W)
{
    const long long tiles = (long long)((H + TILE - 1) / TILE) * ((W + TILE - 1) / TILE);
    if (planes > (((long long)1 << 31) - 1) / tiles) return -1;
    return planes * tiles;
}

// blocks per plane of the statistics launch; the planes are grid.y
int stats_blocks(const int H, const int W) { return mrefsr::cdiv(H, rows_per_block(W)); }

template <int L>
void launch_wavelet(const bool vec, const dim3 grid, hipStream_t stream, const float *x, const float *s, float *out, const int C, const int H,
                    const int W, const int *sizes)
{
    if (vec) hipLaunchKernelGGL((color_fix_wavelet_kernel<L, true>), grid, dim3(WAVELET_THREADS), 0, stream, x, s, out, C, H, W, sizes);
    else hipLaunchKernelGGL((color_fix_wavelet_kernel<L, false>), grid, dim3(WAVELET_THREADS), 0, stream, x, s, out, C, H, W, sizes);
}

}  // namespace

MREFSR_EXPORT int mrefsr_color_fix_wavelet_f32(const float *x, const float *s, float *out, int B, int C, int H, int W, const int32_t *sizes,
                                               int levels, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(aligned(x, 4) && aligned(s, 4) && aligned(out, 4) && out != x && out != s,
                   "color_fix_wavelet: null pointer or out aliasing an input: x=%p s=%p out=%p (4-byte aligned, out a buffer of its own)",
                   (const void *)x, (const void *)s, (const void *)out);
    MREFSR_REQUIRE(shape_ok(B, C, H, W), "color_fix_wavelet: B=%d C=%d H=%d W=%d (positive, H W <= 2^30, B C < 2^31)", B, C, H, W);
    MREFSR_REQUIRE(levels >= 1 && levels <= 5, "color_fix_wavelet: levels=%d outside 1..5", levels);
    const long long blocks = wavelet_blocks((long long)B * C, H, W);
    MREFSR_REQUIRE(blocks > 0, "color_fix_wavelet: %lld planes of %d x %d: more than 2^31 - 1 tiles of 64 x 64", (long long)B * C, H, W);
    const bool vec = aligned(x, 16) && aligned(s, 16) && aligned(out, 16) && W % 4 == 0;
    const dim3 grid((unsigned int)blocks);
    const hipStream_t st = (hipStream_t)stream;
    switch (levels) {
    case 1: launch_wavelet<1>(vec, grid, st, x, s, out, C, H, W, sizes); break;
    case 2: launch_wavelet<2>(vec, grid, st, x, s, out, C, H, W, sizes); break;
    case 3: launch_wavelet<3>(vec, grid, st, x, s, out, C, H, W, sizes); break;
    case 4: launch_wavelet<4>(vec, grid, st, x, s, out, C, H, W, sizes); break;
    default: launch_wavelet<5>(vec, grid, st, x, s, out, C, H, W, sizes); break;
    }
    return mrefsr::check_launch("color_fix_wavelet");
}

MREFSR_EXPORT int64_t mrefsr_color_fix_adain_workspace_bytes(int B, int C, int H, int W)
{
    if (!shape_ok(B, C, H, W) || (long long)B * C > 65535) return -1;
    const int64_t planes = (int64_t)B * C;
    if (planes * stats_blocks(H, W) > 0x7fffffffll) return -1;   // (the ticket counts the blocks in 32 bits)
    return 8 * (PART * planes * stats_blocks(H, W) + STAT * planes);
}

MREFSR_EXPORT int mrefsr_color_fix_adain_f32(const float *x, const float *s, float *out, int B, int C, int H, int W, const int32_t *sizes,
                                             void *workspace, int64_t workspace_bytes, uint32_t *ticket, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(aligned(x, 4) && aligned(s, 4) && aligned(out, 4) && out != x && out != s,
                   "color_fix_adain: null pointer or out aliasing an input: x=%p s=%p out=%p (4-byte aligned, out a buffer of its own)",
                   (const void *)x, (const void *)s, (const void *)out);
    const int64_t need = mrefsr_color_fix_adain_workspace_bytes(B, C, H, W);
    MREFSR_REQUIRE(need > 0, "color_fix_adain: B=%d C=%d H=%d W=%d (positive, H W <= 2^30, B C <= 65535)", B, C, H, W);
    MREFSR_REQUIRE(sizes || (long long)H * W >= 2, "color_fix_adain: a plane of one pixel has no unbiased variance");
    MREFSR_REQUIRE(aligned(workspace, 8) && workspace_bytes >= need && aligned(ticket, 4),
                   "color_fix_adain: null pointer or short workspace: workspace=%p (8-byte aligned) of %lld bytes, %lld needed, ticket=%p", workspace,
                   (long long)workspace_bytes, (long long)need, (const void *)ticket);
    const int planes = B * C;
    const hipStream_t st = (hipStream_t)stream;
    double *ws = (double *)workspace;
    const double *stats = ws + (long long)PART * planes * stats_blocks(H, W);
    hipLaunchKernelGGL(color_fix_adain_stats_kernel, dim3(stats_blocks(H, W), planes), dim3(THREADS), 0, st, x, s, C, H, W, sizes, ws, ticket);
    int rc = mrefsr::check_launch("color_fix_adain (statistics)");
    if (rc != MREFSR_OK) return rc;
    const bool vec = aligned(x, 16) && aligned(out, 16) && W % 4 == 0;
    const long long hw = (long long)H * W;
    const dim3 grid(mrefsr::grid_of(mrefsr::cdiv(vec ? hw / 4 : hw, 4 * THREADS), 4096), planes);
    if (vec) hipLaunchKernelGGL(color_fix_adain_apply_kernel<true>, grid, dim3(THREADS), 0, st, x, out, C, H, W, sizes, stats);
    else hipLaunchKernelGGL(color_fix_adain_apply_kernel<false>, grid, dim3(THREADS), 0, st, x, out, C, H, W, sizes, stats);
    return mrefsr::check_launch("color_fix_adain (apply)");
}
