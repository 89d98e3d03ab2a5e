// The x8 geometric self-ensemble of test() (val.self_ensemble; the "+" protocol of EDSR and its successors): the eight flipped and
// transposed copies of the inputs, and the average of the eight outputs with every transform undone.
//
// Copy j in 0..3 of a group: hf = j & 1, vf = (j >> 1) & 1; the group is untransposed (tr = 0) or transposed (tr = 1).  In torch,
// on src [..., H, W]:   s = src; if hf: s = s.flip(-1); if vf: s = s.flip(-2); if tr: s = s.transpose(-1, -2)
// (the order of data/multi_ref_dataset.py: augment), so with fy(y) = vf ? H - 1 - y : y and fx(x) = hf ? W - 1 - x : x
//     tr = 0:  copy[y][x] = src[fy(y)][fx(x)]              tr = 1:  copy[x][y] = src[fy(y)][fx(x)]      (copy is [W][H])
// and the inverse applied to an output of that copy reads the same element back:
//     tr = 0:  out'[y][x] = a[fy(y)][fx(x)]                tr = 1:  out'[y][x] = b[fx(x)][fy(y)]        (b is [W][H])
//
// dihedral_expand: one block per 32 x 32 tile of a source plane; the tile is read once and written to the four copies.  The flips are
// index arithmetic: a wave's addresses stay contiguous, in descending order under a flip.  In the transposed group the tile goes
// through a [32][33]-word LDS tile (row stride 33: rows and columns of the tile both fall on 32 different banks), so the global
// reads run along the source's rows and the global writes along the copies' rows.  Pure copies of 32-bit words: NaN payloads,
// infinities and -0 keep their bits.
//
// dihedral_merge: one block per 32 x 32 tile of an output plane.  The four outputs of the transposed group are staged in four LDS
// tiles (read along b's rows); then  out = (((((((a0' + a1') + a2') + a3') + b0') + b1') + b2') + b3') * 0.125f  in fp32, the adds
// in exactly this order and one multiply behind them (-ffp-contract=off, Makefile): the bits of the same chain written in torch.
//
// Each kernel has two forms.  16-byte accesses, a thread owning four consecutive words of a row (a flipped group of four is one
// aligned 16-byte access with its words in reverse order), when every row involved starts on a 16-byte boundary: the pointers
// aligned, W % 4 == 0, and H % 4 == 0 where rows of length H are read or written (tr = 1, merge).  4-byte accesses otherwise.
#include "common.h"

namespace {

constexpr int TILE = 32;
constexpr int LD = TILE + 1;
constexpr int THREADS = 256;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// device-memory addresses: said so, they are accessed with global_* instead of flat_* instructions
typedef __attribute__((address_space(1))) unsigned int gu32;
typedef __attribute__((address_space(1))) u32x4 gu32x4;
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

struct Tile {
    long long plane;
    int y0, x0;
};

// blockIdx.x = (plane * tiles_y + tile_y) * tiles_x + tile_x
__device__ __forceinline__ Tile tile_of_block(const int H, const int W)
{
    const int tx = (W + TILE - 1) / TILE, ty = (H + TILE - 1) / TILE;
    const unsigned int b = blockIdx.x;
    Tile t;
    t.x0 = (int)(b % tx) * TILE;
    t.y0 = (int)((b / tx) % ty) * TILE;
    t.plane = b / tx / ty;
    return t;
}

template <typename V> __device__ __forceinline__ V reversed(const V v)
{
    V r;
    r[0] = v[3], r[1] = v[2], r[2] = v[1], r[3] = v[0];
    return r;
}

// src [outer][inner][C][H][W] -> dst [outer][4][inner][C][H][W] (tr = 0) or [outer][4][inner][C][W][H] (tr = 1)
template <bool TR, bool VEC>
__global__ __launch_bounds__(THREADS) void dihedral_expand_kernel(const unsigned int *__restrict__ src_, unsigned int *__restrict__ dst_,
                                                                  const int inner, const int C, const int H, const int W)
{
    __shared__ unsigned int tile[TR ? TILE * LD : 1];
    const Tile t = tile_of_block(H, W);
    const long long hw = (long long)H * W;
    const long long ic = (long long)inner * C;
    const long long o = t.plane / ic, rest = t.plane % ic;   // plane = (o * inner + i) * C + c; rest = i * C + c
    const gu32 *const src = (const gu32 *)src_ + t.plane * hw;
    gu32 *const dst = (gu32 *)dst_ + (o * 4 * ic + rest) * hw;   // copy 0; copy j lies j * ic planes behind it
    const int tid = threadIdx.x;
    if (VEC) {
        const int q = tid & 7, r = tid >> 3;
        const int y = t.y0 + r, x = t.x0 + 4 * q;
        const bool in = y < H && x < W;   // (W % 4 == 0: a group of four is inside or outside as a whole)
        u32x4 v = {0u, 0u, 0u, 0u};
        if (in) v = *(const gu32x4 *)(src + (long long)y * W + x);
        if (!TR) {
            if (!in) return;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int yy = (j & 2) ? H - 1 - y : y, xx = (j & 1) ? W - 4 - x : x;
                *(gu32x4 *)(dst + j * ic * hw + (long long)yy * W + xx) = (j & 1) ? reversed(v) : v;
            }
            return;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[r * LD + 4 * q + e] = v[e];
        __syncthreads();
        // this thread: source rows y0 + 4 q .. + 3 (a group of four along the copies' rows, H % 4 == 0), source column x0 + r
        const int ys = t.y0 + 4 * q, xs = t.x0 + r;
        if (ys >= H || xs >= W) return;
        u32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = tile[(4 * q + e) * LD + r];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = (j & 1) ? W - 1 - xs : xs, col = (j & 2) ? H - 4 - ys : ys;
            *(gu32x4 *)(dst + j * ic * hw + (long long)row * H + col) = (j & 2) ? reversed(w) : w;
        }
        return;
    }
    const int lx = tid & 31, ly = tid >> 5;
    if (!TR) {
        const int x = t.x0 + lx;
#pragma unroll
        for (int k = 0; k < TILE / 8; ++k) {
            const int y = t.y0 + ly + 8 * k;
            if (y >= H || x >= W) continue;
            const unsigned int v = src[(long long)y * W + x];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int yy = (j & 2) ? H - 1 - y : y, xx = (j & 1) ? W - 1 - x : x;
                dst[j * ic * hw + (long long)yy * W + xx] = v;
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < TILE / 8; ++k) {
        const int r = ly + 8 * k, y = t.y0 + r, x = t.x0 + lx;
        if (y < H && x < W) tile[r * LD + lx] = src[(long long)y * W + x];
    }
    __syncthreads();
    // lanes along the source's rows = along the copies' rows
    const int ys = t.y0 + lx;
#pragma unroll
    for (int k = 0; k < TILE / 8; ++k) {
        const int c = ly + 8 * k, xs = t.x0 + c;
        if (ys >= H || xs >= W) continue;
        const unsigned int v = tile[lx * LD + c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = (j & 1) ? W - 1 - xs : xs, col = (j & 2) ? H - 1 - ys : ys;
            dst[j * ic * hw + (long long)row * H + col] = v;
        }
    }
}

// a [4][N][C][H][W], b [4][N][C][W][H] -> out [N][C][H][W]; planes = N * C
template <bool VEC>
__global__ __launch_bounds__(THREADS) void dihedral_merge_kernel(const float *__restrict__ a_, const float *__restrict__ b_,
                                                                 float *__restrict__ out_, const long long planes, const int H, const int W)
{
    __shared__ float tile[4][TILE * LD];   // tile[j][r][c] = b_j[fx(x0 + r)][fy(y0 + c)]
    const Tile t = tile_of_block(H, W);
    const long long hw = (long long)H * W;
    const gf32 *const a = (const gf32 *)a_ + t.plane * hw;
    const gf32 *const b = (const gf32 *)b_ + t.plane * hw;
    gf32 *const out = (gf32 *)out_ + t.plane * hw;
    const long long copy = planes * hw;   // elements of one copy's outputs
    const int tid = threadIdx.x;
    if (VEC) {
        const int q = tid & 7, r = tid >> 3;
        {   // b's rows: tile row r <-> out column x0 + r, four tile columns 4 q .. + 3 <-> out rows y0 + 4 q .. + 3
            const int xs = t.x0 + r, ys = t.y0 + 4 * q;
            if (xs < W && ys < H) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int row = (j & 1) ? W - 1 - xs : xs, col = (j & 2) ? H - 4 - ys : ys;
                    f32x4 v = *(const gf32x4 *)(b + j * copy + (long long)row * H + col);
                    if (j & 2) v = reversed(v);
#pragma unroll
                    for (int e = 0; e < 4; ++e) tile[j][r * LD + 4 * q + e] = v[e];
                }
            }
        }
        __syncthreads();
        const int y = t.y0 + r, x = t.x0 + 4 * q;
        if (y >= H || x >= W) return;
        f32x4 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int yy = (j & 2) ? H - 1 - y : y, xx = (j & 1) ? W - 4 - x : x;
            f32x4 v = *(const gf32x4 *)(a + j * copy + (long long)yy * W + xx);
            if (j & 1) v = reversed(v);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = j == 0 ? v[e] : acc[e] + v[e];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = acc[e] + tile[j][(4 * q + e) * LD + r];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = acc[e] * 0.125f;
        *(gf32x4 *)(out + (long long)y * W + x) = acc;
        return;
    }
    const int lx = tid & 31, ly = tid >> 5;
    {   // lanes along b's rows
        const int ys = t.y0 + lx;
#pragma unroll
        for (int k = 0; k < TILE / 8; ++k) {
            const int r = ly + 8 * k, xs = t.x0 + r;
            if (xs >= W || ys >= H) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = (j & 1) ? W - 1 - xs : xs, col = (j & 2) ? H - 1 - ys : ys;
                tile[j][r * LD + lx] = b[j * copy + (long long)row * H + col];
            }
        }
    }
    __syncthreads();
    const int x = t.x0 + lx;
#pragma unroll
    for (int k = 0; k < TILE / 8; ++k) {
        const int r = ly + 8 * k, y = t.y0 + r;
        if (y >= H || x >= W) continue;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int yy = (j & 2) ? H - 1 - y : y, xx = (j & 1) ? W - 1 - x : x;
            const float v = a[j * copy + (long long)yy * W + xx];
            acc = j == 0 ? v : acc + v;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = acc + tile[j][lx * LD + r];
        out[(long long)y * W + x] = acc * 0.125f;
    }
}

// the number of blocks (one per tile and plane), or -1 when the shape is outside what one launch takes
long long blocks_of(const long long planes, const int H, const int W)
{
    if (planes <= 0 || H <= 0 || W <= 0 || (long long)H * W > ((long long)1 << 30)) return -1;
    const long long tiles = (long long)((H + TILE - 1) / TILE) * ((W + TILE - 1) / TILE);
    if (planes > (((long long)1 << 31) - 1) / tiles) return -1;
    return planes * tiles;
}

bool aligned(const void *p, const size_t a) { return p && ((size_t)p & (a - 1)) == 0; }

}  // namespace

MREFSR_EXPORT int mrefsr_dihedral_expand_f32(const float *src, float *dst, int outer, int inner, int C, int H, int W, int tr,
                                             mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(aligned(src, 4) && aligned(dst, 4) && src != dst, "dihedral_expand: src=%p dst=%p (two 4-byte aligned buffers)",
                   (const void *)src, (const void *)dst);
    MREFSR_REQUIRE(outer > 0 && inner > 0 && C > 0 && (tr == 0 || tr == 1), "dihedral_expand: outer=%d inner=%d C=%d (positive) tr=%d (0 or 1)",
                   outer, inner, C, tr);
    const long long planes = (long long)outer * inner * C;
    const long long blocks = blocks_of(planes, H, W);
    MREFSR_REQUIRE(blocks > 0, "dihedral_expand: %lld planes of %d x %d (H, W >= 1, H W <= 2^30, at most 2^31 - 1 tiles of 32 x 32)", planes, H, W);
    const bool vec = aligned(src, 16) && aligned(dst, 16) && W % 4 == 0 && (!tr || H % 4 == 0);
    const unsigned int *s = (const unsigned int *)src;
    unsigned int *d = (unsigned int *)dst;
    const dim3 grid((unsigned int)blocks), block(THREADS);
    if (tr && vec) hipLaunchKernelGGL((dihedral_expand_kernel<true, true>), grid, block, 0, (hipStream_t)stream, s, d, inner, C, H, W);
    else if (tr) hipLaunchKernelGGL((dihedral_expand_kernel<true, false>), grid, block, 0, (hipStream_t)stream, s, d, inner, C, H, W);
    else if (vec) hipLaunchKernelGGL((dihedral_expand_kernel<false, true>), grid, block, 0, (hipStream_t)stream, s, d, inner, C, H, W);
    else hipLaunchKernelGGL((dihedral_expand_kernel<false, false>), grid, block, 0, (hipStream_t)stream, s, d, inner, C, H, W);
    return mrefsr::check_launch("dihedral_expand");
}

MREFSR_EXPORT int mrefsr_dihedral_merge_f32(const float *a, const float *b, float *out, int N, int C, int H, int W, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(aligned(a, 4) && aligned(b, 4) && aligned(out, 4) && out != a && out != b,
                   "dihedral_merge: a=%p b=%p out=%p (4-byte aligned, out a buffer of its own)", (const void *)a, (const void *)b, (const void *)out);
    MREFSR_REQUIRE(N > 0 && C > 0, "dihedral_merge: N=%d C=%d (positive)", N, C);
    const long long planes = (long long)N * C;
    const long long blocks = blocks_of(planes, H, W);
    MREFSR_REQUIRE(blocks > 0, "dihedral_merge: %lld planes of %d x %d (H, W >= 1, H W <= 2^30, at most 2^31 - 1 tiles of 32 x 32)", planes, H, W);
    const bool vec = aligned(a, 16) && aligned(b, 16) && aligned(out, 16) && W % 4 == 0 && H % 4 == 0;
    const dim3 grid((unsigned int)blocks), block(THREADS);
    if (vec) hipLaunchKernelGGL(dihedral_merge_kernel<true>, grid, block, 0, (hipStream_t)stream, a, b, out, planes, H, W);
    else hipLaunchKernelGGL(dihedral_merge_kernel<false>, grid, block, 0, (hipStream_t)stream, a, b, out, planes, H, W);
    return mrefsr::check_launch("dihedral_merge");
}
