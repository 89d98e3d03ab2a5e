// Differentiable discriminator augmentation (train.d_augment; DiffAugment, Zhao et al. 2020, and the pixel / colour part of ADA's
// pipeline, Karras et al. 2020): one random transformation T per sample in front of every discriminator call.  For fixed
// parameters T(x) = L x + b with L linear, so the forward is one kernel, its backward the adjoint kernel, and the backward of that
// the forward without its bias.
//
// Images are fp32 [B][3][H][W].  Sample b has fpar[b] = {db, s, c, unused} (brightness offset, saturation factor, contrast factor)
// and ipar[b] = {flip, ty, tx, y0, y1, x0, x1, unused} (horizontal flip, integer translation of any size, cut box [y0,y1) x [x0,x1)).
//
// Forward, output pixel (y, x), N = 3 H W, every line one fp32 operation (-ffp-contract=off, Makefile: nothing is fused):
//     inside the cut box                         -> out_ch = 0 for the three channels (selected, not multiplied: a NaN there is dropped)
//     sy = y - ty, sx0 = x - tx outside the image -> out_ch = 0 likewise
//     sx   = flip ? W - 1 - sx0 : sx0
//     v_ch = in[b][ch][sy][sx] + db
//     mu   = ((v_0 + v_1) + v_2) / 3
//     u_ch = s * v_ch + (1 - s) * mu
//     m    = fl32(sum_b / N) + db                 sum_b: the sample's 3 H W inputs added in double in a fixed order (below)
//     out_ch = c * u_ch + (1 - c) * m
// With db = 0, s = 1, c = 1, no flip, no shift and an empty box every line returns its input's value: out == in.  with_bias = 0
// takes db as 0 in v_ch and in m: the linear part L alone, which is the second-order node.
//
// Adjoint, source pixel (sy, sx): x = (flip ? W - 1 - sx : sx) + tx, y = sy + ty is the one output pixel that reads it;
//     G_ch  = g[b][ch][y][x] if (y, x) is inside the image and outside the cut box, else 0 (selected)
//     t_ch  = s * G_ch + (1 - s) * (((G_0 + G_1) + G_2) / 3)
//     gx_ch = c * t_ch + fl32((1 - c) / N) * fl32(S_b)     S_b: g over the sample's kept output pixels, added in double likewise
// (the quotient (1 - c) / N is taken in double from the fp32 difference: one rounding).  The brightness bias has no adjoint term.
//
// The per-sample sums (one launch, skipped when the caller says that no sample has contrast, contrast = 0: c is then taken as 1
// and m, S_b as 0 whatever the table holds): the sample's N elements are cut into R = clamp(ceil(N / 4096), 1, 64) contiguous
// ranges [N r / R, N (r + 1) / R), one block of 256 threads each, thread t adding elements lo + t, lo + t + 256, ... of its range
// in double; block_sum_by_waves; one double per block into workspace[B + b R + r]; the block that draws the last ticket of the
// launch adds each sample's R partials in ascending order into workspace[b].  No float atomics, no readback, the same bits from
// call to call; the grids are pure functions of (B, H, W).  The apply pass is the second launch: one thread per pixel and its
// three channels, plain 4-byte accesses (at B = 4, 160 x 160 the tensors are 1.2 MB and the launches latency-bound).
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int RANGE = 4096;        // elements of a sample per reduction block, until MAX_ROW_BLOCKS caps the count
constexpr int MAX_ROW_BLOCKS = 64;

// device-memory addresses: said so, they are accessed with global_* instead of flat_* instructions
typedef __attribute__((address_space(1))) float gf32;

struct Params {
    float db, s, c;
    int flip;
    long long ty, tx;
    int y0, y1, x0, x1;
};

__device__ __forceinline__ Params load_params(const float *__restrict__ fpar, const int *__restrict__ ipar, const long long b)
{
    Params p;
    p.db = fpar[4 * b + 0], p.s = fpar[4 * b + 1], p.c = fpar[4 * b + 2];
    p.flip = ipar[8 * b + 0] != 0;
    p.ty = ipar[8 * b + 1], p.tx = ipar[8 * b + 2];
    p.y0 = ipar[8 * b + 3], p.y1 = ipar[8 * b + 4], p.x0 = ipar[8 * b + 5], p.x1 = ipar[8 * b + 6];
    return p;
}

// output pixel (y, x) -> is it written from a source pixel (neither cut nor shifted in from outside), and from which
__device__ __forceinline__ bool source_of(const Params &p, const int H, const int W, const int y, const int x, int &sy, int &sx)
{
    if (y >= p.y0 && y < p.y1 && x >= p.x0 && x < p.x1) return false;
    const long long ly = (long long)y - p.ty, lx = (long long)x - p.tx;
    if (ly < 0 || ly >= H || lx < 0 || lx >= W) return false;
    sy = (int)ly;
    sx = p.flip ? W - 1 - (int)lx : (int)lx;
    return true;
}

inline int row_blocks(const long long n)
{
    const long long r = (n + RANGE - 1) / RANGE;
    return (int)(r < 1 ? 1 : (r > MAX_ROW_BLOCKS ? MAX_ROW_BLOCKS : r));
}

// ws: [B] sums, then [B][R] partials.  ADJ: the elements of g at kept output pixels; otherwise every element of x.
template <bool ADJ>
__global__ __launch_bounds__(THREADS) void disc_augment_sum_kernel(const float *__restrict__ src_, const float *__restrict__ fpar,
                                                                   const int *__restrict__ ipar, const int H, const int W, double *ws,
                                                                   unsigned int *ticket)
{
    __shared__ double wsum[THREADS / 64];
    __shared__ int last;
    const int tid = threadIdx.x;
    const long long b = blockIdx.y, hw = (long long)H * W, n = 3 * hw;
    const int B = gridDim.y, R = gridDim.x;
    const gf32 *const src = (const gf32 *)src_ + b * n;
    const long long lo = n * blockIdx.x / R, hi = n * (blockIdx.x + 1) / R;
    Params p;
    if constexpr (ADJ) p = load_params(fpar, ipar, b);
    double acc = 0.0;
    for (long long i = lo + tid; i < hi; i += THREADS) {
        float v = src[i];
        if constexpr (ADJ) {
            const unsigned int q = (unsigned int)i % (unsigned int)hw;   // (N < 2^31: shape_ok)
            int sy, sx;
            if (!source_of(p, H, W, (int)(q / (unsigned int)W), (int)(q % (unsigned int)W), sy, sx)) v = 0.f;
        }
        acc += (double)v;
    }
    const double s = mrefsr::block_sum_by_waves<THREADS>(acc, wsum);
    double *const partial = ws + B;
    if (tid == 0) __hip_atomic_store(partial + b * R + blockIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!mrefsr::last_block_by_ticket(ticket, (unsigned int)B * R, &last)) return;
    for (int q = tid; q < B; q += THREADS) {
        double t = 0.0;
        for (int r = 0; r < R; ++r) t += __hip_atomic_load(partial + (long long)q * R + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ws[q] = t;
    }
}

template <bool CONTRAST>
__global__ __launch_bounds__(THREADS) void disc_augment_fwd_kernel(const float *__restrict__ x_, const float *__restrict__ fpar,
                                                                   const int *__restrict__ ipar, const int H, const int W,
                                                                   const int with_bias, const double *__restrict__ sums,
                                                                   float *__restrict__ out_)
{
    const long long b = blockIdx.y, hw = (long long)H * W;
    const long long q = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (q >= hw) return;
    const Params p = load_params(fpar, ipar, b);
    gf32 *const out = (gf32 *)out_ + b * 3 * hw + q;
    int sy, sx;
    if (!source_of(p, H, W, (int)((unsigned int)q / (unsigned int)W), (int)((unsigned int)q % (unsigned int)W), sy, sx)) {
        out[0] = 0.f, out[hw] = 0.f, out[2 * hw] = 0.f;
        return;
    }
    const gf32 *const in = (const gf32 *)x_ + b * 3 * hw + (long long)sy * W + sx;
    const float db = with_bias ? p.db : 0.f;
    const float v0 = in[0] + db, v1 = in[hw] + db, v2 = in[2 * hw] + db;
    const float mu = ((v0 + v1) + v2) / 3.f;
    const float os = 1.f - p.s, t = os * mu;
    const float u0 = p.s * v0 + t, u1 = p.s * v1 + t, u2 = p.s * v2 + t;
    float c = 1.f, m = 0.f;
    if constexpr (CONTRAST) {
        c = p.c;
        m = (float)(sums[b] / (double)(3 * hw)) + db;
    }
    const float k = (1.f - c) * m;
    out[0] = c * u0 + k, out[hw] = c * u1 + k, out[2 * hw] = c * u2 + k;
}

template <bool CONTRAST>
__global__ __launch_bounds__(THREADS) void disc_augment_adj_kernel(const float *__restrict__ g_, const float *__restrict__ fpar,
                                                                   const int *__restrict__ ipar, const int H, const int W,
                                                                   const double *__restrict__ sums, float *__restrict__ gx_)
{
    const long long b = blockIdx.y, hw = (long long)H * W;
    const long long q = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (q >= hw) return;
    const Params p = load_params(fpar, ipar, b);
    const int sy = (int)((unsigned int)q / (unsigned int)W), sx = (int)((unsigned int)q % (unsigned int)W);
    // the one output pixel that reads this source pixel
    const long long y = (long long)sy + p.ty, x = (long long)(p.flip ? W - 1 - sx : sx) + p.tx;
    const bool kept = y >= 0 && y < H && x >= 0 && x < W && !(y >= p.y0 && y < p.y1 && x >= p.x0 && x < p.x1);
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (kept) {
        const gf32 *const g = (const gf32 *)g_ + b * 3 * hw + y * W + x;
        g0 = g[0], g1 = g[hw], g2 = g[2 * hw];
    }
    const float mg = ((g0 + g1) + g2) / 3.f;
    const float os = 1.f - p.s, t = os * mg;
    const float t0 = p.s * g0 + t, t1 = p.s * g1 + t, t2 = p.s * g2 + t;
    float c = 1.f, k = 0.f;
    if constexpr (CONTRAST) {
        c = p.c;
        k = (float)((double)(1.f - c) / (double)(3 * hw)) * (float)sums[b];
    }
    gf32 *const gx = (gf32 *)gx_ + b * 3 * hw + q;
    gx[0] = c * t0 + k, gx[hw] = c * t1 + k, gx[2 * hw] = c * t2 + k;
}

bool shape_ok(const int B, const int H, const int W)
{
    return B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 28);
}

int check_args(const char *what, const float *a, const float *fpar, const int *ipar, const int B, const int H, const int W,
               const int contrast, const float *o, const void *workspace, const int64_t workspace_bytes, const unsigned int *ticket)
{
    MREFSR_REQUIRE(shape_ok(B, H, W), "%s: B=%d (1..65535) H=%d W=%d (H W in 1..2^28)", what, B, H, W);
    MREFSR_REQUIRE(a && o && fpar && ipar && (((size_t)a | (size_t)o | (size_t)fpar | (size_t)ipar) & 3) == 0 && a != o,
                   "%s: in=%p out=%p fpar=%p ipar=%p (4-byte aligned, not in place)", what, (const void *)a, (const void *)o,
                   (const void *)fpar, (const void *)ipar);
    MREFSR_REQUIRE(!contrast || (workspace && ((size_t)workspace & 7) == 0 && ticket && ((size_t)ticket & 3) == 0 &&
                                 workspace_bytes >= mrefsr_disc_augment_workspace_bytes(B, H, W)),
                   "%s: workspace=%p (8-byte aligned) of %lld bytes, %lld needed, ticket=%p", what, workspace, (long long)workspace_bytes,
                   (long long)mrefsr_disc_augment_workspace_bytes(B, H, W), (const void *)ticket);
    return MREFSR_OK;
}

}  // namespace

MREFSR_EXPORT int64_t mrefsr_disc_augment_workspace_bytes(int B, int H, int W)
{
    return shape_ok(B, H, W) ? (int64_t)B * (1 + row_blocks(3 * (long long)H * W)) * (int64_t)sizeof(double) : -1;
}

MREFSR_EXPORT int mrefsr_disc_augment_f32(const float *x, const float *fpar, const int *ipar, int B, int H, int W, int with_bias,
                                          int contrast, float *out, void *workspace, int64_t workspace_bytes, unsigned int *ticket,
                                          mrefsr_stream_t stream)
{
    if (const int e = check_args("disc_augment", x, fpar, ipar, B, H, W, contrast, out, workspace, workspace_bytes, ticket)) return e;
    const long long hw = (long long)H * W;
    const dim3 grid((unsigned int)((hw + THREADS - 1) / THREADS), B);
    if (contrast) {
        hipLaunchKernelGGL(disc_augment_sum_kernel<false>, dim3(row_blocks(3 * hw), B), dim3(THREADS), 0, (hipStream_t)stream, x, fpar, ipar,
                           H, W, (double *)workspace, ticket);
        hipLaunchKernelGGL(disc_augment_fwd_kernel<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, x, fpar, ipar, H, W, with_bias,
                           (const double *)workspace, out);
    } else {
        hipLaunchKernelGGL(disc_augment_fwd_kernel<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, x, fpar, ipar, H, W, with_bias,
                           (const double *)nullptr, out);
    }
    return mrefsr::check_launch("disc_augment");
}

MREFSR_EXPORT int mrefsr_disc_augment_adj_f32(const float *g, const float *fpar, const int *ipar, int B, int H, int W, int contrast,
                                              float *gx, void *workspace, int64_t workspace_bytes, unsigned int *ticket,
                                              mrefsr_stream_t stream)
{
    if (const int e = check_args("disc_augment_adj", g, fpar, ipar, B, H, W, contrast, gx, workspace, workspace_bytes, ticket)) return e;
    const long long hw = (long long)H * W;
    const dim3 grid((unsigned int)((hw + THREADS - 1) / THREADS), B);
    if (contrast) {
        hipLaunchKernelGGL(disc_augment_sum_kernel<true>, dim3(row_blocks(3 * hw), B), dim3(THREADS), 0, (hipStream_t)stream, g, fpar, ipar,
                           H, W, (double *)workspace, ticket);
        hipLaunchKernelGGL(disc_augment_adj_kernel<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, g, fpar, ipar, H, W,
                           (const double *)workspace, gx);
    } else {
        hipLaunchKernelGGL(disc_augment_adj_kernel<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, g, fpar, ipar, H, W,
                           (const double *)nullptr, gx);
    }
    return mrefsr::check_launch("disc_augment_adj");
}
