// Reflect padding and cropping of channels-last maps, with their adjoints: MRAPAFusion pads its inputs at the bottom and right
// to a multiple of 4 and crops its result back (ref_mrapa_restoration_arch.py:306-311, 348).  Under autograd these are the
// forward and backward of two nodes of the training engine (mrefsr_amd/archs/nhwc_train.py _Pad / _Crop); in inference the
// forward kernels alone.  [N][H][W][C] fp32, C % 4 == 0: one 16-byte vector per thread, one block row of 256 vectors per
// (image, map row) chunk, so a thread finds its pixel with one 32-bit division by C / 4.  Pure data movement, HBM-bound.
#include "common.h"

namespace {

// padded row H + i is source row H - 2 - i (F.pad mode='reflect' at the far edge); a source row y < H is itself
__device__ __forceinline__ int reflect_src(int y, int H) { return y < H ? y : 2 * H - 2 - y; }

__global__ __launch_bounds__(256) void reflect_pad_nhwc_kernel(const float4 *__restrict__ x, float4 *__restrict__ out, int H, int W,
                                                               int Ho, int Wo, int C4)
{
    const int row = blockIdx.x;                               // n * Ho + yo
    const int j = blockIdx.y * 256 + threadIdx.x;             // xo * C4 + c4 within the output row
    if (j >= Wo * C4) return;
    const int n = row / Ho, yo = row - n * Ho;
    const int xo = j / C4, c4 = j - xo * C4;
    const long src = (((long)n * H + reflect_src(yo, H)) * W + reflect_src(xo, W)) * C4 + c4;
    out[(long)row * Wo * C4 + j] = x[src];
}

// Adjoint: source pixel (y, x) gathers its own gradient, then its row image (2H - 2 - y, x), its column image (y, 2W - 2 - x) and
// the corner image (2H - 2 - y, 2W - 2 - x) where those lie inside the padded band -- always in this order, no atomics
__global__ __launch_bounds__(256) void reflect_pad_bwd_nhwc_kernel(const float4 *__restrict__ g, float4 *__restrict__ gx, int H, int W,
                                                                   int Ho, int Wo, int C4)
{
    const int row = blockIdx.x;                               // n * H + y
    const int j = blockIdx.y * 256 + threadIdx.x;             // x * C4 + c4 within the source row
    if (j >= W * C4) return;
    const int n = row / H, y = row - n * H;
    const int x = j / C4, c4 = j - x * C4;
    const int yp = 2 * H - 2 - y, xp = 2 * W - 2 - x;
    const bool rm = y <= H - 2 && yp < Ho, cm = x <= W - 2 && xp < Wo;
    const long base = (long)n * Ho * Wo * C4 + c4;
    float4 a = g[base + ((long)y * Wo + x) * C4];
    if (rm) {
        const float4 b = g[base + ((long)yp * Wo + x) * C4];
        a.x += b.x, a.y += b.y, a.z += b.z, a.w += b.w;
    }
    if (cm) {
        const float4 b = g[base + ((long)y * Wo + xp) * C4];
        a.x += b.x, a.y += b.y, a.z += b.z, a.w += b.w;
    }
    if (rm && cm) {
        const float4 b = g[base + ((long)yp * Wo + xp) * C4];
        a.x += b.x, a.y += b.y, a.z += b.z, a.w += b.w;
    }
    gx[(long)row * W * C4 + j] = a;
}

// top-left H0 x W0 window of x [N][H][W][C]; amax_bits (may be NULL): max |out| as the convolution epilogues publish it
// (mrefsr::publish_amax<true>, reduce.h: one wave reduction, one atomic per wave that raises the word)
__global__ __launch_bounds__(256) void crop_nhwc_kernel(const float4 *__restrict__ x, float4 *__restrict__ out,
                                                        unsigned int *__restrict__ amax_bits, int H, int W, int H0, int W0, int C4)
{
    const int row = blockIdx.x;                               // n * H0 + y
    const int j = blockIdx.y * 256 + threadIdx.x;
    float m = 0.f;
    if (j < W0 * C4) {
        const int n = row / H0, y = row - n * H0;
        const float4 v = x[((long)n * H + y) * W * C4 + j];  // (x < W0 <= W: the window row is a prefix of the source row)
        out[(long)row * W0 * C4 + j] = v;
        m = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    if (amax_bits) mrefsr::publish_amax<true>(amax_bits, m);
}

// adjoint of the crop: g [N][H0][W0][C] into the window of gx [N][H][W][C], zeros in the band to its right and below
__global__ __launch_bounds__(256) void crop_bwd_nhwc_kernel(const float4 *__restrict__ g, float4 *__restrict__ gx, int H, int W, int H0,
                                                            int W0, int C4)
{
    const int row = blockIdx.x;                               // n * H + y
    const int j = blockIdx.y * 256 + threadIdx.x;
    if (j >= W * C4) return;
    const int n = row / H, y = row - n * H;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y < H0 && j < W0 * C4) v = g[((long)n * H0 + y) * W0 * C4 + j];
    gx[(long)row * W * C4 + j] = v;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// one block row per (image, map row) of the written tensor, 256 vectors per block along the row
int launch_rows(const char *what, long rows, long row_vec, dim3 &grid)
{
    MREFSR_REQUIRE(rows > 0 && rows < (1l << 31) && row_vec > 0 && row_vec <= 256l * 65535, "%s: %ld rows of %ld vectors", what, rows, row_vec);
    grid = dim3((unsigned)rows, (unsigned)((row_vec + 255) / 256));
    return MREFSR_OK;
}

}  // namespace

MREFSR_EXPORT int mrefsr_reflect_pad_nhwc_f32(const float *x, float *out, int N, int H, int W, int C, int ph, int pw, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && out, "reflect_pad_nhwc: null pointer");
    MREFSR_REQUIRE(aligned16(x) && aligned16(out), "reflect_pad_nhwc: tensors must be 16-byte aligned");
    MREFSR_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "reflect_pad_nhwc: N=%d H=%d W=%d C=%d (C a positive multiple of 4)", N, H, W, C);
    MREFSR_REQUIRE(ph >= 0 && ph <= 3 && pw >= 0 && pw <= 3, "reflect_pad_nhwc: pads %d x %d (0..3)", ph, pw);
    MREFSR_REQUIRE(ph < H && pw < W, "reflect_pad_nhwc: pads %d x %d need a map larger than that, got %d x %d", ph, pw, H, W);
    dim3 grid;
    if (int rc = launch_rows("reflect_pad_nhwc", (long)N * (H + ph), (long)(W + pw) * (C / 4), grid)) return rc;
    hipLaunchKernelGGL(reflect_pad_nhwc_kernel, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(x),
                       reinterpret_cast<float4 *>(out), H, W, H + ph, W + pw, C / 4);
    return mrefsr::check_launch("reflect_pad_nhwc");
}

MREFSR_EXPORT int mrefsr_reflect_pad_bwd_nhwc_f32(const float *g, float *gx, int N, int H, int W, int C, int ph, int pw, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(g && gx, "reflect_pad_bwd_nhwc: null pointer");
    MREFSR_REQUIRE(aligned16(g) && aligned16(gx), "reflect_pad_bwd_nhwc: tensors must be 16-byte aligned");
    MREFSR_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "reflect_pad_bwd_nhwc: N=%d H=%d W=%d C=%d (C a positive multiple of 4)", N, H,
                   W, C);
    MREFSR_REQUIRE(ph >= 0 && ph <= 3 && pw >= 0 && pw <= 3, "reflect_pad_bwd_nhwc: pads %d x %d (0..3)", ph, pw);
    MREFSR_REQUIRE(ph < H && pw < W, "reflect_pad_bwd_nhwc: pads %d x %d need a map larger than that, got %d x %d", ph, pw, H, W);
    dim3 grid;
    if (int rc = launch_rows("reflect_pad_bwd_nhwc", (long)N * H, (long)W * (C / 4), grid)) return rc;
    hipLaunchKernelGGL(reflect_pad_bwd_nhwc_kernel, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(g),
                       reinterpret_cast<float4 *>(gx), H, W, H + ph, W + pw, C / 4);
    return mrefsr::check_launch("reflect_pad_bwd_nhwc");
}

MREFSR_EXPORT int mrefsr_crop_nhwc_f32(const float *x, float *out, float *amax, int N, int H, int W, int C, int H0, int W0, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && out, "crop_nhwc: null pointer");
    MREFSR_REQUIRE(aligned16(x) && aligned16(out), "crop_nhwc: tensors must be 16-byte aligned");
    MREFSR_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "crop_nhwc: N=%d H=%d W=%d C=%d (C a positive multiple of 4)", N, H, W, C);
    MREFSR_REQUIRE(H0 > 0 && H0 <= H && W0 > 0 && W0 <= W, "crop_nhwc: window %d x %d of a %d x %d map", H0, W0, H, W);
    dim3 grid;
    if (int rc = launch_rows("crop_nhwc", (long)N * H0, (long)W0 * (C / 4), grid)) return rc;
    hipLaunchKernelGGL(crop_nhwc_kernel, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(x),
                       reinterpret_cast<float4 *>(out), reinterpret_cast<unsigned int *>(amax), H, W, H0, W0, C / 4);
    return mrefsr::check_launch("crop_nhwc");
}

MREFSR_EXPORT int mrefsr_crop_bwd_nhwc_f32(const float *g, float *gx, int N, int H, int W, int C, int H0, int W0, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(g && gx, "crop_bwd_nhwc: null pointer");
    MREFSR_REQUIRE(aligned16(g) && aligned16(gx), "crop_bwd_nhwc: tensors must be 16-byte aligned");
    MREFSR_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "crop_bwd_nhwc: N=%d H=%d W=%d C=%d (C a positive multiple of 4)", N, H, W, C);
    MREFSR_REQUIRE(H0 > 0 && H0 <= H && W0 > 0 && W0 <= W, "crop_bwd_nhwc: window %d x %d of a %d x %d map", H0, W0, H, W);
    dim3 grid;
    if (int rc = launch_rows("crop_bwd_nhwc", (long)N * H, (long)W * (C / 4), grid)) return rc;
    hipLaunchKernelGGL(crop_bwd_nhwc_kernel, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(g),
                       reinterpret_cast<float4 *>(gx), H, W, H0, W0, C / 4);
    return mrefsr::check_launch("crop_bwd_nhwc");
}
