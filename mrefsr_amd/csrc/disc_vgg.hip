// VGGStyleDiscriminator of the adversarial training step (basicsr/archs/discriminator_arch.py:47-125, input_size 160; trained by
// MultiRefRestorationModel.optimize_parameters and differentiated twice by gradient_penalty_loss, basicsr/models/losses.py:370-404):
// the kernels of mrefsr_amd/archs/nhwc_vggdisc.py that csrc/disc.hip does not have.  BatchNorm + LeakyReLU and the image packing are
// disc.hip's entry points, used as they are.
//   disc_vconv_*            the 3x3 / stride 1 / pad 1 and 4x4 / stride 2 / pad 1 convolutions: forward (+ bias + LeakyReLU), input
//                           gradient, weight gradient and the weight packing, on the implicit-GEMM kernel and the host drivers of
//                           disc_conv_gemm.h (which disc_sg2.hip shares); here: the table of the two layers and the entry points
//   lrelu_mask              g lrelu'(y), the mask from the output's sign (backward and double backward of conv0_0's LeakyReLU)
//   lin_*                   the head: NCHW flatten of f [N][HW][C] -> Linear(C HW, J) -> LeakyReLU -> Linear(J, 1): forward,
//                           backward, double backward (linear1's weight is read in torch's [J][C HW] layout, feature c HW + p)
// No float atomics anywhere: two runs give the same bits.
#include "disc_conv_gemm.h"

namespace {

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
        const float s = mrefsr::block_sum<256>(red, part);
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
const ConvLayer kLayers[] = {conv_layer<3, 1, 1>(), conv_layer<4, 2, 1>()};

int check_vconv(const char *what, int N, int H, int W, int Cin, int Cout, int ks, const ConvLayer *&L)
{
    L = find_layer(kLayers, ks);
    if (!L) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: kernel size %d (3: stride 1, 4: stride 2; pad 1)", what, ks);
    if (N <= 0 || H < (ks == 4 ? 2 : 1) || W < (ks == 4 ? 2 : 1))
        return mrefsr::fail(MREFSR_E_INVALID, "%s: N=%d H=%d W=%d", what, N, H, W);
    return check_channels(what, Cin, Cout);
}

}  // namespace

MREFSR_EXPORT int mrefsr_disc_vconv_pack_weight_f32(const float *w, float *wpk, int Cout, int CinR, int Cin, int ks, int dgrad, mrefsr_stream_t stream)
{
    return conv_pack_weight("disc_vconv_pack_weight", find_layer(kLayers, ks), w, wpk, Cout, CinR, Cin, ks, dgrad, stream);
}

MREFSR_EXPORT int64_t mrefsr_disc_vconv_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks, int dgrad)
{
    const ConvLayer *L;
    if (check_vconv("disc_vconv_workspace_bytes", N, H, W, Cin, Cout, ks, L)) return -1;
    return conv_workspace_bytes(*L, N, H, W, Cin, Cout, dgrad);
}

MREFSR_EXPORT int mrefsr_disc_vconv_f32(const float *x, const float *wpk, const float *bias, float *y, int N, int H, int W, int Cin, int Cout, int ks,
                                        int act, float slope, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && wpk && y, "disc_vconv: null pointer");
    const ConvLayer *L;
    int rc = check_vconv("disc_vconv", N, H, W, Cin, Cout, ks, L);
    if (rc) return rc;
    return conv_run("disc_vconv", *L, 0, x, wpk, bias, nullptr, y, N, H, W, Cin, Cout, act, slope, workspace, workspace_bytes, stream);
}

MREFSR_EXPORT int mrefsr_disc_vconv_dgrad_f32(const float *dy, const float *wpk_d, float *dx, int N, int H, int W, int Cin, int Cout, int ks,
                                              void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(dy && wpk_d && dx, "disc_vconv_dgrad: null pointer");
    const ConvLayer *L;
    int rc = check_vconv("disc_vconv_dgrad", N, H, W, Cin, Cout, ks, L);
    if (rc) return rc;
    return conv_run("disc_vconv_dgrad", *L, 1, dy, wpk_d, nullptr, nullptr, dx, N, H, W, Cin, Cout, 0, 0.f, workspace, workspace_bytes, stream);
}

MREFSR_EXPORT int64_t mrefsr_disc_vconv_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks)
{
    const ConvLayer *L;
    if (check_vconv("disc_vconv_wgrad_workspace_bytes", N, H, W, Cin, Cout, ks, L)) return -1;
    return conv_wgrad_workspace_bytes(*L, N, H, W, Cin, Cout);
}

MREFSR_EXPORT int mrefsr_disc_vconv_wgrad_f32(const float *x, const float *dy, float *dw, int N, int H, int W, int Cin, int CinR, int Cout, int ks,
                                              void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && dy && dw && workspace, "disc_vconv_wgrad: null pointer");
    const ConvLayer *L;
    int rc = check_vconv("disc_vconv_wgrad", N, H, W, Cin, Cout, ks, L);
    if (rc) return rc;
    return conv_wgrad("disc_vconv_wgrad", *L, x, dy, dw, N, H, W, Cin, CinR, Cout, workspace, workspace_bytes, stream);
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
