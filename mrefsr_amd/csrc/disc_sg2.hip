// StyleGAN2Discriminator of the adversarial training step (basicsr/archs/stylegan2_arch.py:733-799; trained by
// MultiRefRestorationModel.optimize_parameters and differentiated twice by gradient_penalty_loss): the kernels of
// mrefsr_amd/archs/nhwc_sg2disc.py that csrc/disc_vgg.hip and csrc/disc.hip do not have.  conv1 of every ResBlock and final_conv run on
// disc_vgg.hip's 3x3 / stride-1 convolution, final_linear on its linear head, the image packing and the bias gradient on disc.hip.
//   sg2_fir<ADJ>            upfirdn2d(x, outer(k, k), down d, pad (p0, p1)) on a channels-last map with a separable FIR of 2 .. 4 taps,
//                           and its adjoint (the input gradient): both gathers, each one's backward is the other
//   disc_sg2_conv_*         the convolutions behind the FIR, pad 0: 3x3 / stride 2 (conv2 of a ResBlock, on the blurred
//                           (H + 1) x (W + 1) map) and 1x1 / stride 1 (the skip, on the FIR's stride-2 output, and the input stage on
//                           the packed image): forward (+ bias + LeakyReLU + residual, the ResBlock's merge), input gradient, weight
//                           gradient and the weight packing, on the implicit-GEMM kernel and the host drivers of disc_conv_gemm.h
//                           (which disc_vgg.hip shares); here: the table of the two layers and the entry points
// No float atomics anywhere: two runs give the same bits.
#include "disc_conv_gemm.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// FIR.  kf = the taps as upfirdn2d applies them (the normalised 1-D kernel, flipped).  One thread per (pixel, 4 channels).
//   ADJ 0: out [N][Ho][Wo][C], out(oy, ox) = sum_{ky, kx} kf[ky] kf[kx] x(oy d + ky - p0, ox d + kx - p0)   (x [N][H][W][C])
//   ADJ 1: out [N][H][W][C],   out(iy, ix) = sum over (ky, kx) with (iy + p0 - ky) = d oy, (ix + p0 - kx) = d ox of
//                                             kf[ky] kf[kx] g(oy, ox)                                         (g [N][Ho][Wo][C])
// ---------------------------------------------------------------------------------------------------------------
struct Fir {
    float k[4];
    int L, p0, d;
};

template <int ADJ>
__global__ __launch_bounds__(256) void sg2_fir_kernel(const float *__restrict__ src, float *__restrict__ out, int N, int H, int W, int Ho, int Wo, int C,
                                                      const Fir f)
{
    const int C4 = C >> 2;
    const int Hd = ADJ ? H : Ho, Wd = ADJ ? W : Wo;   // the written map
    const int Hs = ADJ ? Ho : H, Ws = ADJ ? Wo : W;   // the read map
    const long total = (long)N * Hd * Wd * C4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = 4 * (int)(i % C4);
        long r = i / C4;
        const int x = (int)(r % Wd);
        r /= Wd;
        const int y = (int)(r % Hd);
        const long n = r / Hd;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int ky = 0; ky < f.L; ++ky) {
            int sy;
            if (ADJ) {
                const int t = y + f.p0 - ky;
                if (t < 0 || t % f.d) continue;
                sy = t / f.d;
            } else {
                sy = y * f.d + ky - f.p0;
            }
            if (sy < 0 || sy >= Hs) continue;
            for (int kx = 0; kx < f.L; ++kx) {
                int sx;
                if (ADJ) {
                    const int t = x + f.p0 - kx;
                    if (t < 0 || t % f.d) continue;
                    sx = t / f.d;
                } else {
                    sx = x * f.d + kx - f.p0;
                }
                if (sx < 0 || sx >= Ws) continue;
                const float wgt = f.k[ky] * f.k[kx];
                const float4 v = *reinterpret_cast<const float4 *>(src + ((n * Hs + sy) * Ws + sx) * C + c);
                acc.x += wgt * v.x, acc.y += wgt * v.y, acc.z += wgt * v.z, acc.w += wgt * v.w;
            }
        }
        *reinterpret_cast<float4 *>(out + ((n * Hd + y) * Wd + x) * C + c) = acc;
    }
}

// ------------------------------------------------------------------------------------------------- host side
const ConvLayer kLayers[] = {conv_layer<3, 2, 0>(), conv_layer<1, 1, 0>()};

int check_sconv(const char *what, int N, int H, int W, int Cin, int Cout, int ks, const ConvLayer *&L)
{
    L = find_layer(kLayers, ks);
    if (!L) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: kernel size %d (1: stride 1, 3: stride 2; pad 0)", what, ks);
    if (N <= 0 || H < ks || W < ks) return mrefsr::fail(MREFSR_E_INVALID, "%s: N=%d H=%d W=%d", what, N, H, W);
    return check_channels(what, Cin, Cout);
}

int fir_out(int n, int L, int p0, int p1, int d) { return (n + p0 + p1 - L) / d + 1; }

int check_fir(const char *what, int N, int H, int W, int C, const float *taps, int L, int p0, int p1, int d)
{
    if (!taps || L < 2 || L > 4) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: a separable FIR of 2 .. 4 taps (got %d)", what, L);
    if (d != 1 && d != 2) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: down=%d (1 or 2)", what, d);
    if (p0 < 0 || p1 < 0 || p0 >= L || p1 >= L) return mrefsr::fail(MREFSR_E_INVALID, "%s: pad (%d, %d) for %d taps", what, p0, p1, L);
    if (N <= 0 || C <= 0 || C % 4) return mrefsr::fail(MREFSR_E_UNSUPPORTED, "%s: N=%d C=%d (C a multiple of 4)", what, N, C);
    if (H + p0 + p1 < L || W + p0 + p1 < L) return mrefsr::fail(MREFSR_E_INVALID, "%s: H=%d W=%d", what, H, W);
    return MREFSR_OK;
}

Fir make_fir(const float *taps, int L, int p0, int d)
{
    Fir f = {{0.f, 0.f, 0.f, 0.f}, L, p0, d};
    for (int i = 0; i < L; ++i) f.k[i] = taps[L - 1 - i];   // upfirdn2d convolves: the kernel is applied flipped
    return f;
}

}  // namespace

MREFSR_EXPORT int mrefsr_disc_sg2_fir_f32(const float *x, float *y, int N, int H, int W, int C, const float *taps, int L, int pad0, int pad1, int down,
                                          int adjoint, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && y, "disc_sg2_fir: null pointer");
    int rc = check_fir("disc_sg2_fir", N, H, W, C, taps, L, pad0, pad1, down);
    if (rc) return rc;
    const int Ho = fir_out(H, L, pad0, pad1, down), Wo = fir_out(W, L, pad0, pad1, down);
    const Fir f = make_fir(taps, L, pad0, down);
    const long total = (long)N * (adjoint ? (long)H * W : (long)Ho * Wo) * (C / 4);
    const dim3 grid(grid_of((total + 255) / 256, 16384));
    if (adjoint) hipLaunchKernelGGL(sg2_fir_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, Ho, Wo, C, f);
    else hipLaunchKernelGGL(sg2_fir_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, Ho, Wo, C, f);
    return mrefsr::check_launch("disc_sg2_fir");
}

MREFSR_EXPORT int mrefsr_disc_sg2_pack_weight_f32(const float *w, float *wpk, int Cout, int CinR, int Cin, int ks, int dgrad, mrefsr_stream_t stream)
{
    return conv_pack_weight("disc_sg2_pack_weight", find_layer(kLayers, ks), w, wpk, Cout, CinR, Cin, ks, dgrad, stream);
}

MREFSR_EXPORT int64_t mrefsr_disc_sg2_conv_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks, int dgrad)
{
    const ConvLayer *L;
    if (check_sconv("disc_sg2_conv_workspace_bytes", N, H, W, Cin, Cout, ks, L)) return -1;
    return conv_workspace_bytes(*L, N, H, W, Cin, Cout, dgrad);
}

MREFSR_EXPORT int mrefsr_disc_sg2_conv_f32(const float *x, const float *wpk, const float *bias, const float *res, float *y, int N, int H, int W, int Cin,
                                           int Cout, int ks, int act, float slope, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && wpk && y, "disc_sg2_conv: null pointer");
    const ConvLayer *L;
    int rc = check_sconv("disc_sg2_conv", N, H, W, Cin, Cout, ks, L);
    if (rc) return rc;
    return conv_run("disc_sg2_conv", *L, 0, x, wpk, bias, res, y, N, H, W, Cin, Cout, act, slope, workspace, workspace_bytes, stream);
}

MREFSR_EXPORT int mrefsr_disc_sg2_conv_dgrad_f32(const float *dy, const float *wpk_d, float *dx, int N, int H, int W, int Cin, int Cout, int ks,
                                                 void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(dy && wpk_d && dx, "disc_sg2_conv_dgrad: null pointer");
    const ConvLayer *L;
    int rc = check_sconv("disc_sg2_conv_dgrad", N, H, W, Cin, Cout, ks, L);
    if (rc) return rc;
    return conv_run("disc_sg2_conv_dgrad", *L, 1, dy, wpk_d, nullptr, nullptr, dx, N, H, W, Cin, Cout, 0, 0.f, workspace, workspace_bytes, stream);
}

MREFSR_EXPORT int64_t mrefsr_disc_sg2_conv_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks)
{
    const ConvLayer *L;
    if (check_sconv("disc_sg2_conv_wgrad_workspace_bytes", N, H, W, Cin, Cout, ks, L)) return -1;
    return conv_wgrad_workspace_bytes(*L, N, H, W, Cin, Cout);
}

MREFSR_EXPORT int mrefsr_disc_sg2_conv_wgrad_f32(const float *x, const float *dy, float *dw, int N, int H, int W, int Cin, int CinR, int Cout, int ks,
                                                 void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && dy && dw && workspace, "disc_sg2_conv_wgrad: null pointer");
    const ConvLayer *L;
    int rc = check_sconv("disc_sg2_conv_wgrad", N, H, W, Cin, Cout, ks, L);
    if (rc) return rc;
    return conv_wgrad("disc_sg2_conv_wgrad", *L, x, dy, dw, N, H, W, Cin, CinR, Cout, workspace, workspace_bytes, stream);
}
