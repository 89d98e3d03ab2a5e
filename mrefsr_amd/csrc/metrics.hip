// Validation metrics on the device: tensor2img's uint8 quantisation, PSNR (RGB), PSNR-Y and SSIM (Y or per RGB channel) of
// mrefsr_amd/metrics.py (basicsr/utils/img_util.py:38-94, basicsr/metrics/psnr_ssim.py).
//
// Per batch (of at most VM_CHUNK images; larger batches run chunk by chunk into the same result rows):
//   quant_kernel     one pass over every output pixel: the uint8 values of output and GT (-> workspace planes, and the output's HWC
//                    image when asked), per block the exact int64 sum of squared RGB differences, the fp64 sum of squared Y
//                    differences over the cropped region, and the count of non-finite inputs in the valid region;
//   ssim_kernel      the SSIM map of one 32 x 16 tile of one image and one channel (Y, R, G or B): the uint8 tile + a 10-pixel halo
//                    to LDS as fp64, the 11-tap Gaussian "valid" filter down the columns, then along the rows, of x, y, x^2, y^2
//                    and xy; per block the fp64 sum of the map values;
//   finish_kernel    one block per image adds the per-block partials in a fixed order into the image's result row.
// Every reduction is per thread in a fixed sequence, then a fixed LDS tree: no atomics, so two runs give the same bits.
//
// This file is built with -ffp-contract=off: each fp64 product and sum is rounded on its own, in the order numpy evaluates
// metrics.py (rgb_to_y's dot, whose float64 BLAS kernel is an FMA chain, is written with explicit fma).  The filtered maps then
// equal numpy's bit for bit; only the final sums (numpy: pairwise) differ in order.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int VM_THREADS = 256;
constexpr int VM_CHUNK = 32;          // images per launch (their valid regions travel in the kernel arguments)
constexpr int TX = 32, TY = 16;       // SSIM output tile
constexpr int KS = 11, HALO = KS - 1;
constexpr int LX = TX + HALO, LY = TY + HALO;
constexpr int RES_WORDS = 8;          // result row: see mrefsr_val_metrics_f32 in the header

struct Geo {
    int H, W;         // output tensor
    int Hg, Wg;       // GT tensor
    int cb;           // crop_border
    int nblk1;        // quant_kernel blocks per image
    int tiles_x, tiles_y, tile_stride;
};

struct Regions {
    int oh[VM_CHUNK], ow[VM_CHUNK];
};

struct SsimConst {
    double k[KS];     // Gaussian taps (metrics._gaussian_window)
    double c1, c2;
};

struct Part1 {
    long long sse;
    double sse_y;
    long long nonfinite;
};

__device__ __forceinline__ unsigned char quantise(float v)
{
    // torch clamp_(0, 1), numpy `img * 255.0` in float32, .round() (half to even), astype(uint8)
    return (unsigned char)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f);
}

// tab[v] = float32(v) / 255 as metrics.rgb_to_y computes it (float32 division), widened to fp64.  The fp64 quotient rounded to
// float is the correctly rounded float quotient: v / 255 has the 8-bit period of v in binary, so it never sits on a float midpoint.
__device__ __forceinline__ void fill_ytab(double *tab)
{
    for (int v = threadIdx.x; v < 256; v += blockDim.x) tab[v] = (double)(float)((double)v / 255.0);
}

// metrics.rgb_to_y: (dot(rgb / 255, [65.481, 128.553, 24.966]) + 16) / 255 * 255, in numpy's order
__device__ __forceinline__ double y_of(const double *tab, int r, int g, int b)
{
    const double d = fma(tab[b], 24.966, fma(tab[g], 128.553, tab[r] * 65.481));
    return (d + 16.0) / 255.0 * 255.0;
}

// grid (nblk1, images of the chunk).  Pixels of one image are visited p = blockIdx.x * 256 + tid + k * nblk1 * 256.
template <bool IMG>
__global__ __launch_bounds__(VM_THREADS) void quant_kernel(const float *__restrict__ out, const float *__restrict__ gt,
                                                           unsigned char *__restrict__ q, unsigned char *__restrict__ img,
                                                           Part1 *__restrict__ part, Geo g, Regions rg)
{
    __shared__ double ytab[256];
    __shared__ long long red_i[VM_THREADS];
    __shared__ double red_d[VM_THREADS];
    fill_ytab(ytab);
    __syncthreads();
    const int i = blockIdx.y, oh = rg.oh[i], ow = rg.ow[i], cb = g.cb;
    const long HW = (long)g.H * g.W, HWg = (long)g.Hg * g.Wg;
    const float *o = out + (long)i * 3 * HW, *t = gt + (long)i * 3 * HWg;
    unsigned char *qo = q + (long)i * 6 * HW, *qg = qo + 3 * HW;
    long long sse = 0, bad = 0;
    double sse_y = 0.0;
    for (long p = (long)blockIdx.x * VM_THREADS + threadIdx.x; p < HW; p += (long)g.nblk1 * VM_THREADS) {
        const int r = (int)(p / g.W), c = (int)(p - (long)r * g.W);
        float xo[3];
        unsigned char uo[3];
        for (int ch = 0; ch < 3; ++ch) {
            xo[ch] = o[ch * HW + p];
            uo[ch] = quantise(xo[ch]);
        }
        if (IMG) {
            unsigned char *d = img + ((long)i * HW + p) * 3;
            d[0] = uo[0], d[1] = uo[1], d[2] = uo[2];
        }
        if (r >= oh || c >= ow) continue;
        const long pg = (long)r * g.Wg + c;
        unsigned char ug[3];
        for (int ch = 0; ch < 3; ++ch) {
            const float xg = t[ch * HWg + pg];
            ug[ch] = quantise(xg);
            bad += !isfinite(xo[ch]) + !isfinite(xg);
            qo[ch * HW + p] = uo[ch];
            qg[ch * HW + p] = ug[ch];
        }
        if (r < cb || r >= oh - cb || c < cb || c >= ow - cb) continue;
        for (int ch = 0; ch < 3; ++ch) {
            const int d = (int)uo[ch] - (int)ug[ch];
            sse += d * d;
        }
        const double dy = y_of(ytab, uo[0], uo[1], uo[2]) - y_of(ytab, ug[0], ug[1], ug[2]);
        sse_y += dy * dy;
    }
    sse = mrefsr::block_sum<VM_THREADS>(red_i, sse);
    bad = mrefsr::block_sum<VM_THREADS>(red_i, bad);
    sse_y = mrefsr::block_sum<VM_THREADS>(red_d, sse_y);
    if (threadIdx.x == 0) part[(long)i * g.nblk1 + blockIdx.x] = Part1{sse, sse_y, bad};
}

// tensor2img alone: x [N][C][H][W] -> img [N][H][W][C]
__global__ __launch_bounds__(VM_THREADS) void tensor2img_kernel(const float *__restrict__ x, unsigned char *__restrict__ img, long HW, int C,
                                                                long total)
{
    for (long e = (long)blockIdx.x * VM_THREADS + threadIdx.x; e < total; e += (long)gridDim.x * VM_THREADS) {
        const long n = e / (HW * C), rem = e - n * HW * C, p = rem / C;
        const int ch = (int)(rem - p * C);
        img[e] = quantise(x[(n * C + ch) * HW + p]);
    }
}

// grid (tiles, channel slots, images of the chunk).  Slot 0 = Y, 1..3 = R, G, B; blockIdx.y + slot0 is the slot.
__global__ __launch_bounds__(VM_THREADS) void ssim_kernel(const unsigned char *__restrict__ q, double *__restrict__ part, Geo g, Regions rg,
                                                          SsimConst sc, int slot0)
{
    __shared__ double ytab[256];
    __shared__ double sx[LY][LX], sy[LY][LX];
    __shared__ double vf[5][TY][LX];   // column-filtered x, y, x^2, y^2, xy
    __shared__ double red[VM_THREADS];
    const int i = blockIdx.z, slot = blockIdx.y + slot0, tile = blockIdx.x;
    const int cb = g.cb, h = rg.oh[i] - 2 * cb, w = rg.ow[i] - 2 * cb, mh = h - HALO, mw = w - HALO;
    const int oy0 = (tile / g.tiles_x) * TY, ox0 = (tile % g.tiles_x) * TX;
    double *dst = part + ((long)i * 4 + slot) * g.tile_stride + tile;
    if (oy0 >= mh || ox0 >= mw) {      // a tile past this image's map (another image of the chunk is larger)
        if (threadIdx.x == 0) *dst = 0.0;
        return;
    }
    fill_ytab(ytab);
    __syncthreads();
    const long HW = (long)g.H * g.W;
    const unsigned char *qo = q + (long)i * 6 * HW, *qg = qo + 3 * HW;
    for (int e = threadIdx.x; e < LY * LX; e += VM_THREADS) {
        const int ly = e / LX, lx = e - ly * LX, gy = oy0 + ly, gx = ox0 + lx;
        double a = 0.0, b = 0.0;
        if (gy < h && gx < w) {
            const long p = (long)(gy + cb) * g.W + gx + cb;
            if (slot == 0) {
                a = y_of(ytab, qo[p], qo[HW + p], qo[2 * HW + p]);
                b = y_of(ytab, qg[p], qg[HW + p], qg[2 * HW + p]);
            } else {
                a = (double)qo[(slot - 1) * HW + p];
                b = (double)qg[(slot - 1) * HW + p];
            }
        }
        sx[ly][lx] = a;
        sy[ly][lx] = b;
    }
    __syncthreads();
    // metrics._filter_valid, first axis: sum(k[i] * img[i + r]) from 0, i ascending; the squares and the product are formed first
    for (int e = threadIdx.x; e < TY * LX; e += VM_THREADS) {
        const int r = e / LX, c = e - r * LX;
        double m1 = 0.0, m2 = 0.0, q11 = 0.0, q22 = 0.0, q12 = 0.0;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const double a = sx[r + k][c], b = sy[r + k][c], wk = sc.k[k];
            m1 = m1 + wk * a;
            m2 = m2 + wk * b;
            q11 = q11 + wk * (a * a);
            q22 = q22 + wk * (b * b);
            q12 = q12 + wk * (a * b);
        }
        vf[0][r][c] = m1, vf[1][r][c] = m2, vf[2][r][c] = q11, vf[3][r][c] = q22, vf[4][r][c] = q12;
    }
    __syncthreads();
    double acc = 0.0;
    for (int e = threadIdx.x; e < TY * TX; e += VM_THREADS) {
        const int r = e / TX, c = e - r * TX;
        if (oy0 + r >= mh || ox0 + c >= mw) continue;
        double f[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < KS; ++k)
            for (int j = 0; j < 5; ++j) f[j] = f[j] + sc.k[k] * vf[j][r][c + k];
        // metrics._ssim
        const double mu1_sq = f[0] * f[0], mu2_sq = f[1] * f[1], mu1_mu2 = f[0] * f[1];
        const double s1 = f[2] - mu1_sq, s2 = f[3] - mu2_sq, s12 = f[4] - mu1_mu2;
        acc += ((2.0 * mu1_mu2 + sc.c1) * (2.0 * s12 + sc.c2)) / ((mu1_sq + mu2_sq + sc.c1) * (s1 + s2 + sc.c2));
    }
    acc = mrefsr::block_sum<VM_THREADS>(red, acc);
    if (threadIdx.x == 0) *dst = acc;
}

// one block per image of the chunk: res[img0 + i] from the partials of both kernels
__global__ __launch_bounds__(VM_THREADS) void finish_kernel(const Part1 *__restrict__ part1, const double *__restrict__ part2,
                                                            long long *__restrict__ res, Geo g, int slot0, int slot1, int ntiles)
{
    __shared__ long long red_i[VM_THREADS];
    __shared__ double red_d[VM_THREADS];
    const int i = blockIdx.x;
    const Part1 *p1 = part1 + (long)i * g.nblk1;
    long long sse = 0, bad = 0;
    double sse_y = 0.0;
    for (int b = threadIdx.x; b < g.nblk1; b += VM_THREADS) {
        sse += p1[b].sse;
        bad += p1[b].nonfinite;
        sse_y += p1[b].sse_y;
    }
    sse = mrefsr::block_sum<VM_THREADS>(red_i, sse);
    bad = mrefsr::block_sum<VM_THREADS>(red_i, bad);
    sse_y = mrefsr::block_sum<VM_THREADS>(red_d, sse_y);
    double ssim[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = slot0; s < slot1; ++s) {
        const double *p2 = part2 + ((long)i * 4 + s) * g.tile_stride;
        double a = 0.0;
        for (int b = threadIdx.x; b < ntiles; b += VM_THREADS) a += p2[b];
        ssim[s] = mrefsr::block_sum<VM_THREADS>(red_d, a);
    }
    if (threadIdx.x == 0) {
        long long *row = res + (long)i * RES_WORDS;
        row[0] = sse;
        row[1] = bad;
        row[2] = __double_as_longlong(sse_y);
        for (int s = 0; s < 4; ++s) row[3 + s] = __double_as_longlong(ssim[s]);
        row[7] = 0;
    }
}

int nblk1_of(long HW) { return (int)std::min<long>((HW + 4 * VM_THREADS - 1) / (4 * VM_THREADS), 1024); }
int tiles_of(int n, int t) { return n > HALO ? (n - HALO + t - 1) / t : 0; }

struct Layout {
    int chunk, nblk1, tile_stride;
    int64_t part1, part2, planes, total;   // byte offsets
};

Layout layout_of(int N, int H, int W)
{
    Layout L;
    L.chunk = std::min(N, VM_CHUNK);
    L.nblk1 = nblk1_of((long)H * W);
    L.tile_stride = std::max(1, tiles_of(H, TY) * tiles_of(W, TX));
    L.part1 = 0;
    L.part2 = L.part1 + (int64_t)L.chunk * L.nblk1 * (int64_t)sizeof(Part1);
    L.planes = L.part2 + (int64_t)L.chunk * 4 * L.tile_stride * 8;
    L.total = L.planes + (int64_t)L.chunk * 6 * H * W;
    return L;
}

// metrics._gaussian_window (numpy: k / k.sum(), the sum of 11 values taken as ((k0+k1)+(k2+k3))+((k4+k5)+(k6+k7)), then +k8+k9+k10)
// and the constants of metrics._ssim
SsimConst ssim_const()
{
    SsimConst sc;
    double e[KS];
    for (int j = 0; j < KS; ++j) {
        const double x = (double)j - (KS - 1) / 2.0;
        e[j] = std::exp(-(x * x) / (2.0 * 1.5 * 1.5));
    }
    double s = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
    s = s + e[8];
    s = s + e[9];
    s = s + e[10];
    for (int j = 0; j < KS; ++j) sc.k[j] = e[j] / s;
    const double a = 0.01 * 255, b = 0.03 * 255;
    sc.c1 = a * a;
    sc.c2 = b * b;
    return sc;
}

}  // namespace

MREFSR_EXPORT int64_t mrefsr_val_metrics_workspace_bytes(int N, int H, int W)
{
    if (N <= 0 || H <= 0 || W <= 0) return -1;
    return layout_of(N, H, W).total;
}

MREFSR_EXPORT int mrefsr_val_metrics_f32(const float *out, const float *gt, int N, int H, int W, int Hg, int Wg, const int *sizes,
                                         int crop_border, int flags, unsigned char *img, int64_t *res, void *workspace,
                                         int64_t workspace_bytes, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(out && gt && res && workspace, "val_metrics: null pointer");
    MREFSR_REQUIRE(N > 0 && H > 0 && W > 0 && Hg > 0 && Wg > 0, "val_metrics: N=%d output %dx%d GT %dx%d", N, H, W, Hg, Wg);
    MREFSR_REQUIRE(crop_border >= 0, "val_metrics: crop_border=%d", crop_border);
    MREFSR_REQUIRE((flags & ~(MREFSR_VALM_SSIM_Y | MREFSR_VALM_SSIM_RGB)) == 0, "val_metrics: flags=%d", flags);
    MREFSR_REQUIRE(sizes || (H == Hg && W == Wg), "val_metrics: output %dx%d and GT %dx%d differ and no valid sizes are given", H, W, Hg, Wg);
    const int min_side = flags ? KS : 1;
    for (int i = 0; i < N; ++i) {
        const int oh = sizes ? sizes[2 * i] : H, ow = sizes ? sizes[2 * i + 1] : W;
        MREFSR_REQUIRE(oh > 0 && ow > 0 && oh <= std::min(H, Hg) && ow <= std::min(W, Wg),
                       "val_metrics: image %d: valid region %dx%d outside output %dx%d / GT %dx%d", i, oh, ow, H, W, Hg, Wg);
        MREFSR_REQUIRE(oh - 2 * crop_border >= min_side && ow - 2 * crop_border >= min_side,
                       "val_metrics: image %d: %dx%d less crop_border %d leaves %dx%d (at least %dx%d)", i, oh, ow, crop_border,
                       oh - 2 * crop_border, ow - 2 * crop_border, min_side, min_side);
    }
    const Layout L = layout_of(N, H, W);
    MREFSR_REQUIRE(workspace_bytes >= L.total, "val_metrics: workspace of %ld bytes < %ld", (long)workspace_bytes, (long)L.total);
    char *ws = (char *)workspace;
    Part1 *part1 = (Part1 *)(ws + L.part1);
    double *part2 = (double *)(ws + L.part2);
    unsigned char *planes = (unsigned char *)(ws + L.planes);
    const int slot0 = (flags & MREFSR_VALM_SSIM_Y) ? 0 : 1, slot1 = (flags & MREFSR_VALM_SSIM_RGB) ? 4 : 1;
    const SsimConst sc = ssim_const();
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)H * W, HWg = (long)Hg * Wg;
    for (int i0 = 0; i0 < N; i0 += VM_CHUNK) {
        const int n = std::min(VM_CHUNK, N - i0);
        Regions rg;
        int mh = 0, mw = 0;
        for (int i = 0; i < VM_CHUNK; ++i) {
            rg.oh[i] = i < n ? (sizes ? sizes[2 * (i0 + i)] : H) : 0;
            rg.ow[i] = i < n ? (sizes ? sizes[2 * (i0 + i) + 1] : W) : 0;
            if (i < n) {
                mh = std::max(mh, rg.oh[i] - 2 * crop_border);
                mw = std::max(mw, rg.ow[i] - 2 * crop_border);
            }
        }
        Geo g = {H, W, Hg, Wg, crop_border, L.nblk1, tiles_of(mw, TX), tiles_of(mh, TY), L.tile_stride};
        const float *o = out + (long)i0 * 3 * HW, *t = gt + (long)i0 * 3 * HWg;
        unsigned char *im = img ? img + (long)i0 * HW * 3 : nullptr;
        if (im)
            hipLaunchKernelGGL(quant_kernel<true>, dim3(L.nblk1, n), dim3(VM_THREADS), 0, st, o, t, planes, im, part1, g, rg);
        else
            hipLaunchKernelGGL(quant_kernel<false>, dim3(L.nblk1, n), dim3(VM_THREADS), 0, st, o, t, planes, im, part1, g, rg);
        const int ntiles = flags ? g.tiles_x * g.tiles_y : 0;
        if (flags)
            hipLaunchKernelGGL(ssim_kernel, dim3(ntiles, slot1 - slot0, n), dim3(VM_THREADS), 0, st, planes, part2, g, rg, sc, slot0);
        hipLaunchKernelGGL(finish_kernel, dim3(n), dim3(VM_THREADS), 0, st, part1, part2, (long long *)res + (long)i0 * RES_WORDS, g,
                           flags ? slot0 : 0, flags ? slot1 : 0, ntiles);
        int rc = mrefsr::check_launch("val_metrics");
        if (rc) return rc;
    }
    return MREFSR_OK;
}

MREFSR_EXPORT int mrefsr_tensor2img_u8(const float *x, unsigned char *img, int N, int C, int H, int W, mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(x && img, "tensor2img: null pointer");
    MREFSR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "tensor2img: N=%d C=%d H=%d W=%d", N, C, H, W);
    const long HW = (long)H * W, total = (long)N * C * HW;
    const int blocks = (int)std::min<long>((total + VM_THREADS - 1) / VM_THREADS, 8192);
    hipLaunchKernelGGL(tensor2img_kernel, dim3(blocks), dim3(VM_THREADS), 0, (hipStream_t)stream, x, img, HW, C, total);
    return mrefsr::check_launch("tensor2img");
}
