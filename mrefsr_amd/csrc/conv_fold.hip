// Composition of convolution weights that stand in a row with nothing non-linear between them, done once per weight version
// (next to the pack kernels of conv_nhwc.hip; the result is packed like any other weight).
//
// 1x1 after 3x3 -- MRAPAFusion's spatial_attn_add2 followed by the reference half of feat_fusion (ref_mrapa_restoration_arch.py:
// 338-347): Wf_r . (W2 * a + b2) = (Wf_r . W2) * a + Wf_r . b2, zero padding included (the 1x1 acts after it).  The sums run in
// double in ascending m; a product of two floats is exact in double, so every element is the double sum of exact terms in a
// fixed order, rounded to float once.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void conv_compose_1x1_3x3_kernel(const float *__restrict__ w1, long ld1, int off, const float *__restrict__ w3,
                                                                   const float *__restrict__ b3, const float *__restrict__ b1,
                                                                   float *__restrict__ out_w, float *__restrict__ out_b, int Cout, int Cmid, int Cin)
{
    const long row = (long)Cin * 9, n_w = (long)Cout * row, total = n_w + (out_b ? Cout : 0);
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        if (e < n_w) {   // out_w[o][i][tap]: consecutive threads read consecutive (i, tap) of every w3 row, the w1 element is a broadcast
            const long o = e / row, it = e - o * row;
            const float *a = w1 + o * ld1 + off, *b = w3 + it;
            double s = 0.0;
            for (int m = 0; m < Cmid; ++m) s += (double)a[m] * (double)b[m * row];
            out_w[e] = (float)s;
        } else {         // out_b[o] = b1[o] + sum_m w1[o][off + m] b3[m]
            const long o = e - n_w;
            const float *a = w1 + o * ld1 + off;
            double s = b1 ? (double)b1[o] : 0.0;
            if (b3)
                for (int m = 0; m < Cmid; ++m) s += (double)a[m] * (double)b3[m];
            out_b[o] = (float)s;
        }
    }
}

}  // namespace

MREFSR_EXPORT int mrefsr_conv_compose_1x1_3x3_f32(const float *w1x1, int64_t ld_1x1, int cin_offset, const float *w3x3, const float *b3x3,
                                                  const float *b1x1, float *out_w, float *out_b, int Cout, int Cmid, int Cin,
                                                  mrefsr_stream_t stream)
{
    MREFSR_REQUIRE(w1x1 && w3x3 && out_w, "conv_compose_1x1_3x3: null pointer");
    MREFSR_REQUIRE(Cout > 0 && Cmid > 0 && Cin > 0, "conv_compose_1x1_3x3: Cout=%d Cmid=%d Cin=%d", Cout, Cmid, Cin);
    MREFSR_REQUIRE(cin_offset >= 0 && (int64_t)cin_offset + Cmid <= ld_1x1, "conv_compose_1x1_3x3: columns [%d, %d + %d) of a 1x1 row of %ld", cin_offset,
                   cin_offset, Cmid, (long)ld_1x1);
    const long total = (long)Cout * Cin * 9 + (out_b ? Cout : 0);
    hipLaunchKernelGGL(conv_compose_1x1_3x3_kernel, dim3(mrefsr::grid_of((total + 255) / 256, 16384)), dim3(256), 0, (hipStream_t)stream, w1x1,
                       (long)ld_1x1, cin_offset, w3x3, b3x3, b1x1, out_w, out_b, Cout, Cmid, Cin);
    return mrefsr::check_launch("conv_compose_1x1_3x3");
}
