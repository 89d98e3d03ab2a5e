/*
 * mrefsr_hip.h -- C ABI of libmrefsr_hip.so: the MI355X (gfx950) kernels of the MRefSR
 * multi-reference matching-and-reconstruction hot path.
 *
 * Conventions
 *   - plain C, no torch / ATen types: raw DEVICE pointers + sizes + a hipStream_t passed as void*.
 *   - every function enqueues work on `stream` and returns immediately: 0 = ok, <0 = MREFSR_E_*.
 *     mrefsr_last_error() gives the message for the calling thread.  Nothing allocates device
 *     memory; scratch is caller-provided (size queries are separate entry points).
 *   - thread-safe: no mutable globals besides the thread-local error string.
 *   - tensors are dense row-major fp32 unless stated; "HW" = H*W.
 *
 * Each entry cites the reference interface it replaces (paths relative to the reference repo).
 */
#ifndef MREFSR_HIP_H
#define MREFSR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MREFSR_ABI_VERSION 1

enum {
    MREFSR_OK = 0,
    MREFSR_E_INVALID = -1,     /* bad argument (null pointer, non-positive size, unsupported combo) */
    MREFSR_E_UNSUPPORTED = -2, /* shape outside what the kernels implement (message says which)    */
    MREFSR_E_LAUNCH = -3       /* hipGetLastError() after the launch                               */
};

typedef void *mrefsr_stream_t; /* hipStream_t */

int mrefsr_abi_version(void);
const char *mrefsr_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Correlation path: basicsr/archs/corres_generation_arch.py:53-68 + basicsr/archs/ref_map_util.py
 * --------------------------------------------------------------------------------------------- */

/* Padded channel count of the pixel-major feature layout used by the correlation kernel
 * (multiple of 64).  Returns <0 if C is unsupported (C > 256). */
int mrefsr_corr_padded_channels(int C);

/* Per-pixel channel L2 normalisation + transposition to the pixel-major "split" layout.
 * Replaces F.normalize(feat.reshape(c,-1), dim=0)  (corres_generation_arch.py:57-59) and the
 * unfold of sample_patches (ref_map_util.py:4-23, never materialised here).
 *   x  [N][C][HW]           raw features (VGG16 conv3_1); x_nhwc = 1: [N][HW][C] fp32; x_nhwc = 2: [N][HW][C] bf16 (the
 *                           2-byte activation storage of BASELINE configs[4], passed through the same pointer)
 *   y  [N][HW][Cp]          Cp = mrefsr_corr_padded_channels(C); element (p, c) lives at
 *                           p*Cp + (c&1)*(Cp/2) + (c>>1); channels >= C are zero
 *   n2 [N][HW]              sum over c of y^2 (fmaf chain, c ascending)
 *   ybf                     NULL, or the operand of the pre-filter correlation pass, natural channel order:
 *                           ybf_fmt 0: [N][HW][2][Cp] bf16, two-term split y = hi + lo (hi = bf16(y), lo = bf16(y - hi))
 *                           ybf_fmt 1: [N][HW][Cp] fp16, yh = fp16(y)
 *   normalize               1: y = x / max(||x||, 1e-12) (the path); 0: y = x (layout change only,
 *                           for callers of feature_match_index that pass un-normalised maps)
 *   d2 [N][HW]              NULL, or sum over c of (y - fp16(y))^2: the squared norm of the rounding error of the
 *                           fp16 operand, from which the caller derives the pre-filter window (`tau` below)     */
int mrefsr_pixnorm_f32(const float *x, float *y, float *n2, void *ybf, int N, int C, int HW,
                       int normalize, int x_nhwc, int ybf_fmt, float *d2, mrefsr_stream_t stream);

/* 3x3 patch norms: batch.norm(p=2, dim=(0,1,2)) + 1e-5  (ref_map_util.py:62-63, :79-80).
 *   n2 [N][h][w] -> nrm_eps [N][h-2][w-2] = sqrt(sum of 9) + 1e-5 ; inv = 1 / nrm_eps
 * either output may be NULL. */
int mrefsr_patch_norm_f32(const float *n2, float *nrm_eps, float *inv, int N, int h, int w,
                          mrefsr_stream_t stream);

/* Fused 3x3-patch correlation + top-1:  feature_match_index(feat_in, feat_ref, patch_size=3,
 * input_stride=1, ref_stride=1, is_norm=True, norm_input=True)  (ref_map_util.py:26-86); the
 * (n_ref_patches x n_query) correlation matrix (:64-67) is never written to memory.
 *   y_in     [n_in ][h*w][Cp]   from mrefsr_pixnorm_f32
 *   y_ref    [n_pair][h*w][Cp]
 *   inv_ref  [n_pair][(h-2)(w-2)]  from mrefsr_patch_norm_f32 on the ref n2
 *   nrm_in   [n_in ][(h-2)(w-2)]   nrm_eps of the input n2
 *   max_idx  [n_pair][(h-2)(w-2)] int64, value ry*(w-2)+rx, lowest index on exact ties
 *   max_val  [n_pair][(h-2)(w-2)] fp32 or NULL (max corr / nrm_in, ref_map_util.py:78-84)
 * pair p matches input (p % n_in) against ref p, so refs stacked [K][B] batch in one launch.
 * C <= 256 (Cp = padded), h, w >= 3. */
int mrefsr_corr_top1_f32(const float *y_in, const float *y_ref, const float *inv_ref,
                         const float *nrm_in, int64_t *max_idx, float *max_val, int n_in,
                         int n_pair, int Cp, int h, int w, mrefsr_stream_t stream);

/* feature_match_index in its general form (ref_map_util.py:26-86): any patch_size, input_stride, ref_stride, input and
 * reference maps of different sizes, is_norm / norm_input as in the reference.  feat_in [C][h][w], feat_ref [C][hr][wr] as given
 * (NCHW, not re-laid out); max_idx [nqy*nqx] int64 = ry*nrx + rx (n = (size - patch) / stride + 1), lowest index on exact ties;
 * max_val [nqy*nqx] or NULL.  Same defined operation order as mrefsr_corr_top1_f32 (per-tap fmaf chains over the channels,
 * taps added row-major, one multiply by 1 / (||ref patch|| + 1e-5)): with patch 3, strides 1 and equal sizes it returns that
 * entry's bits.  A scalar-FMA kernel, O(n_q n_r patch^2 C): the general entry, not the benchmark's path.
 * workspace: mrefsr_feature_match_index_workspace_bytes(h, w, hr, wr) bytes of device memory. */
int64_t mrefsr_feature_match_index_workspace_bytes(int h, int w, int hr, int wr);
int mrefsr_feature_match_index_f32(const float *feat_in, const float *feat_ref, int C, int h, int w, int hr, int wr, int patch,
                                   int stride_in, int stride_ref, int is_norm, int norm_input, int64_t *max_idx, float *max_val,
                                   void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);

/* Same result, fast path: approximate MFMA pre-filter (candidates within a proven error window of
 * the approximate maximum) + exact fp32 re-scoring of the candidates in the canonical operation
 * order + brute force for queries whose candidate set overflows.  Indices and values are
 * bit-identical to mrefsr_corr_top1_f32.  ybf_* from mrefsr_pixnorm_f32 in format ybf_fmt:
 *   0  bf16 hi|lo two-term split, three bf16 MFMAs per term (any Cp)
 *   1  fp16 single plane, one fp16 MFMA per term (Cp = 256 only).  Window: `tau` [n_pair][(h-2)(w-2)], a proven bound
 *      per query on twice the error of an approximate score, i.e. with d = sqrt(d2) per pixel, D = 3x3 patch norm
 *      of d (mrefsr_patch_norm_f32 on d2), rho = max over the pair's reference patches of D_ref * inv_ref:
 *          tau = 2.02 * (D_in + (nrm_in + 3 D_in) * rho) + 2e-4 * nrm_in
 *      (Cauchy-Schwarz on y_a y_b - h_a h_b = d_a.h_b + h_a.d_b + d_a.d_b over channels and taps, + 1e-4 nrm_in for
 *      the fp32 accumulation orders).  tau = NULL: the worst-case window 2.02 * 1.1e-3 * nrm_in, 2-4x
 *      wider -- more candidates, overflow -> brute force on maps full of near-ties.
 * workspace of mrefsr_corr_workspace_bytes(n_pair, h, w) bytes.
 * ybf_ref must be followed by at least (6*w + 16) pixels of readable bytes (6 image rows + 16 pixels,
 * i.e. (6*w + 16)*2*Cp*2 bytes in format 0, (6*w + 16)*Cp*2 in format 1): edge tiles (8 rows x 16
 * pixels from an origin <= (h-3, w-3)) are staged by LDS-DMA without clamping; what is read there
 * never reaches a valid patch. */
int64_t mrefsr_corr_workspace_bytes(int n_pair, int h, int w);
/* Which pre-filter kernel mrefsr_corr_top1_prefilter_f32 launches for these operands and how much matrix work it issues: the
 * MFMA FLOP per (sample, reference) pair (< 0: invalid arguments); kernel_name (may be NULL) receives the kernel's name,
 * *mfma_dtype (may be NULL) 1 for one fp16 MFMA per product, 0 for three bf16 MFMAs.  No reference counterpart: measurement
 * support (bench.py's roofline divides this figure by the measured time of the call). */
int64_t mrefsr_corr_prefilter_info(int ybf_fmt, int Cp, int h, int w, char *kernel_name, int name_len, int *mfma_dtype);
int mrefsr_corr_top1_prefilter_f32(const float *y_in, const float *y_ref, const void *ybf_in,
                                   const void *ybf_ref, const float *inv_ref, const float *nrm_in,
                                   int64_t *max_idx, float *max_val, void *workspace,
                                   int64_t workspace_bytes, int n_in, int n_pair, int Cp, int h,
                                   int w, int ybf_fmt, const float *tau, mrefsr_stream_t stream);

/* index -> flow -> 9 shifted offset planes at scales 1, 2, 4
 * (CorrespondenceGenerationArch.index_to_flow + forward, corres_generation_arch.py:30-47,:70-105;
 * tensor_shift arch_util.py:386-410).
 *   max_idx [N][(h-2)(w-2)] int64
 *   off_s   [N][9][s*h][s*w][2] fp32, last dim [x, y]; any of the three may be NULL */
int mrefsr_offsets_from_idx_f32(const int64_t *max_idx, float *off_s1, float *off_s2,
                                float *off_s4, int N, int h, int w, mrefsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * DynAgg glue: ref_mrapa_restoration_arch.py:56-73
 *   om  [B][3*dg*9][H][W]   output of conv_offset_mask (o1 | o2 | mask chunks); om_nhwc = 1: [B][H][W][3*dg*9]
 *   om_bias [3*dg*9] or NULL  bias of conv_offset_mask when the convolution ran without it
 *   pre [B][9][H][W][2]     pre-computed offsets, last dim [x, y]
 *   offset [B][dg*18][H][W] = om[:, :dg*18] + pre re-ordered to [y, x] per tap (:59-67)
 *   mask   [B][dg*9][H][W]  = sigmoid(om[:, dg*18:])                             (:69)
 *   abs_sum: device double[1], += sum |om[:, :dg*18]| (the :70-73 guard, no host sync); or NULL */
int mrefsr_dynagg_prep_f32(const float *om, const float *om_bias, const float *pre, float *offset,
                           float *mask, double *abs_sum, int B, int dg, int H, int W, int om_nhwc,
                           mrefsr_stream_t stream);

/* backward of the above: g_om[:, :dg*18] = g_offset ; g_om[:, dg*18:] = g_mask * m * (1 - m) */
int mrefsr_dynagg_prep_bwd_f32(const float *g_offset, const float *g_mask, const float *mask,
                               float *g_om, int B, int dg, int H, int W, mrefsr_stream_t stream);
/* The same with g_om channels-last, [B][H*W][27*dg] -- the layout the input-gradient / weight-gradient kernels of conv_offset_mask
 * read -- and its two reductions in the same pass: bias_grad[27*dg] += per-channel sums, amax[0] = max(amax[0], max |g_om|)
 * (both zero-initialised by the caller; either may be NULL).  27*dg <= 256. */
int mrefsr_dynagg_prep_bwd_nhwc_f32(const float *g_offset, const float *g_mask, const float *mask, float *g_om, float *bias_grad,
                                    float *amax, int B, int dg, int H, int W, mrefsr_stream_t stream);
/* The same, bitwise reproducible: every block writes its per-channel sums to its own row of `workspace`
 * ([mrefsr_dynagg_prep_bwd_blocks][27*dg] floats, workspace_bytes >= mrefsr_dynagg_prep_bwd_det_workspace_bytes), and the block
 * that finishes last adds the rows in ascending block order (image-major, then pixel tiles) into bias_grad -- a fixed order
 * instead of the float atomics above, in the same launch.  ticket[0] (device memory) is 0 before the first launch; the launch
 * leaves it 0 again, so it needs no memset between launches or graph replays.  One launch at a time per workspace / ticket.
 * g_om and amax as above, bit for bit. */
int mrefsr_dynagg_prep_bwd_blocks(int B, int dg, int H, int W);
int64_t mrefsr_dynagg_prep_bwd_det_workspace_bytes(int B, int dg, int H, int W);
int mrefsr_dynagg_prep_bwd_nhwc_det_f32(const float *g_offset, const float *g_mask, const float *mask, float *g_om, float *bias_grad,
                                        float *amax, int B, int dg, int H, int W, void *workspace, int64_t workspace_bytes,
                                        uint32_t *ticket, mrefsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * DCNv2 / DCNv1: basicsr/ops/dcn (deform_conv_ext: deform_conv_ext.cpp:52-147) and
 * mmcv.ops.modulated_deform_conv2d as called at ref_mrapa_restoration_arch.py:74-76.
 * Arithmetic spec: deform_conv_cuda_kernel.cu:467-767, deform_conv_cuda.cpp:490-685.
 *   x [B][C][H][W]; offset [B][dg*2*kh*kw][Ho][Wo] ([g][tap][y,x]); mask [B][dg*kh*kw][Ho][Wo]
 *   or NULL (DCNv1); weight [Co][C/groups][kh][kw]; bias [Co] or NULL; out [B][Co][Ho][Wo].
 *   act_slope: fused LeakyReLU slope applied to the output (1.0f = none).
 * --------------------------------------------------------------------------------------------- */
typedef struct {
    int B, C, H, W, Co, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, groups, dg;
} mrefsr_dcn_shape;

/* replaces modulated_deform_conv_forward (deform_conv_ext.cpp:107-125) / deform_conv_forward.
 * One fused kernel (deformable gather -> LDS -> MFMA GEMM -> bias + LeakyReLU) when the shape is
 * MFMA-eligible (groups 1, 3x3, C % 32 == 0, C/dg in {8,16,32,64,..}, Co in {64,128,256}: every
 * DynAgg of the path); a generic kernel otherwise.  `workspace` holds the re-packed weights
 * (mrefsr_dcn_fwd_workspace_bytes(s) bytes, 0 for the generic path).
 * nhwc (MFMA path only): bit 0: x is [B][H][W][C] -- a thread's 8 channels of a bilinear corner are
 * then two 16-byte loads instead of 8 scalar gathers; bit 1: out is written [B][Ho][Wo][Co]
 * (offset / mask stay planar).  With bit 0 the GEMM runs on the 16-bit matrix pipe from exact splits of columns
 * and weights, fp32-equivalent as in mrefsr_conv_nhwc_f32: fp16 two-term / three products (needs |column| < 65504:
 * `range_flag`, an int32 in device memory or NULL, is set to 1 otherwise -- same contract as the convolution's), or
 * the bf16 three-term / six-product split without range limit (bit 3, with bit 0; the re-run path of a caller whose
 * range flag fired).
 * bit 4 (with bits 0, 1, 2): x and out are bf16 tensors (2-byte channels-last storage; offset / mask stay fp32 planar).
 * bit 2 (with bit 0): bf16 ARITHMETIC instead (BASELINE configs[4]): columns and weights rounded to bf16,
 * fp32 accumulation, output rounded to bf16 in its fp32 container. */
int64_t mrefsr_dcn_fwd_workspace_bytes(const mrefsr_dcn_shape *s);
int mrefsr_dcn_fwd_f32(const float *x, const float *offset, const float *mask,
                       const float *weight, const float *bias, float *out,
                       const mrefsr_dcn_shape *s, float act_slope, int nhwc, void *workspace,
                       int64_t workspace_bytes, int *range_flag, mrefsr_stream_t stream);
/* the same with out_amax[0] = max(out_amax[0], max |out|) (device memory, zero-initialised by the caller, may be NULL; channels-last
 * x only): the input scale of the Winograd convolutions that read the aggregated features (MRAPAFusion.conv_emb2 / conv_ass,
 * ref_mrapa_restoration_arch.py:271-304, 321-335) -- see mrefsr_conv_nhwc_amax_f32. */
int mrefsr_dcn_fwd_amax_f32(const float *x, const float *offset, const float *mask,
                            const float *weight, const float *bias, float *out,
                            const mrefsr_dcn_shape *s, float act_slope, int nhwc, void *workspace,
                            int64_t workspace_bytes, int *range_flag, float *out_amax, mrefsr_stream_t stream);

/* columns[B][C*kh*kw][Ho*Wo] = mask * bilinear(x)  (modulated_deformable_im2col, .cu:570-633);
 * used by the backward's weight gradient (deform_conv_cuda.cpp:640-663). */
int mrefsr_dcn_im2col_f32(const float *x, const float *offset, const float *mask, float *columns,
                          const mrefsr_dcn_shape *s, mrefsr_stream_t stream);

/* grad_col [B][C*kh*kw][Ho*Wo] (= W^T grad_out, computed by the caller's GEMM) ->
 * grad_offset, grad_mask (assigned; .cu:695-767) and grad_x (accumulated with atomics into a
 * caller-zeroed buffer; .cu:635-693).  grad_x or grad_mask may be NULL. */
int mrefsr_dcn_col2im_f32(const float *grad_col, const float *x, const float *offset,
                          const float *mask, float *grad_x, float *grad_offset, float *grad_mask,
                          const mrefsr_dcn_shape *s, mrefsr_stream_t stream);

/* The backward of the modulated deformable convolution w.r.t. offset, mask and input as ONE fused launch -- what
 * deform_conv_cuda.cpp:571-685 runs as a GEMM (d columns = W^T . grad_out, :617-620) into a C*9*H*W buffer followed by
 * modulated_deformable_col2im + col2im_coord (deform_conv_cuda_kernel.cu:635-767): the column gradient is formed per tile of 32
 * pixels on the matrix pipe (fp16 two-term split, fp32-equivalent) and consumed from the accumulators.
 *   3x3, stride 1, pad 1, dilation 1, groups 1, C % 32 == 0, Co % 16 == 0, C / dg in {8, 16, 32}
 *   grad_out [B][H][W][Co], x [B][H][W][C] channels-last; offset [B][18 dg][H][W], mask [B][9 dg][H][W] planar (mask may be NULL)
 *   packed_wT: the weight [Co][C][3][3] packed by mrefsr_conv_pack_weight_view_f32(weight, packed, Cout := C, Cin := Co, 3, terms 16,
 *              wscale, stride_o = 9, stride_i = 9 C, flip = 0): the transposed operator, taps in place
 *   g_amax: device float, max |grad_out| (NULL: grad_out is used as it is; it must then lie inside the fp16 range)
 *   grad_x [B][C][H][W] PLANAR, zero-initialised by the caller (float atomics), or NULL; grad_offset / grad_mask like offset / mask */
int mrefsr_dcn_bwd_data_f32(const float *grad_out, const float *x, const float *offset, const float *mask, const void *packed_wT,
                            float wscale, const float *g_amax, float *grad_x, float *grad_offset, float *grad_mask,
                            const mrefsr_dcn_shape *s, mrefsr_stream_t stream);
/* d weight [Co][C][3][3] of the same convolution: grad_out . columns^T (deform_conv_cuda.cpp:640-657) with the columns re-gathered
 * tile by tile instead of read back from a C*9*H*W buffer -- a pixel-K GEMM on the matrix pipe (fp16 two-term split of both
 * operands), partial sums per K split in `workspace` (mrefsr_dcn_bwd_weight_workspace_bytes), added in split order.
 * Layouts as mrefsr_dcn_bwd_data_f32; range_flag (device int, may be NULL) is raised when a column leaves the fp16 range. */
int64_t mrefsr_dcn_bwd_weight_workspace_bytes(const mrefsr_dcn_shape *s);
int mrefsr_dcn_bwd_weight_f32(const float *grad_out, const float *x, const float *offset, const float *mask, const float *g_amax,
                              float *grad_weight, void *workspace, int64_t workspace_bytes, const mrefsr_dcn_shape *s,
                              int *range_flag, mrefsr_stream_t stream);

/* Weight gradient of a 1x1 convolution (conv_emb1, spatial_attn, feat_fusion of ref_mrapa_restoration_arch.py:271-304; what
 * torch.autograd runs as miopenConvolutionBackwardWeights under multi_ref_restoration_model.py:197-279):
 * grad_weight[o][i] = sum over pixels of g[pixel][o] * x[pixel][i], g [pixels][ld_g] and x [pixels][ld_x] channels-last fp32;
 * a pixel-K GEMM on the matrix pipe (fp16 two-term split of both operands, g scaled by max |g| = *g_amax into the fp16 range),
 * partial sums per K split in `workspace`, added in split order (deterministic). */
int64_t mrefsr_conv_wgrad1x1_workspace_bytes(int64_t pixels, int Cout, int Cin);
int mrefsr_conv_wgrad1x1_f32(const float *g, const float *x, const float *g_amax, float *grad_weight, void *workspace,
                             int64_t workspace_bytes, int64_t pixels, int Cout, int ld_g, int Cin, int ld_x, int *range_flag,
                             mrefsr_stream_t stream);
/* The same three operators for every dtype of the reference's dispatch (AT_DISPATCH_FLOATING_TYPES_AND_HALF,
 * deform_conv_cuda_kernel.cu:259,353,451,781,813,846): all tensors of one `dtype` (0 = f32, 1 = f16, 3 = f64), planar
 * NCHW layouts as above, any stride / dilation / groups / kernel size; float accumulation (double for f64).  Portable
 * kernels (one thread per output pixel x 16 channels), not the fused MFMA path: the fp32 product path is
 * mrefsr_dcn_fwd_f32.  mrefsr_dcn_col2im takes f32 / f64 (native atomics); an f16 caller accumulates gradients in f32. */
int mrefsr_dcn_fwd(const void *x, const void *offset, const void *mask, const void *weight, const void *bias,
                   void *out, const mrefsr_dcn_shape *s, float act_slope, int dtype, mrefsr_stream_t stream);
int mrefsr_dcn_im2col(const void *x, const void *offset, const void *mask, void *columns,
                      const mrefsr_dcn_shape *s, int dtype, mrefsr_stream_t stream);
int mrefsr_dcn_col2im(const void *grad_col, const void *x, const void *offset, const void *mask, void *grad_x,
                      void *grad_offset, void *grad_mask, const mrefsr_dcn_shape *s, int dtype,
                      mrefsr_stream_t stream);


/* ---------------------------------------------------------------------------------------------
 * Multi-reference feature-transfer attention core: ref_mrapa_restoration_arch.py:321-335
 *   q   [N][c][HW]       conv_emb1(target) * c^-1/2
 *   emb [N*T][c][HW]     conv_emb2(refs)  (refs stacked [N][T] on dim 0, :318)
 *   ass [N*T][c2][HW]    conv_ass(refs)
 *   out [N][c2][HW]      sum_t softmax_t(<q, emb_t>) * ass_t        T <= 16
 *   prob [N][T][HW]      softmax weights (saved for backward) or NULL
 *   t_major              0: refs stacked [N][T] as above; 1: stacked [T][N] (image t*N + n), the
 *                        layout of the batched-over-references path (no permute copy either way)
 * --------------------------------------------------------------------------------------------- */
int mrefsr_mrattn_fwd_f32(const float *q, const float *emb, const float *ass, float *out,
                          float *prob, int N, int T, int c, int c2, int HW, int t_major,
                          mrefsr_stream_t stream);
/* channels-last forward for the inference path: q [N][HW][c], emb [T*N][HW][c], ass [T*N][HW][2c]
 * (t-major), out [N][HW][2c]; c in {64, 128, 256}, T <= 16. */
int mrefsr_mrattn_fwd_nhwc_f32(const float *q, const float *emb, const float *ass, float *out, int N,
                               int T, int c, int HW, mrefsr_stream_t stream);
/* the same with `q * q_scale` (`self.conv_emb1(target) * self.scale`, ref_mrapa_restoration_arch.py:321) formed on the way in: each product
 * rounded on its own -- the bits of a separate element-wise pass over q, without the pass. */
int mrefsr_mrattn_fwd_nhwc_scaled_f32(const float *q, const float *emb, const float *ass, float *out, int N,
                                      int T, int c, int HW, float q_scale, mrefsr_stream_t stream);
int mrefsr_mrattn_bwd_f32(const float *q, const float *emb, const float *ass, const float *prob,
                          const float *g_out, float *g_q, float *g_emb, float *g_ass, int N,
                          int T, int c, int c2, int HW, int t_major, mrefsr_stream_t stream);
/* The channels-last attention core on bf16 tensors (2-byte activation storage, BASELINE configs[4]): same lanes and
 * operation order as mrefsr_mrattn_fwd_nhwc_f32, fp32 math, the result rounded to bf16 (round-to-nearest-even). */
int mrefsr_mrattn_fwd_nhwc_bf16(const void *q, const void *emb, const void *ass, void *out, int N, int T,
                                int c, int HW, mrefsr_stream_t stream);
/* Per-sample reference masks (mixed reference counts in one batch): the kernels above with
 *   valid_bits [N]       one 32-bit word per sample, bit t set = reference t of the sample is present (bits >= T are ignored)
 * An absent t is left out of the maximum, the denominator and the weighted sum; its emb / ass values are never read (inf or NaN
 * there reaches no output); `prob` is written as exact 0 for it; mrefsr_mrattn_bwd_masked_f32 writes its g_emb / g_ass as exact
 * zeros and sums g_q over the present t only.  The present terms run in ascending t with the operations of the unmasked kernels,
 * so a sample's result is that of the unmasked kernel on its compacted references.  A word with no bit below T: out = 0, prob = 0
 * and all three gradients 0 for that sample.  mrefsr_mrattn_fwd_nhwc_masked_f32 takes q_scale as
 * mrefsr_mrattn_fwd_nhwc_scaled_f32 does (1 = none). */
int mrefsr_mrattn_fwd_masked_f32(const float *q, const float *emb, const float *ass, const uint32_t *valid_bits, float *out,
                                 float *prob, int N, int T, int c, int c2, int HW, int t_major, mrefsr_stream_t stream);
int mrefsr_mrattn_bwd_masked_f32(const float *q, const float *emb, const float *ass, const float *prob, const float *g_out,
                                 const uint32_t *valid_bits, float *g_q, float *g_emb, float *g_ass, int N, int T, int c, int c2,
                                 int HW, int t_major, mrefsr_stream_t stream);
int mrefsr_mrattn_fwd_nhwc_masked_f32(const float *q, const float *emb, const float *ass, const uint32_t *valid_bits, float *out,
                                      int N, int T, int c, int HW, float q_scale, mrefsr_stream_t stream);
int mrefsr_mrattn_fwd_nhwc_masked_bf16(const void *q, const void *emb, const void *ass, const uint32_t *valid_bits, void *out, int N,
                                       int T, int c, int HW, mrefsr_stream_t stream);
/* The same head with the blend moved in front of conv_ass (ref_mrapa_restoration_arch.py:321-335).  conv_ass is a plain 3x3
 * convolution and the softmax weights depend on the output pixel only, so
 *   sum_t p_t(x) (sum_d W_d s_t(x + d) + b)  =  sum_d W_d (sum_t p_t(x) s_t(x + d))  +  b sum_t p_t(x):
 * one implicit GEMM over N images instead of a convolution over T * N images and a pass that folds its T results.
 * mrefsr_mrattn_prob_nhwc_f32 (ref_mrapa_restoration_arch.py:321-335: the softmax of :323-329): prob [N][HW][T] fp32 from
 * q [N][HW][c] and emb [T*N][HW][c] (t-major), q * q_scale formed on the way in -- the logits, maximum, expf, denominator and
 * reciprocal of mrefsr_mrattn_fwd_nhwc_scaled_f32 / _masked_f32 in their order.  valid_bits may be NULL (every reference present);
 * an absent t is never read and gets exactly 0, a sample without a present reference all zeros.  c in {64, 128, 256}, T <= 16. */
int mrefsr_mrattn_prob_nhwc_f32(const float *q, const float *emb, const uint32_t *valid_bits, float *prob, int N, int T, int c,
                                int HW, float q_scale, mrefsr_stream_t stream);
/* mrefsr_mrattn_blend_conv_f32 (ref_mrapa_restoration_arch.py:321-335: conv_ass of :322 and the assembly of :331-335 in one launch):
 *   refs [T*N][H][W][C] fp32 (t-major)   the warped reference maps conv_ass would read
 *   prob [N][H][W][T]                    the weights above.  Precondition: prob >= 0 and sum_t prob <= 1 at every pixel; the range
 *                                        guard checks the staged references, and |blend| <= max |refs| holds only under it
 *   packed                               conv_ass.weight [2C][C][3][3] packed by mrefsr_conv_pack_weight_f32 with terms = 16 and
 *                                        the power-of-two scale `wscale`
 *   bias [2C] or NULL                    enters as bias * sum_t prob_t (the sum in fp32, present t ascending)
 *   valid_bits [N] or NULL               an absent t is never staged or read (Inf / NaN there reaches nothing)
 *   in_amax or NULL                      device word with max |refs|: the staged values are scaled by an exact power of two as in
 *                                        mrefsr_conv_nhwc_scaled_f32
 *   range_flag or NULL                   bit 0 is set when a staged value leaves the fp16 range (|x| > 65000)
 *   out [N][H][W][2C] fp32
 * The blend is an fp32 fma chain over t ascending, split exactly into two fp16 terms; three v_mfma_f32_32x32x16_f16 per product,
 * fp32 accumulation in the fixed order channel chunk, tap, term: fp32-equivalent and bit-reproducible.  Any H, W >= 1;
 * C in {64, 128, 256}; T <= 16. */
int mrefsr_mrattn_blend_conv_f32(const float *refs, const float *prob, const void *packed, const float *bias, const uint32_t *valid_bits,
                                 const float *in_amax, int *range_flag, float *out, int N, int T, int H, int W, int C, float wscale,
                                 mrefsr_stream_t stream);


/* ---------------------------------------------------------------------------------------------
 * basicsr/ops/fused_act: fused_bias_act(input, bias, refer, act, grad, alpha, scale)
 * (fused_bias_act.cpp:14-26, kernel fused_bias_act_kernel.cu:19-50).  bias / ref may be NULL
 * ("empty tensor" in the reference).  dtype: 0 = f32, 1 = f16, 2 = bf16, 3 = f64 (the reference dispatches
 * AT_DISPATCH_FLOATING_TYPES_AND_HALF, fused_bias_act_kernel.cu:81; bf16 is an extension); math in float, double for f64.
 * --------------------------------------------------------------------------------------------- */
int mrefsr_fused_bias_act(const void *x, const void *bias, const void *ref, void *out,
                          int64_t size_x, int step_b, int size_b, int act, int grad, float alpha,
                          float scale, int dtype, mrefsr_stream_t stream);

/* Tail of the restoration network (ref_mrapa_restoration_arch.py:132-137: base = F.interpolate(x, None, 4, 'bilinear', False); ... out + base):
 * out [B][C][h*scale][w*scale] (NCHW) = y [B][h*scale][w*scale][ld >= C] (channels-last result of the last convolution) +
 * bilinear(x [B][C][h][w]) with align_corners = False, in one pass; the interpolation returns the bits of torch's upsample_bilinear2d. */
int mrefsr_tail_bilinear_add_f32(const float *y_nhwc, const float *x, float *out, int B, int C, int h, int w, int scale, int ld,
                                 mrefsr_stream_t stream);

/* Convolution epilogue of the NCHW fp32 path (the `conv -> (+bias) -> LeakyReLU/ReLU -> (+x)` idiom
 * of ResidualBlockNoBN arch_util.py:113-116, the VGG stacks and the lrelu(conv(.)) chains of
 * ref_mrapa_restoration_arch.py): out = lrelu(x + bias[c] + pre, slope) + residual in one pass.
 * pre [pre_N][C][HW] is added BEFORE the activation and broadcast over N / pre_N groups (image n
 * uses pre[n % pre_N]: the x-half of offset_conv1 shared by the K references); bias / pre /
 * residual may be NULL; out may alias x; slope 1 = identity, 0 = ReLU. */
int mrefsr_bias_act_res_f32(const float *x, const float *bias, const float *pre, int64_t pre_N,
                            const float *residual, float *out, int64_t N, int C, int64_t HW,
                            float slope, mrefsr_stream_t stream);

/* 3x3 (pad 1) / 1x1 stride-1 convolution with fused epilogue, for the residual trunks, VGG stacks,
 * offset convolutions and fusion heads (arch_util.py ResidualBlockNoBN, ref_mrapa_restoration_arch.py
 * :139-348, vgg_arch.py, contras_multi_extractor_arch.py) on channels-last activations.
 * fp32-equivalent arithmetic on the bf16 matrix pipe: operands split exactly into 3 bf16 terms,
 * `terms` = 6 partial products per product (all those >= 2^-24 relative; 3 = two-term split,
 * ~2^-16 relative, for experiments only; 1 = bf16 ARITHMETIC for BASELINE configs[4]: both operands rounded to
 * bf16, one product, fp32 accumulation, result rounded to bf16 in its fp32 container).  `terms` = 16: fp16 two-term split (11 + 11 significand
 * bits, three products, dropped term 2^-22 relative; as accurate as an fp32 convolution whose own
 * accumulation error dominates, at twice the speed of terms = 6).  It needs |activation| < 65504 and
 * a per-layer power-of-two weight scale `wscale` with max|w| * wscale in [2^13, 2^14), given to the
 * pack call and in the descriptor (the epilogue divides it out); `range_flag` (device int, may be
 * NULL) is set to 1 by any block that meets an activation outside +-65000 (or NaN): the result of
 * that launch is then not to be trusted and the caller should rerun with terms = 6.
 * `terms` = 2 (descriptor only; weights packed with terms = 1): the bf16 arithmetic of terms = 1 on bf16 TENSORS -- x1, x2,
 * pre, residual and out are [..][C] arrays of 2-byte bf16 passed through the same pointers (channel counts and leading
 * dimensions multiples of 8; bias and slope stay fp32).  Same values as terms = 1, half the activation bytes.
 * `terms` = 17: the terms-16 arithmetic in Winograd F(2x2, 3x3) form (3x3 kernels, fp32 tensors, epilogues 0 / 1 / 2, at least 17
 * input channels, H W ld 4 < 2^32): Y = A^T [sum_c (G g G^T) . (B^T d B)] A with G g G^T formed (fp64) and split at pack time under the
 * same `wscale`, B^T d B formed in fp32 and then split -- 2.25x fewer MFMAs per output, the same or a smaller error against fp64
 * (the accumulation chains are 9x shorter); the fp16 guard fires when a transform value leaves the fp16 range (|B^T d B| <= 4 max|x|
 * after the input scale: the eight-wave kernel compares |x| with 16000, the four-wave kernel flags the non-finite outputs), the low term of an
 * activation is an fp16 subnormal below |x| = 2^-3 (absolute error <= 2^-25) unless the launch is given the input's maximum
 * (mrefsr_conv_nhwc_scaled_f32).  Weights packed with terms = 17
 * (mrefsr_conv_packed_bytes / mrefsr_conv_pack_weight[_view]_f32) only serve terms = 17 descriptors.
 *   input   = channel concatenation of x1 [N1][H][W][ld1] (first C1 channels used) and, if C2 > 0,
 *             x2 [N2][H][W][ld2]; image n reads x1[n % N1], x2[n % N2] (batch broadcast);
 *             C1, C2, ld1, ld2 multiples of 4; C1 a multiple of 16 when C2 > 0
 *   packed  = weight [Cout][C1+C2][k][k] re-ordered once by mrefsr_conv_pack_weight_f32 into
 *             mrefsr_conv_packed_bytes(Cout, C1+C2, ksize, terms) bytes (a weight with fewer input
 *             channels than C1+C2 packs with zero padding: pass its own Cin to both calls)
 *   v       = conv + bias[c] + pre[n % pre_N][y][x][c]          (bias, pre may be NULL; pre has ld = Cout)
 *   v       = act ? LeakyReLU(v, slope_ptr ? *slope_ptr : slope) : v     (slope 0 = ReLU; *slope_ptr = PReLU)
 *   v      += residual[n][y][x][c]  (ld_res)                    (may be NULL)
 *   epilogue 0: out[n][y][x][c] (ld_out)   1: MaxPool2d(2,2) -> out [N][H/2][W/2][ld_out]
 *            2: PixelShuffle(2)  -> out [N][2H][2W][ld_out], channel c/4 */
typedef struct mrefsr_conv_desc {
    int32_t N, H, W, ksize;
    int32_t C1, ld1, N1;
    int32_t C2, ld2, N2;
    int32_t Cout, ld_out, ld_res, pre_N;
    int32_t act, epilogue, terms;
    float slope;
    float wscale; /* terms == 16 only */
} mrefsr_conv_desc;
int64_t mrefsr_conv_packed_bytes(int Cout, int Cin, int ksize, int terms);
int mrefsr_conv_pack_weight_f32(const float *weight, void *packed, int Cout, int Cin, int ksize, int terms,
                                float wscale, mrefsr_stream_t stream);
/* The same packing of a strided VIEW of a weight: element (o, i, tap) is read at
 * weight[o * stride_o + i * stride_i + (flip ? k*k - 1 - tap : tap)].  stride_o = Cin_total*k*k, stride_i = k*k, flip = 0 and a
 * pointer offset select an input-channel slice in place (the two halves of offset_conv1, ref_mrapa_restoration_arch.py:217);
 * swapped strides with flip = 1 pack the operator of the convolution's INPUT GRADIENT (Cout := the slice's channels,
 * Cin := the original Cout): what torch.autograd runs as miopenConvolutionBackwardData in the reference's training step
 * (multi_ref_restoration_model.py:197-279) is mrefsr_conv_nhwc_f32 on the output gradient with these weights. */
int mrefsr_conv_pack_weight_view_f32(const float *weight, void *packed, int Cout, int Cin, int ksize, int terms, float wscale,
                                     int64_t stride_o, int64_t stride_i, int flip, mrefsr_stream_t stream);
/* n_jobs such packings in ONE launch -- every convolution weight of net_g and its input-gradient operator after an optimiser
 * step (optimizer_g.step(), multi_ref_restoration_model.py:277: the reference's weights change once per step, so do the packed
 * copies).  `jobs` is a table in DEVICE memory, each entry the arguments of mrefsr_conv_pack_weight_view_f32.  range_flag
 * (device int32 or NULL) is set to 1 if a terms-16 entry meets |weight * wscale| > 65000 or a non-finite weight. */
typedef struct mrefsr_conv_pack_job {
    const float *weight;
    void *packed;
    int64_t stride_o, stride_i;
    int32_t Cout, Cin, ksize, terms, flip;
    float wscale;
} mrefsr_conv_pack_job;
int mrefsr_conv_pack_weights_multi_f32(const mrefsr_conv_pack_job *jobs, int n_jobs, int *range_flag, mrefsr_stream_t stream);
/* A 1x1 convolution that follows a 3x3 one with nothing non-linear between them, as ONE 3x3 convolution (csrc/conv_fold.hip) --
 * spatial_attn_add2 and the reference half of feat_fusion at inference (ref_mrapa_restoration_arch.py:338-347: the 1x1 acts after
 * the zero padding, so the composition is exact):
 *   out_w[o][i][tap] = float( sum_m w1x1[o * ld_1x1 + cin_offset + m] * w3x3[m][i][tap] )        [Cout][Cin][3][3]
 *   out_b[o]         = float( b1x1[o] + sum_m w1x1[o * ld_1x1 + cin_offset + m] * b3x3[m] )      (out_b, b1x1, b3x3 may be NULL)
 * w1x1 is [Cout][ld_1x1] (columns cin_offset .. cin_offset + Cmid are used), w3x3 [Cmid][Cin][3][3].  The sums run in double in
 * ascending m (exact products, one rounding per element): two calls give the same bits.  The result is an ordinary weight: it goes
 * through mrefsr_conv_pack_weight_f32 for any `terms`.  Done once per weight version, not per step. */
int mrefsr_conv_compose_1x1_3x3_f32(const float *w1x1, int64_t ld_1x1, int cin_offset, const float *w3x3, const float *b3x3,
                                    const float *b1x1, float *out_w, float *out_b, int Cout, int Cmid, int Cin, mrefsr_stream_t stream);
int mrefsr_conv_nhwc_f32(const mrefsr_conv_desc *d, const float *x1, const float *x2, const void *packed,
                         const float *bias, const float *slope_ptr, const float *pre, const float *residual,
                         float *out, int *range_flag, mrefsr_stream_t stream);
/* mrefsr_conv_nhwc_f32 (terms = 16) on inputs of unknown, possibly tiny magnitude -- the output gradients of a training step
 * (multi_ref_restoration_model.py:197-279), which sit far below the fp16 normal range: in_amax[0] (device memory, written by
 * mrefsr_act_bwd_nhwc_f32) is max |x| over the input tensor(s); the kernel multiplies x by the power of two that brings it into
 * [2^13, 2^14) before the two-term split and the result by its inverse -- both exact -- so the three-product mode serves the
 * input-gradient convolutions as it serves the forward ones.  in_amax = NULL: exactly mrefsr_conv_nhwc_f32.
 * terms = 17 takes it too: the Winograd kernels split B^T d B after forming it, and the LOW term of a value below 2^-3 is an fp16
 * subnormal; with in_amax they bring max |x| into [2^11, 2^12) first (the transform grows values by at most 4) and the forward
 * convolution of small activations (1e-2 and less) is as accurate as an fp32 one.  The host mirror hands every layer the maximum
 * its producer measured (mrefsr_conv_nhwc_amax_f32 / mrefsr_dcn_fwd_amax_f32: out_amax of one launch = in_amax of the next). */
int mrefsr_conv_nhwc_scaled_f32(const mrefsr_conv_desc *d, const float *x1, const float *x2, const void *packed,
                                const float *bias, const float *slope_ptr, const float *pre, const float *residual,
                                float *out, int *range_flag, const float *in_amax, mrefsr_stream_t stream);
/* mrefsr_conv_nhwc_scaled_f32 that also MEASURES its output: out_amax[0] = max(out_amax[0], max |out|) (device memory, the caller
 * zero-initialises it; may be NULL; terms 16 / 17, fp32 tensors, every epilogue).  The Winograd launch that reads `out` next takes
 * the same word as its in_amax: the input scale of every 3x3 layer of the path is the CURRENT batch's maximum, measured in the
 * producing kernel's epilogue (the values are in registers there) -- no reduction pass, no calibration that could go stale
 * (round 5 measured once per layer with two torch launches; archs/nhwc.py).  Replaces, per layer, what the reference leaves to
 * fp32 arithmetic (arch_util.py:89-117, ref_mrapa_restoration_arch.py:213-259). */
int mrefsr_conv_nhwc_amax_f32(const mrefsr_conv_desc *d, const float *x1, const float *x2, const void *packed,
                              const float *bias, const float *slope_ptr, const float *pre, const float *residual,
                              float *out, int *range_flag, const float *in_amax, float *out_amax, mrefsr_stream_t stream);
/* The input-gradient convolution of a training step (torch.autograd's miopenConvolutionBackwardData in the reference,
 * multi_ref_restoration_model.py:197-279) with the element-wise pass that would follow it folded into its epilogue -- inside a
 * residual block (arch_util.py:45-70) the gradient of conv2's input is masked by the ReLU between the two convolutions and
 * summed per channel for conv1's bias:  residual_is_mask = 1 turns `residual` into that mask source (out = residual > 0 ? conv : 0);
 * stat_sum[Cout] += per-channel sums of out, stat_amax[0] = max(stat_amax[0], max |out|) (zero-initialised by the caller, either
 * may be NULL).  terms = 16, fp32 tensors, plain epilogue, Cout / ld_out / ld_res multiples of 4; in_amax as above. */
int mrefsr_conv_nhwc_bwd_f32(const mrefsr_conv_desc *d, const float *x1, const void *packed, const float *residual,
                             int residual_is_mask, float *out, int *range_flag, const float *in_amax, float *stat_sum,
                             float *stat_amax, mrefsr_stream_t stream);
/* The same, bitwise reproducible: every block writes its 64 per-cout sums to its own row of `workspace` (workspace_bytes >=
 * mrefsr_conv_nhwc_bwd_det_workspace_bytes(d)), the rows of a cout block in (image, tile row, tile column) order whatever order
 * the blocks ran in, and the block that finishes last adds them in that order into stat_sum -- a fixed order instead of float
 * atomics, in the same launch.  ticket[0] (device memory) is 0 before the first launch and 0 again after every launch (no
 * memset between launches or graph replays).  One launch at a time per workspace / ticket.  out and stat_amax as above, bit for bit. */
int64_t mrefsr_conv_nhwc_bwd_det_workspace_bytes(const mrefsr_conv_desc *d);
int mrefsr_conv_nhwc_bwd_det_f32(const mrefsr_conv_desc *d, const float *x1, const void *packed, const float *residual,
                                 int residual_is_mask, float *out, int *range_flag, const float *in_amax, float *stat_sum,
                                 float *stat_amax, void *workspace, int64_t workspace_bytes, uint32_t *ticket, mrefsr_stream_t stream);
/* conv_offset_mask of a DynAgg + its glue in one launch (ref_mrapa_restoration_arch.py:56-73: chunk / cat / repeat /
 * re-order / add / sigmoid / mean-abs): the 3x3 convolution `x` [N][H][W][C1] -> 27*dg channels runs as in
 * mrefsr_conv_nhwc_f32 (same packed weights, terms, wscale, range flag; fields N, H, W, C1, ld1, Cout = 27*dg, ksize = 3,
 * terms, wscale of `d` are read), and its epilogue writes what mrefsr_dcn_fwd_f32 reads, PLANAR:
 *   offset [N][18*dg][H][W] = channels [0, 18 dg) + pre_offset (pre_offset [N][9][H][W][2] is [x, y] per tap: channel
 *                              g*18 + 2*tap gets y, + 1 gets x),   mask [N][9*dg][H][W] = sigmoid(channels [18 dg, 27 dg)),
 *   *abs_sum (double, device, may be NULL) += sum |channels [0, 18 dg)|  (the reference's `offset mean > 100` guard, read by
 *   the host when it likes).  Bit-identical to mrefsr_conv_nhwc_f32 followed by mrefsr_dynagg_prep_f32(om_nhwc = 1). */
int mrefsr_conv_dynagg_f32(const mrefsr_conv_desc *d, const float *x, const void *packed, const float *bias,
                           const float *pre_offset, float *offset, float *mask, double *abs_sum, int dg,
                           int *range_flag, mrefsr_stream_t stream);


/* Spatial-attention modulation of MRAPAFusion (ref_mrapa_restoration_arch.py:343-345) in one pass:
 * mul_inout[i] = refs[i] * sigmoid(mul_inout[i]) * 2 + add[i]; n a multiple of 4, any (common) layout.  The f32 entry takes
 * add = NULL: refs[i] * sigmoid(mul_inout[i]) * 2, the same expression without its last add (the addend then reaches feat_fusion
 * as the `pre` of its launch, mrefsr_conv_compose_1x1_3x3_f32). */
int mrefsr_attn_modulate_f32(const float *refs, float *mul_inout, const float *add, int64_t n,
                             mrefsr_stream_t stream);
int mrefsr_attn_modulate_bf16(const void *refs, void *mul_inout, const void *add, int64_t n, mrefsr_stream_t stream);


/* Input normalisation of the feature extractors (vgg_arch.py:150-153: `(x + 1) / 2` when range_norm, then `(x - mean) / std`;
 * contras_multi_extractor_arch.py:41) fused with the engine's channels-last packing: img [N][3][HW] -> out [N][HW][4]
 * (channel 3 = 0; the packed first-layer weights carry a zero fourth input channel).  mean3 / std3: 3 floats in device memory,
 * both NULL = no normalisation.  ATen's operations in ATen's order: bit-identical to the six launches it replaces. */
int mrefsr_image_to_nhwc4_f32(const float *img, float *out, int64_t N, int64_t HW, int range_norm, const float *mean3,
                              const float *std3, mrefsr_stream_t stream);


/* conv -> +bias -> ReLU -> MaxPool2d(2, 2) of the VGG stacks (vgg_arch.py:113-120,
 * contras_multi_extractor_arch.py:14-27) in one pass: out [N][C][H/2][W/2] = relu(max2x2(x) + bias[c])
 * (bit-identical to pooling the biased, rectified map). */
int mrefsr_bias_relu_pool2_f32(const float *x, const float *bias, float *out, int64_t N, int C, int H,
                               int W, mrefsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * basicsr/ops/upfirdn2d: upfirdn2d(input (major,in_h,in_w,minor), kernel (kh,kw), up, down, pad)
 * (upfirdn2d.cpp:13-24, upfirdn2d_kernel.cu:50-370).  out (major,out_h,out_w,minor) with
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kh + down_y) / down_y  (.cu:240-243).
 * --------------------------------------------------------------------------------------------- */
int mrefsr_upfirdn2d_f32(const float *in, const float *kernel, float *out, int major, int in_h,
                         int in_w, int minor, int kh, int kw, int up_x, int up_y, int down_x,
                         int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                         mrefsr_stream_t stream);
/* The same for any of the reference's dtypes (AT_DISPATCH_FLOATING_TYPES_AND_HALF, upfirdn2d_kernel.cu:312): input, kernel
 * and output share `dtype` (0 = f32, 1 = f16, 2 = bf16 (extension), 3 = f64); accumulation in float (double for f64). */
int mrefsr_upfirdn2d(const void *in, const void *kernel, void *out, int major, int in_h, int in_w,
                     int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0,
                     int pad_x1, int pad_y0, int pad_y1, int dtype, mrefsr_stream_t stream);

/* ---- backward glue of the channels-last training engine (net_g under MultiRefRestorationModel.optimize_parameters,
 * multi_ref_restoration_model.py:197-279; what torch.autograd runs as separate elementwise / reduction kernels per layer).
 *
 * mrefsr_act_bwd_nhwc_f32: backward of the fused convolution epilogue  out = act(conv + bias):
 *   g_pre[p][c] (ld_pre; may be NULL) = g_out[p][c] * (out[p][c] > 0 ? 1 : slope)        act 1: LeakyReLU(slope), 0 = ReLU
 *                                                                                      act 2: PReLU(*slope_ptr); act 0: copy
 *   bias_grad[c] (may be NULL)  += sum of g_pre over the pixels: the bias gradient (torch's conv backward bias term).  The
 *                     caller zero-initialises it; blocks add their totals with float atomics (order not fixed, like the
 *                     reference's own atomically accumulating backward kernels, deform_conv_cuda_kernel.cu:330,688)
 *   slope_grad[0] (act 2, may be NULL) += sum of g_out * x over x < 0, x = out / slope (PReLU weight gradient); needs
 *                     slope > 0 -- *flag (int32, device, may be NULL) is set to 1 otherwise
 *   amax[0] (may be NULL) = max(amax[0], max |g_pre|) (zero-initialised by the caller): the input scale of
 *                     mrefsr_conv_nhwc_scaled_f32 for the input-gradient convolution that follows
 *   g_out, out contiguous [npix][C]; C <= 1024, a multiple of 4 when > 256. */
int mrefsr_act_bwd_blocks(int64_t npix, int C);
int mrefsr_act_bwd_nhwc_f32(const float *g_out, const float *out, float *g_pre, int ld_pre, float *bias_grad, float *slope_grad, float *amax,
                            int64_t npix, int C, int act, float slope, const float *slope_ptr, int *flag, mrefsr_stream_t stream);
/* mrefsr_act_bwd_nhwc_det_f32: the same, bitwise reproducible.  Every block writes its C channel sums and its slope sum to its
 *   own row of `workspace` ([mrefsr_act_bwd_blocks][C + 1] floats, workspace_bytes >= mrefsr_act_bwd_det_workspace_bytes), and
 *   the block that finishes last adds the rows in ascending block order into bias_grad / slope_grad -- a fixed order instead of
 *   float atomics, in the same launch.  ticket[0] (device memory) is 0 before the first launch and 0 again after every launch
 *   (no memset between launches or graph replays).  One launch at a time per workspace / ticket.  g_pre, amax and *flag as
 *   above, bit for bit. */
int64_t mrefsr_act_bwd_det_workspace_bytes(int64_t npix, int C);
int mrefsr_act_bwd_nhwc_det_f32(const float *g_out, const float *out, float *g_pre, int ld_pre, float *bias_grad, float *slope_grad, float *amax,
                                int64_t npix, int C, int act, float slope, const float *slope_ptr, int *flag, void *workspace,
                                int64_t workspace_bytes, uint32_t *ticket, mrefsr_stream_t stream);
/* Weight gradient of a 3x3 stride-1 'same' convolution over channels-last tensors (torch's miopenConvolutionBackwardWeights in
 * the reference's training step):  dw[co][ci][ty][tx] (+)= sum_{n,y,x} g[n][y][x][co] * x[n][y+ty-1][x+tx-1][ci].
 *   x [N][H][W][ld_x] (channels [0, Cin) used), g [N][H][W][ld_g] (channels [0, Cout)); dw element (co, ci, tap) at
 *   dw[co*stride_co + ci*stride_ci + tap] -- an OIHW tensor or an input-channel slice of one; accumulate = 0 overwrites it,
 *   1 adds to it.  Blocks leave 64 x 64 x 9 partial sums in `workspace` (mrefsr_conv_wgrad3x3_workspace_bytes), a second
 *   launch adds them in a fixed order: deterministic.
 *   g_amax[0] = max |g| (device memory, from mrefsr_act_bwd_nhwc_f32): the gradient is scaled by an exact power of two into the
 *   fp16 range before its two-term split, as in mrefsr_conv_nhwc_scaled_f32; x must satisfy |x| < 65504 (range_flag, may be
 *   NULL).  fp32-equivalent: three fp16 MFMA products per term, fp32 accumulation. */
int64_t mrefsr_conv_wgrad3x3_workspace_bytes(int N, int H, int W, int Cin, int Cout);
/* The same for n_jobs (<= MREFSR_WGRAD_MAX_JOBS) convolutions of ONE geometry -- the 32 convolutions of a residual trunk
 * (arch_util.py:45-70 stacked 16 times, ref_mrapa_restoration_arch.py) whose weight gradients autograd runs one after the other --
 * in one launch pair: x, g, g_amax, dw are host arrays of n_jobs device pointers. */
#define MREFSR_WGRAD_MAX_JOBS 32
int64_t mrefsr_conv_wgrad3x3_batch_workspace_bytes(int n_jobs, int N, int H, int W, int Cin, int Cout);
int mrefsr_conv_wgrad3x3_batch_f32(int n_jobs, const float *const *x, int ld_x, int Cin, const float *const *g, int ld_g, int Cout,
                                   float *const *dw, int64_t stride_co, int64_t stride_ci, int accumulate, const float *const *g_amax,
                                   int N, int H, int W, void *workspace, int64_t workspace_bytes, int *range_flag, mrefsr_stream_t stream);
int mrefsr_conv_wgrad3x3_f32(const float *x, int ld_x, int Cin, const float *g, int ld_g, int Cout, float *dw, int64_t stride_co,
                             int64_t stride_ci, int accumulate, const float *g_amax, int N, int H, int W, void *workspace,
                             int64_t workspace_bytes, int *range_flag, mrefsr_stream_t stream);
/* gradient of mrefsr_mrattn_fwd_nhwc_f32 (ref_mrapa_restoration_arch.py:321-335 under autograd): same layouts, g_out [N][HW][2c]
 * -> g_q [N][HW][c], g_emb [T*N][HW][c], g_ass [T*N][HW][2c]; the softmax is recomputed, nothing is saved by the forward. */
int mrefsr_mrattn_bwd_nhwc_f32(const float *q, const float *emb, const float *ass, const float *g_out, float *g_q, float *g_emb,
                               float *g_ass, int N, int T, int c, int HW, mrefsr_stream_t stream);
/* the same under per-sample reference masks (valid_bits [N] as mrefsr_mrattn_fwd_nhwc_masked_f32): the softmax is recomputed over
 * the present references only, g_emb / g_ass of an absent reference are written as exact zeros without reading its emb / ass,
 * g_q sums the present ones; a word with no bit below T gives zeros in all three. */
int mrefsr_mrattn_bwd_nhwc_masked_f32(const float *q, const float *emb, const float *ass, const float *g_out,
                                      const uint32_t *valid_bits, float *g_q, float *g_emb, float *g_ass, int N, int T, int c, int HW,
                                      mrefsr_stream_t stream);
/* gradient of refs * sigmoid(mul) * 2 + add (ref_mrapa_restoration_arch.py:343-345) w.r.t. refs and mul (d/d add = g);
 * `mul` is the value BEFORE mrefsr_attn_modulate_f32 overwrote it. */
int mrefsr_attn_modulate_bwd_f32(const float *g, const float *refs, const float *mul, float *g_refs, float *g_mul, int64_t n,
                                 mrefsr_stream_t stream);

/* ---- reflect padding and cropping of channels-last maps (MRAPAFusion, ref_mrapa_restoration_arch.py:306-311, 348), with their
 * adjoints: the pad / crop nodes of the training engine.  [N][H][W][C] fp32, C a multiple of 4, 16-byte aligned; nothing is
 * allocated, nothing is synchronised.
 *
 * mrefsr_reflect_pad_nhwc_f32: x [N][H][W][C] -> out [N][H+ph][W+pw][C], the bottom and right padded by ph, pw in 0..3 with
 *   F.pad(mode='reflect') semantics (padded row H + i is source row H - 2 - i, likewise for columns); ph < H and pw < W, as F.pad
 *   requires.  Bit-identical to F.pad.
 * mrefsr_reflect_pad_bwd_nhwc_f32: its adjoint, g [N][H+ph][W+pw][C] -> gx [N][H][W][C]: each source pixel adds to its own
 *   gradient the row image, the column image and the corner image that mirror it, in this order (deterministic, no atomics).
 * mrefsr_crop_nhwc_f32: the top-left H0 x W0 window of x [N][H][W][C] -> out [N][H0][W0][C]; amax (may be NULL, zero-initialised
 *   by the caller) = max(amax[0], max |out|), the Winograd input scale of the convolution that reads the crop
 *   (as mrefsr_conv_nhwc_amax_f32's out_amax).
 * mrefsr_crop_bwd_nhwc_f32: its adjoint, g [N][H0][W0][C] -> gx [N][H][W][C]: g inside the window, zero in the band. */
int mrefsr_reflect_pad_nhwc_f32(const float *x, float *out, int N, int H, int W, int C, int ph, int pw, mrefsr_stream_t stream);
int mrefsr_reflect_pad_bwd_nhwc_f32(const float *g, float *gx, int N, int H, int W, int C, int ph, int pw, mrefsr_stream_t stream);
int mrefsr_crop_nhwc_f32(const float *x, float *out, float *amax, int N, int H, int W, int C, int H0, int W0, mrefsr_stream_t stream);
int mrefsr_crop_bwd_nhwc_f32(const float *g, float *gx, int N, int H, int W, int C, int H0, int W0, mrefsr_stream_t stream);

/* ---- perceptual / style loss of the training step (PerceptualLoss, basicsr/models/losses.py:141-238, under
 * multi_ref_restoration_model.py:237-279): the VGG19 node of mrefsr_amd/archs/nhwc_train.py.  Channels-last [N][H][W][C]
 * fp32 tensors, C % 4 == 0.
 *
 * mrefsr_maxpool2_nhwc_f32: MaxPool2d(2, 2) (floor sizes: out [N][H/2][W/2][C]); within a window (0,0) (0,1) (1,0) (1,1) the
 *   first maximum wins (torch's max_pool2d, bit for bit).  relu = 1 pools max(x, 0) (a pre-activation map whose ReLU was not
 *   stored).  plane (may be NULL): one byte per output element, bits 0-1 the arg-max, bit 2 = (max > 0).
 * mrefsr_maxpool2_bwd_nhwc_f32: g [N][H/2][W/2][C] -> g_in [N][H][W][C] (every element written; the floored last row / column
 *   of an odd map gets 0): g goes to the arg-max (from plane, else recomputed from x with the same rule), times the ReLU
 *   derivative (max > 0) when mask = 1.  amax (may be NULL, zero-initialised): max(amax, max |g_in|), the input scale of the
 *   fp16-split input-gradient convolution that follows (as mrefsr_act_bwd_nhwc_f32). */
int mrefsr_maxpool2_nhwc_f32(const float *x, float *out, uint8_t *plane, int N, int H, int W, int C, int relu, mrefsr_stream_t stream);
int mrefsr_maxpool2_bwd_nhwc_f32(const float *g, const float *x, const uint8_t *plane, float *g_in, float *amax, int N, int H, int W, int C,
                                 int relu, int mask, mrefsr_stream_t stream);
/* mrefsr_tap_crit_f32: criterion of up to MREFSR_TAP_MAX_JOBS taps in one launch (+ a one-block second stage).
 *   crit 0: l1 = mean |x - y| (nn.L1Loss()), 1: fro = ||x - y||_F (torch.norm(p='fro')).  Job j: x, y [n] (n % 4 == 0, 16-byte
 *   aligned), weight = w_k, group 0 / 1 (perceptual / style total).
 *   partial (may be NULL when no loss is wanted): mrefsr_tap_crit_workspace_bytes; the sums are formed in a fixed order (double,
 *   no atomics): two calls give the same bits.  losses[j] (may be NULL) = the criterion of job j; totals[g] (may be NULL) =
 *   (sum over the jobs of group g, in order, of losses[j] * w_k) * loss_weight_g.
 *   grad (per job, may be NULL): d total / d x with torch's autograd arithmetic, times gup[group] (device, NULL = 1):
 *   l1: ((gup * loss_weight) * w_k) * inv_n * sgn(x - y) (inv_n = 1.0f / n), fro: (x - y) * (((gup * loss_weight) * w_k) / norms[j])
 *   (norms = the losses of the forward; 0 where the norm is 0); accumulate = 1 adds it to grad.  amax (may be NULL): max |grad|. */
#define MREFSR_TAP_MAX_JOBS 16
typedef struct {
    const float *x, *y;
    float *grad;
    int64_t n;
    float inv_n, weight;
    int group;
} mrefsr_tap_job;
int mrefsr_tap_crit_blocks(int64_t n);
int mrefsr_tap_crit_workspace_bytes(const mrefsr_tap_job *jobs, int n_jobs);
int mrefsr_tap_crit_f32(const mrefsr_tap_job *jobs, int n_jobs, int crit, float loss_weight0, float loss_weight1, const float *gup,
                        const float *norms, int accumulate, double *partial, float *losses, float *totals, float *amax,
                        mrefsr_stream_t stream);
/* mrefsr_gram_nhwc_f32: gram[n] = F_n^T F_n / (C HW) for f [N][HW][C] (C a multiple of 64) -> gram [N][C][C] (exactly symmetric):
 *   exact f32 products on v_mfma_f32_16x16x4_f32, upper 64 x 64 tiles only, split over the pixels into mrefsr_gram_splits parts
 *   whose partial tiles (workspace, mrefsr_gram_workspace_bytes) are added in a fixed order.
 * mrefsr_gram_bwd_nhwc_f32: df[n] (+)= (2 / (C HW)) F_n S_n with S = d style / d gram(x) of an l1 style term formed inside:
 *   S = sgn(gx - gg) * ((gup * loss_weight) * weight) / (N C C)  (gx, gg [N][C][C]; gup device, NULL = 1); accumulate = 1 adds to
 *   df [N][HW][C]; amax (may be NULL): max |df|. */
int mrefsr_gram_splits(int N, int HW, int C);
int64_t mrefsr_gram_workspace_bytes(int N, int HW, int C);
int mrefsr_gram_nhwc_f32(const float *f, int N, int HW, int C, float *gram, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);
/* the same sums times `scale` instead of 1 / (C HW) (scale = 1: the raw Gram matrix of the texture loss) */
int mrefsr_gram_nhwc_scaled_f32(const float *f, int N, int HW, int C, float scale, float *gram, void *workspace, int64_t workspace_bytes,
                                mrefsr_stream_t stream);
int mrefsr_gram_bwd_nhwc_f32(const float *f, const float *gx, const float *gg, float *df, int N, int HW, int C, const float *gup,
                             float loss_weight, float weight, int accumulate, float *amax, mrefsr_stream_t stream);
/* gradient of mrefsr_image_to_nhwc4_f32: g4 [N][HW][ld] (channels 0..2 read) -> g_img [N][3][HW] = g / std3[c] (std3 may be NULL),
 * then * 0.5 when range_norm -- torch's backward of (x + 1) * 0.5 and (x - mean) / std, bit for bit. */
int mrefsr_image_to_nhwc4_bwd_f32(const float *g4, int ld, float *g_img, int64_t N, int64_t HW, int range_norm, const float *std3,
                                  mrefsr_stream_t stream);

/* ---- ImageDiscriminator of the adversarial training step (basicsr/archs/discriminator_arch.py:10-45; the D step and the
 * generator's adversarial term of multi_ref_restoration_model.py:219-278, the gradient penalty of basicsr/models/losses.py:370-404):
 * the autograd nodes of mrefsr_amd/archs/nhwc_disc.py.  Channels-last [N][H][W][C] fp32 maps; every sum is formed in a fixed
 * order (no float atomics), so two calls give the same bits.
 *
 * mrefsr_disc_pack_image_f32: img [B][3][H][W] -> x4 [B][H][W][4] (channel 3 = 0); mrefsr_disc_unpack_image_f32: its gradient
 *   g4 [B][H][W][4] -> [B][3][H][W] (channel 3 dropped).
 * mrefsr_disc_conv_pack_weight_f32: torch's w [Cout][CinR][3][3] -> dgrad 0: [9][Cin][Cout] (the forward's B operand), 1:
 *   [9][Cout][Cin] (the input gradient's); channels CinR..Cin-1 are 0 (CinR = 3, Cin = 4 for the image).
 * mrefsr_disc_conv3x3_f32: nn.Conv2d(Cin, Cout, 3, stride, 1) + bias (bias may be NULL): x [N][H][W][Cin] -> y [N][Ho][Wo][Cout],
 *   Ho = ceil(H / stride) as torch computes it.  Implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32 products).  Cin = 4 or a
 *   multiple of 16, Cout a multiple of 16, stride 1 or 2; anything else returns MREFSR_E_UNSUPPORTED.
 * mrefsr_disc_conv3x3_dgrad_f32: input gradient dy [N][Ho][Wo][Cout] -> dx [N][H][W][Cin] (every element written) with the dgrad = 1
 *   packing; a stride-2 layer runs as four output-parity phases, each a gather over its 1-2 taps per dimension.
 * mrefsr_disc_conv3x3_wgrad_f32: dw [Cout][CinR][3][3] = sum over the pixels of x (x) dy (a GEMM over the pixels, split into partial
 *   tiles added in a fixed order; workspace: mrefsr_disc_conv3x3_wgrad_workspace_bytes). */
int mrefsr_disc_pack_image_f32(const float *img, float *x4, int B, int H, int W, mrefsr_stream_t stream);
int mrefsr_disc_unpack_image_f32(const float *g4, float *img, int B, int H, int W, mrefsr_stream_t stream);
int mrefsr_disc_conv_pack_weight_f32(const float *w, float *wpk, int Cout, int CinR, int Cin, int dgrad, mrefsr_stream_t stream);
int mrefsr_disc_conv3x3_f32(const float *x, const float *wpk, const float *bias, float *y, int N, int H, int W, int Cin, int Cout, int stride,
                            mrefsr_stream_t stream);
int mrefsr_disc_conv3x3_dgrad_f32(const float *dy, const float *wpk_d, float *dx, int N, int H, int W, int Cin, int Cout, int stride,
                                  mrefsr_stream_t stream);
int64_t mrefsr_disc_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int stride);
int mrefsr_disc_conv3x3_wgrad_f32(const float *x, const float *dy, float *dw, int N, int H, int W, int Cin, int CinR, int Cout, int stride,
                                  void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);
/* Per-channel reductions over P = N H W pixels of C channels (C a multiple of 16 for BatchNorm); workspace:
 *   mrefsr_disc_chan_workspace_bytes (double partials + merged sums).
 * mrefsr_disc_bias_grad_f32: db[c] = sum over the pixels of dy (the conv bias gradient).
 * mrefsr_disc_bn_lrelu_f32: nn.BatchNorm2d (training mode: batch mean, biased variance from per-block (count, mean, M2) partials
 *   merged in a fixed order) then LeakyReLU(slope): y = lrelu((x - mean) invstd gamma + beta); saves mean and invstd =
 *   1 / sqrt(var + eps); run_mean / run_var (may be NULL) get torch's update with momentum (variance unbiased by n / (n - 1)),
 *   *num_batches_tracked (may be NULL) += 1.
 * mrefsr_disc_bn_lrelu_bwd_f32: g = gy lrelu'(y) (the mask from the output's sign); gx = gamma invstd (g - mean g - xh mean(g xh)),
 *   ggamma = sum g xh, gbeta = sum g (any output may be NULL).
 * mrefsr_disc_bn_lrelu_dbl_f32: double backward of the above (torch's batchnorm_double_backward through the mask): from ggx and
 *   ggamma / gbeta (may be NULL = 0) -> d_gy, d_x, d_gamma (any may be NULL); the beta gradient is 0. */
int64_t mrefsr_disc_chan_workspace_bytes(int64_t P, int C);
int mrefsr_disc_bias_grad_f32(const float *dy, float *db, int64_t P, int C, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_disc_bn_lrelu_f32(const float *x, const float *gamma, const float *beta, float *y, float *mean, float *invstd, float *run_mean,
                             float *run_var, int64_t *num_batches_tracked, int64_t P, int C, float eps, float momentum, float slope,
                             void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_disc_bn_lrelu_bwd_f32(const float *gy, const float *y, const float *x, const float *mean, const float *invstd, const float *gamma,
                                 float *gx, float *ggamma, float *gbeta, int64_t P, int C, float slope, void *workspace,
                                 int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_disc_bn_lrelu_dbl_f32(const float *ggx, const float *ggamma, const float *gbeta, const float *gy, const float *y, const float *x,
                                 const float *mean, const float *invstd, const float *gamma, float *d_gy, float *d_x, float *d_gamma, int64_t P,
                                 int C, float slope, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);
/* Head: f [N][HW][C] -> AdaptiveAvgPool2d(1) -> 1x1 conv (w1 [J][C], b1 [J]) -> LeakyReLU(slope) -> 1x1 conv (w2 [J], b2 [1]) ->
 *   Sigmoid = out [N].  Saves pooled [N][C] and hidden (the pre-activation) [N][J].  C a multiple of 16 up to 2048, J up to 4096.
 * mrefsr_disc_head_bwd_f32: from gs = d / d out: gf [N][HW][C] and the parameter gradients (each may be NULL).
 * mrefsr_disc_head_dbl_f32: double backward for an upstream gradient ggf of gf alone (the gradient penalty's case): d_gs, d_f and the
 *   parameter gradients (each may be NULL).  Workspace of both: mrefsr_disc_head_workspace_bytes. */
int64_t mrefsr_disc_head_workspace_bytes(int N, int C, int J);
int mrefsr_disc_head_fwd_f32(const float *f, const float *w1, const float *b1, const float *w2, const float *b2, float *out, float *pooled,
                             float *hidden, int N, int HW, int C, int J, float slope, mrefsr_stream_t stream);
int mrefsr_disc_head_bwd_f32(const float *gs, const float *s, const float *pooled, const float *hidden, const float *w1, const float *w2,
                             float *gf, float *gw1, float *gb1, float *gw2, float *gb2, int N, int HW, int C, int J, float slope, void *workspace,
                             int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_disc_head_dbl_f32(const float *ggf, const float *gs, const float *s, const float *pooled, const float *hidden, const float *w1,
                             const float *w2, float *d_gs, float *d_f, float *d_w1, float *d_b1, float *d_w2, float *d_b2, int N, int HW, int C,
                             int J, float slope, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);

/* ---- VGGStyleDiscriminator of the adversarial training step (basicsr/archs/discriminator_arch.py:47-125 with input_size 160; the
 * same D step and penalty as above): the kernels of mrefsr_amd/archs/nhwc_vggdisc.py that the ImageDiscriminator entry points above
 * do not cover.  Its BatchNorm + LeakyReLU layers and the image packing use mrefsr_disc_bn_lrelu*_f32 and mrefsr_disc_pack_image_f32.
 * Channels-last fp32 maps, fixed summation orders (no float atomics).
 *
 * mrefsr_disc_vconv_pack_weight_f32: torch's w [Cout][CinR][ks][ks] -> dgrad 0: [Cout][ks ks][Cin] (the forward's operand), 1:
 *   [Cin][ks ks][Cout] (the input gradient's); channels CinR..Cin-1 are 0.
 * mrefsr_disc_vconv_f32: nn.Conv2d(Cin, Cout, ks, stride, 1) with ks 3 (stride 1: conv{i}_0, discriminator_arch.py:62, 66, 71, 76,
 *   81) or ks 4 (stride 2: conv{i}_1, :63, 68, 73, 78, 83) + bias (may be NULL), then LeakyReLU(slope) when act (conv0_0, :103):
 *   x [N][H][W][Cin] -> y [N][Ho][Wo][Cout], Ho = H for ks 3 and floor(H / 2) for ks 4, as torch computes them.  Implicit GEMM on
 *   v_mfma_f32_16x16x4_f32 (exact f32 products) with LDS-staged operand tiles; Cin a multiple of 4, Cout of 16.  Small layers split
 *   the reduction into partial tiles added in a fixed order (workspace: mrefsr_disc_vconv_workspace_bytes(.., dgrad 0), may be 0).
 * mrefsr_disc_vconv_dgrad_f32: input gradient dy [N][Ho][Wo][Cout] -> dx [N][H][W][Cin] (every element written) with the dgrad = 1
 *   packing; ks 4 runs as four output-parity phases, each a gather over exactly 2 x 2 taps (workspace: .._workspace_bytes(.., 1)).
 * mrefsr_disc_vconv_wgrad_f32: dw [Cout][CinR][ks][ks] = sum over the output pixels of x (x) dy, split over the pixels into partial
 *   tiles added in a fixed order (workspace: mrefsr_disc_vconv_wgrad_workspace_bytes).
 * mrefsr_disc_lrelu_mask_f32: out = g lrelu'(y), the mask from the sign of the LeakyReLU's output y: the backward of conv0_0's
 *   LeakyReLU, and (applied to the upstream gradient of its result) its double backward w.r.t. g; the one w.r.t. y is 0. */
int mrefsr_disc_vconv_pack_weight_f32(const float *w, float *wpk, int Cout, int CinR, int Cin, int ks, int dgrad, mrefsr_stream_t stream);
int64_t mrefsr_disc_vconv_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks, int dgrad);
int mrefsr_disc_vconv_f32(const float *x, const float *wpk, const float *bias, float *y, int N, int H, int W, int Cin, int Cout, int ks, int act,
                          float slope, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_disc_vconv_dgrad_f32(const float *dy, const float *wpk_d, float *dx, int N, int H, int W, int Cin, int Cout, int ks, void *workspace,
                                int64_t workspace_bytes, mrefsr_stream_t stream);
int64_t mrefsr_disc_vconv_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks);
int mrefsr_disc_vconv_wgrad_f32(const float *x, const float *dy, float *dw, int N, int H, int W, int Cin, int CinR, int Cout, int ks, void *workspace,
                                int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_disc_lrelu_mask_f32(const float *g, const float *y, float *out, int64_t n, float slope, mrefsr_stream_t stream);
/* Linear head (discriminator_arch.py:115-118): f [N][HW][C] channels-last, flattened in the reference's NCHW order (feature c HW + p,
 *   view(B, -1)) -> linear1 (w1 [J][C HW] in torch's layout, b1 [J]) -> LeakyReLU(slope) -> linear2 (w2 [J], b2 [1]) = out [N]; saves
 *   hidden (linear1's output before the activation) [N][J].
 * mrefsr_disc_linear_head_bwd_f32: from gs = d / d out: gf [N][HW][C] and the parameter gradients (each output may be NULL; f is read
 *   for gw1 only).
 * mrefsr_disc_linear_head_dbl_f32: double backward for an upstream gradient ggf of gf alone (the gradient penalty's case): d_gs, d_w1,
 *   d_w2 (each may be NULL); the gradients w.r.t. f, b1 and b2 are 0 (the LeakyReLU mask is piecewise constant).  Workspace:
 *   mrefsr_disc_linear_head_workspace_bytes. */
int mrefsr_disc_linear_head_fwd_f32(const float *f, const float *w1, const float *b1, const float *w2, const float *b2, float *out, float *hidden,
                                    int N, int HW, int C, int J, float slope, mrefsr_stream_t stream);
int mrefsr_disc_linear_head_bwd_f32(const float *gs, const float *hidden, const float *f, const float *w1, const float *w2, float *gf, float *gw1,
                                    float *gb1, float *gw2, float *gb2, int N, int HW, int C, int J, float slope, mrefsr_stream_t stream);
int64_t mrefsr_disc_linear_head_workspace_bytes(int N, int J);
int mrefsr_disc_linear_head_dbl_f32(const float *ggf, const float *gs, const float *hidden, const float *w1, const float *w2, float *d_gs,
                                    float *d_w1, float *d_w2, int N, int HW, int C, int J, float slope, void *workspace, int64_t workspace_bytes,
                                    mrefsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Validation metrics: basicsr/utils/img_util.py:38-94 (tensor2img) and basicsr/metrics/psnr_ssim.py (calculate_psnr,
 * calculate_ssim) as restated by mrefsr_amd/metrics.py, on the device (the reference runs them in numpy on the host).
 * --------------------------------------------------------------------------------------------- */

/* mrefsr_tensor2img_u8: tensor2img's quantisation, x [N][C][H][W] fp32 -> img [N][H][W][C] uint8: clamp to [0, 1], times 255.0f in
 *   fp32, round half to even, to uint8 (NaN gives 0). */
int mrefsr_tensor2img_u8(const float *x, uint8_t *img, int N, int C, int H, int W, mrefsr_stream_t stream);

/* mrefsr_val_metrics_f32: per image of out [N][3][H][W] against gt [N][3][Hg][Wg] (fp32 in [0, 1]), both quantised as above:
 *   the valid region is rows [0, oh) and columns [0, ow) (sizes [N][2] = (oh, ow) in HOST memory, the dataset's zero-padding crop;
 *   NULL: oh = H, ow = W, and the shapes must be equal); the metrics see that region less crop_border on every side, h x w.
 *   res [N][8] int64 (device), one row per image, fp64 values stored by their bits:
 *     [0] sum of squared uint8 differences over the h x w x 3 values (exact)
 *     [1] count of non-finite values of out and gt in the valid region
 *     [2] fp64 sum of squared differences of the Y planes (metrics.rgb_to_y, BT.601) over h x w
 *     [3] fp64 sum of the Y SSIM map over (h - 10) x (w - 10)        (flags & MREFSR_VALM_SSIM_Y, else 0)
 *     [4..6] the same for the R, G and B planes                       (flags & MREFSR_VALM_SSIM_RGB, else 0)
 *     [7] 0
 *   The caller forms mse = [0] / (3 h w) and 10 log10(255^2 / mse) exactly as calculate_psnr does; SSIM is the map sum over its
 *   count.  SSIM: 11 x 11 Gaussian window (sigma 1.5) as a separable "valid" filter in fp64, c1 = (0.01 * 255)^2,
 *   c2 = (0.03 * 255)^2.  Needs h, w >= 1, and >= 11 with an SSIM flag.  img: NULL, or the [N][H][W][3] uint8 image of out
 *   (mrefsr_tensor2img_u8's).  Fixed summation orders, no atomics: bitwise reproducible.  Up to 32 images per set of three
 *   launches.  Workspace: mrefsr_val_metrics_workspace_bytes. */
#define MREFSR_VALM_SSIM_Y 1
#define MREFSR_VALM_SSIM_RGB 2
int64_t mrefsr_val_metrics_workspace_bytes(int N, int H, int W);
int mrefsr_val_metrics_f32(const float *out, const float *gt, int N, int H, int W, int Hg, int Wg, const int *sizes, int crop_border,
                           int flags, uint8_t *img, int64_t *res, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);

/* ---- UNetDiscriminatorSN of the adversarial training step (basicsr/archs/discriminator_arch.py:127-200; the same D step and
 * penalty as above): the kernels of mrefsr_amd/archs/nhwc_unetdisc.py that the entry points above do not cover.  conv0 .. conv8 run
 * on mrefsr_disc_vconv*_f32 (conv1 .. conv8 with W = W_orig / sigma), the image packing on mrefsr_disc_pack_image_f32.
 * Channels-last fp32 maps, fixed summation orders (no float atomics).
 *
 * mrefsr_disc_sn_power_f32: torch.nn.utils.spectral_norm (n_power_iterations 1, dim 0) of L <= 8 layers in four launches (two when
 *   update is 0).  Host arrays of L device pointers: w[l] = W_orig as a rows[l] x cols[l] matrix, u[l] [rows], v[l] [cols].  update 1
 *   (training): v = W^T u / max(|W^T u|, eps), u = W v / max(|W v|, eps), written to u[l], v[l] in place and to the snapshots snap_u
 *   [sum rows], snap_v [sum cols] (layers concatenated); update 0 (eval): the snapshots are copies of u, v.  sigma[l] = snap_u . (W
 *   snap_v).  Workspace: mrefsr_disc_sn_workspace_bytes.
 * mrefsr_disc_sn_scale_f32: w[l] = w_orig[l] / sigma[l] (sigma in device memory) for every layer in one launch.
 * mrefsr_disc_sn_bwd_f32: dw[l] = g[l] / sigma - (<g[l], w_orig[l]> / sigma^2) u v^T with the snapshot's u, v, sigma (the gradient of
 *   W = W_orig / sigma(W_orig) at fixed u, v); the dot product split into chunks added in a fixed order.  Workspace:
 *   mrefsr_disc_sn_bwd_workspace_bytes. */
int64_t mrefsr_disc_sn_workspace_bytes(const int *rows, const int *cols, int L);
int mrefsr_disc_sn_power_f32(const float *const *w, float *const *u, float *const *v, const int *rows, const int *cols, int L, int update, float eps,
                             float *snap_u, float *snap_v, float *sigma, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_disc_sn_scale_f32(const float *const *w_orig, float *const *w, const int *rows, const int *cols, int L, const float *sigma,
                             mrefsr_stream_t stream);
int64_t mrefsr_disc_sn_bwd_workspace_bytes(const int *rows, const int *cols, int L);
int mrefsr_disc_sn_bwd_f32(const float *const *g, const float *const *w_orig, float *const *dw, const int *rows, const int *cols, int L,
                           const float *snap_u, const float *snap_v, const float *sigma, void *workspace, int64_t workspace_bytes,
                           mrefsr_stream_t stream);
/* mrefsr_disc_up2_f32: F.interpolate(y (+ skip), scale_factor=2, mode='bilinear', align_corners=False) on y [N][h][w][C] (skip may be
 *   NULL) -> out [N][2h][2w][C], C a multiple of 4 (16-byte aligned tensors).  mrefsr_disc_up2_adj_f32: its adjoint, g [N][2h][2w][C]
 *   -> out [N][h][w][C], a gather over at most 4 x 4 taps.  mrefsr_disc_add_f32: out = a + b. */
int mrefsr_disc_up2_f32(const float *y, const float *skip, float *out, int N, int h, int w, int C, mrefsr_stream_t stream);
int mrefsr_disc_up2_adj_f32(const float *g, float *out, int N, int h, int w, int C, mrefsr_stream_t stream);
int mrefsr_disc_add_f32(const float *a, const float *b, float *out, int64_t n, mrefsr_stream_t stream);
/* conv9 (nn.Conv2d(C, 1, 3, 1, 1), discriminator_arch.py:150): x [N][H][W][C] -> y [N][H][W] (+ bias[0] when bias is not NULL);
 *   w in torch's [1][C][3][3] layout; C a multiple of 4, at most 512.  _dgrad: gy [N][H][W] -> dx [N][H][W][C].  _wgrad: dw [1][C][3][3]
 *   = sum over the pixels of x (x) gy, split over pixel chunks added in a fixed order (workspace: mrefsr_disc_conv9_wgrad_workspace_bytes);
 *   the bias gradient is mrefsr_disc_bias_grad_f32 of gy. */
int mrefsr_disc_conv9_f32(const float *x, const float *w, const float *bias, float *y, int N, int H, int W, int C, mrefsr_stream_t stream);
int mrefsr_disc_conv9_dgrad_f32(const float *gy, const float *w, float *dx, int N, int H, int W, int C, mrefsr_stream_t stream);
int64_t mrefsr_disc_conv9_wgrad_workspace_bytes(int N, int H, int W, int C);
int mrefsr_disc_conv9_wgrad_f32(const float *x, const float *gy, float *dw, int N, int H, int W, int C, void *workspace, int64_t workspace_bytes,
                                mrefsr_stream_t stream);

/* ---- StyleGAN2Discriminator of the adversarial training step (basicsr/archs/stylegan2_arch.py:733-799; the same D step and penalty
 * as above): the kernels of mrefsr_amd/archs/nhwc_sg2disc.py that the entry points above do not cover.  conv1 of every ResBlock and
 * final_conv run on mrefsr_disc_vconv*_f32 (ks 3), final_linear on mrefsr_disc_linear_head*_f32, the image packing on
 * mrefsr_disc_pack_image_f32.  Channels-last fp32 maps, fixed summation orders (no float atomics).
 *
 * mrefsr_disc_sg2_fir_f32: upfirdn2d(x, outer(taps, taps), up 1, down, pad (pad0, pad1)) with a separable FIR of L = 2 .. 4 taps (HOST
 *   memory, already normalised to sum 1), down 1 or 2, on x [N][H][W][C] -> y [N][Ho][Wo][C], Ho = (H + pad0 + pad1 - L) / down + 1; C a
 *   multiple of 4.  adjoint 1: its input gradient, x = the gradient [N][Ho][Wo][C] -> y [N][H][W][C] (H, W still name the forward's
 *   input; every element written).  Both are gathers; each is the other's backward.
 * mrefsr_disc_sg2_pack_weight_f32: torch's w [Cout][CinR][ks][ks] (ks 1 or 3) -> dgrad 0: [Cout][ks ks][Cin], 1: [Cin][ks ks][Cout];
 *   channels CinR..Cin-1 are 0.
 * mrefsr_disc_sg2_conv_f32: conv2d(x, w, stride, padding 0) with ks 3 (stride 2: conv2 of a ResBlock, on the FIR's output) or ks 1
 *   (stride 1: the ResBlock's skip, on the FIR's stride-2 output, and the input stage on the packed image): x [N][H][W][Cin] ->
 *   y [N][Ho][Wo][Cout], Ho = (H - 3) / 2 + 1 or H; y = lrelu(conv + bias, slope) (bias may be NULL; LeakyReLU when act) + res (may be
 *   NULL; [N][Ho][Wo][Cout]: the ResBlock's merge).  Implicit GEMM on v_mfma_f32_16x16x4_f32 with LDS-staged operand tiles; Cin a
 *   multiple of 4, Cout of 16; small layers split the reduction into partial tiles added in a fixed order (workspace:
 *   mrefsr_disc_sg2_conv_workspace_bytes(.., dgrad 0), may be 0).
 * mrefsr_disc_sg2_conv_dgrad_f32: input gradient dy [N][Ho][Wo][Cout] -> dx [N][H][W][Cin] (every element written); ks 3 runs as four
 *   input-parity phases of 4, 2, 2 and 1 taps (workspace: .._workspace_bytes(.., 1)).
 * mrefsr_disc_sg2_conv_wgrad_f32: dw [Cout][CinR][ks][ks] = sum over the output pixels of x (x) dy, split over the pixels into partial
 *   tiles added in a fixed order (workspace: mrefsr_disc_sg2_conv_wgrad_workspace_bytes). */
int mrefsr_disc_sg2_fir_f32(const float *x, float *y, int N, int H, int W, int C, const float *taps, int L, int pad0, int pad1, int down,
                            int adjoint, mrefsr_stream_t stream);
int mrefsr_disc_sg2_pack_weight_f32(const float *w, float *wpk, int Cout, int CinR, int Cin, int ks, int dgrad, mrefsr_stream_t stream);
int64_t mrefsr_disc_sg2_conv_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks, int dgrad);
int mrefsr_disc_sg2_conv_f32(const float *x, const float *wpk, const float *bias, const float *res, float *y, int N, int H, int W, int Cin,
                             int Cout, int ks, int act, float slope, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_disc_sg2_conv_dgrad_f32(const float *dy, const float *wpk_d, float *dx, int N, int H, int W, int Cin, int Cout, int ks,
                                   void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);
int64_t mrefsr_disc_sg2_conv_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks);
int mrefsr_disc_sg2_conv_wgrad_f32(const float *x, const float *dy, float *dw, int N, int H, int W, int Cin, int CinR, int Cout, int ks,
                                   void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);

/* ---- the parameter update: Adam and the exponential moving average (EMA) of net_g, multi-tensor ---------------------------------
 * The reference's optimiser is a plain torch.optim.Adam over four parameter groups (multi_ref_restoration_model.py:60-104, stepped
 * at :277); basicsr's EMA of net_g is one mul_ and one add_ per parameter (base_model.py:75-82, model_ema; sr_model.py:118-119).
 * Here both are ONE launch over a table of jobs in DEVICE memory (as mrefsr_conv_pack_weights_multi_f32), one job per tensor:
 *   p     the parameter, n floats, 4-byte aligned (any 4-byte alignment works; streams that share their offset inside 16 bytes,
 *         as separately allocated tensors do, are moved 16 bytes at a time)
 *   g     its gradient, or NULL: the job takes no Adam step (torch skips parameters whose .grad is None); m, v the moments
 *         exp_avg / exp_avg_sq (not NULL where g is not)
 *   ema   the EMA copy of p, or NULL
 *   first_chunk   the jobs are laid end to end in chunks: first_chunk of job 0 is 0, of job j + 1 it is first_chunk[j] +
 *         mrefsr_optim_job_chunks(n[j]) (no job may get fewer chunks than that; the elements beyond them would be left out)
 *   group index into `groups` (Adam only)
 * No atomics, no workspace; a table is read-only and can be reused for as long as its addresses hold.
 *
 * mrefsr_ema_multi_f32: ema = ema * decay + p * one_minus_decay for every job with an ema (g, m, v, group are not looked at); two
 *   roundings (the product p * one_minus_decay, then one fused multiply-add).  decay == 0 copies p's bits and does not read ema
 *   (model_ema(0), the reference's initialisation).
 * mrefsr_adam_multi_f32: torch.optim.Adam's step (weight_decay added to the gradient, no amsgrad, no maximize) in fp32, the bias
 *   corrections 1 - beta^step in double from the group's values:
 *     g += weight_decay p;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;
 *     p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *   `step` is the count INCLUDING this update (>= 1).  Jobs with an ema get the EMA update of the new p in the same pass, jobs
 *   without a gradient included; ema_decay as for mrefsr_ema_multi_f32. */
typedef struct mrefsr_optim_job {
    float *p;
    const float *g;
    float *m, *v, *ema;
    int64_t n;
    int32_t first_chunk, group;
} mrefsr_optim_job;
typedef struct mrefsr_adam_group {
    double lr, beta1, beta2, eps, weight_decay;
    int64_t step;
} mrefsr_adam_group;
int mrefsr_optim_job_chunks(int64_t n); /* -1: n < 0 or n > 2^40 */
int mrefsr_ema_multi_f32(const mrefsr_optim_job *jobs, int n_jobs, float decay, float one_minus_decay, mrefsr_stream_t stream);
int mrefsr_adam_multi_f32(const mrefsr_optim_job *jobs, int n_jobs, const mrefsr_adam_group *groups, int n_groups, float ema_decay,
                          float one_minus_ema_decay, mrefsr_stream_t stream);

/* ---- gradient-norm clipping and non-finite step skipping over the same job table ------------------------------------------------
 * torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False) between backward and the update, without a host
 * synchronisation: total_norm = sqrt(sum g^2) over every job with a gradient, coef = min(max_norm / (total_norm + 1e-6), 1) in
 * fp32, the update consumes fl32(g * coef) (multiplied also when coef == 1: no bit changes).  Squares are taken and added per
 * lane in fp32, so a square -- or a lane's sum -- that overflows fp32 is inf and the norm counts as NON-FINITE although every
 * gradient element is finite (|g| above 1.8e19); lanes and blocks are added in double, in a fixed order, without atomics: the
 * same bits from run to run.  The relative error of total_norm is at most ((L + 1) / 2 + 2) 2^-24, L = 4 ceil(T / 2048) the
 * squares one lane adds, T the chunks of the table.
 *
 * mrefsr_grad_sqnorm_multi_f32: reads job.g only (jobs without one are skipped; p, m, v, ema, group are not looked at) and writes
 *   one double per block into `workspace` (mrefsr_grad_norm_workspace_bytes() bytes, 8-byte aligned, owned by the caller).
 * mrefsr_grad_norm_finalize_f32: one block; adds the workspace in index order and writes *state: total_norm (unclipped), coef
 *   (max_norm <= 0: no clipping, coef = 1; a NaN norm gives a NaN coef, an infinite one 0, as in torch), found_inf = 1 when
 *   total_norm is inf or NaN, else 0 (a float, so that it can be handed to torch's fused Adam as optimizer.found_inf), and
 *   skipped += 1 when found_inf and skip_nonfinite.  The caller zeroes *state once; `skipped` is written by this launch only.
 * mrefsr_grad_scale_multi_f32: g = fl32(g * state->coef) in place for every job with a gradient (torch's clip; for torch's Adam).
 * mrefsr_adam_multi_clip_f32: mrefsr_adam_multi_f32 on fl32(g * state->coef) formed in registers -- the gradient tensors are not
 *   written.  With skip_nonfinite and state->found_inf, no job takes its Adam step (p, m, v keep their bits) while the EMA
 *   update is done as always.  The bias corrections are taken at group.step - state->skipped (at least 1): the host may go on
 *   counting skipped steps and need not read the state back.  All entries must be launched on one stream, in this order. */
typedef struct mrefsr_grad_clip_state {
    float total_norm, coef, found_inf, reserved;
    int64_t skipped;
} mrefsr_grad_clip_state;
int64_t mrefsr_grad_norm_workspace_bytes(void);
int mrefsr_grad_sqnorm_multi_f32(const mrefsr_optim_job *jobs, int n_jobs, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_grad_norm_finalize_f32(const void *workspace, int64_t workspace_bytes, float max_norm, int skip_nonfinite,
                                  mrefsr_grad_clip_state *state, mrefsr_stream_t stream);
int mrefsr_grad_scale_multi_f32(const mrefsr_optim_job *jobs, int n_jobs, const mrefsr_grad_clip_state *state, mrefsr_stream_t stream);
int mrefsr_adam_multi_clip_f32(const mrefsr_optim_job *jobs, int n_jobs, const mrefsr_adam_group *groups, int n_groups, float ema_decay,
                               float one_minus_ema_decay, const mrefsr_grad_clip_state *state, int skip_nonfinite, mrefsr_stream_t stream);

/* ---- R1 regularisation of the discriminator (csrc/gan_reg.hip) --------------------------------------------------------------------
 * basicsr/losses/losses.py:391-405 (r1_penalty): grad_real.pow(2).view(B, -1).sum(1) of the discriminator's input gradient on the
 * real images, applied every net_d_reg_every steps in basicsr/models/stylegan2_model.py:208-219.  The discriminator's double
 * backward runs on its own nodes; these entries are the per-sample sum of squares and its backward.
 *
 * mrefsr_r1_sqnorm_f32 (losses.py:404): g is `batch` contiguous rows of n floats, the first row at any 4-byte boundary;
 *   out[b] = sum_i g[b][i]^2.  Squares are taken and added per lane in fp32 -- a lane's four elements as (q0 + q1) + (q2 + q3),
 *   then onto its accumulator -- so a square that overflows fp32 is inf, and inf / NaN elements reach out[b] as they are (no
 *   clamp); lanes, waves and the mrefsr_r1_sqnorm_row_blocks(n) blocks of a row are added in double in a fixed order, out[b] is
 *   that sum rounded to fp32.  No atomics: the same bits from run to run.  Relative error against the float64 sum of the same
 *   fp32 elements: at most (L / 4 + 3) 2^-24, below ((L + 1) / 2 + 2) 2^-24, L = 4 ceil(T / row_blocks) the squares one lane
 *   adds, T = ceil((n + 3) / 1024).  Two launches (per-block partials into `workspace`, mrefsr_r1_sqnorm_workspace_bytes(batch, n)
 *   bytes, 8-byte aligned, owned by the caller; then one block per row).
 * mrefsr_r1_sqnorm_bwd_f32 (the backward of losses.py:404 towards grad_real): gg[b][i] = fl32(fl32(2 gs[b]) g[b][i]), the bits of
 *   torch's g * (2 * gs).view(B, 1); gg has g's layout and may sit at any 4-byte boundary too.  One launch.
 * batch in 1..65535, n in 1..2^40 (the -1 of the two size queries otherwise). */
int mrefsr_r1_sqnorm_row_blocks(int64_t n);
int64_t mrefsr_r1_sqnorm_workspace_bytes(int batch, int64_t n);
int mrefsr_r1_sqnorm_f32(const float *g, int batch, int64_t n, float *out, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_r1_sqnorm_bwd_f32(const float *g, const float *gs, int batch, int64_t n, float *gg, mrefsr_stream_t stream);

/* ---- differentiable discriminator augmentation (csrc/disc_augment.hip; train.d_augment) -------------------------------------------
 * No reference counterpart: the colour, translation, cutout and flip operators of DiffAugment (Zhao et al., NeurIPS 2020) and of
 * ADA's pipeline (Karras et al., NeurIPS 2020), one random transformation T per sample in front of every discriminator call.  For
 * fixed parameters T(x) = L x + b, L linear.  Images fp32 [B][3][H][W]; fpar [B][4] = {db, s, c, unused}: brightness offset,
 * saturation factor, contrast factor; ipar [B][8] = {flip, ty, tx, y0, y1, x0, x1, unused}: horizontal flip (0 / 1), integer
 * translation (any value), cut box [y0,y1) x [x0,x1).  Both tables in device memory.  N = 3 H W.
 *
 * mrefsr_disc_augment_f32: output pixel (y, x) of sample b, every line one fp32 operation in this order, nothing fused:
 *     inside the cut box, or sy = y - ty, sx0 = x - tx outside the image:  out_ch = 0 (selected: a NaN there does not get out)
 *     sx = flip ? W - 1 - sx0 : sx0;   v_ch = in[b][ch][sy][sx] + db;   mu = ((v_0 + v_1) + v_2) / 3
 *     u_ch = s v_ch + (1 - s) mu;      m = fl32(sum_b / N) + db;        out_ch = c u_ch + (1 - c) m
 *   sum_b: the sample's N inputs added in double in a fixed order (a NaN anywhere in the sample reaches every pixel of it through
 *   m).  Identity parameters (0, 1, 1, no flip, no shift, empty box) return the input's values.  with_bias = 0 takes db as 0 in
 *   both places: L x, the node of the second derivative.
 * mrefsr_disc_augment_adj_f32: gx = L^T g.  Source pixel (sy, sx) is read by output pixel y = sy + ty, x = (flip ? W - 1 - sx : sx)
 *   + tx alone;  G_ch = g[b][ch][y][x] if that pixel is inside the image and outside the cut box, else 0 (selected);
 *     gx_ch = c (s G_ch + (1 - s) ((G_0 + G_1) + G_2) / 3) + fl32((1 - c) / N) fl32(S_b)
 *   S_b: g over the sample's kept output pixels, added in double in a fixed order.  The brightness bias has no adjoint term.
 * contrast = 0 is the caller's statement that c = 1 in every sample: c is taken as 1, m and S_b as 0, the sum launch is skipped and
 *   workspace / ticket may be NULL (one launch).  Otherwise two launches: per-block double partials and, by the block that arrives
 *   last, the per-sample sums into `workspace` (mrefsr_disc_augment_workspace_bytes(B, H, W) bytes, 8-byte aligned, the caller's),
 *   then the apply pass.  `ticket`: one zeroed word that every launch leaves zero again.  No float atomics, no readback, the same
 *   bits from call to call.  Absolute error against the same formulas in float64: at most 16 * 2^-24 * max(U, |c| U + |1 - c| A) (13 for the adjoint),
 *   A = max |in| + |db| (max |g| for the adjoint), U = (|s| + |1 - s|) A.
 * B in 1..65535, H W in 1..2^28 (the -1 of the size query otherwise); out / gx must not alias the input. */
int64_t mrefsr_disc_augment_workspace_bytes(int B, int H, int W);
int mrefsr_disc_augment_f32(const float *x, const float *fpar, const int *ipar, int B, int H, int W, int with_bias, int contrast, float *out,
                            void *workspace, int64_t workspace_bytes, unsigned int *ticket, mrefsr_stream_t stream);
int mrefsr_disc_augment_adj_f32(const float *g, const float *fpar, const int *ipar, int B, int H, int W, int contrast, float *gx,
                                void *workspace, int64_t workspace_bytes, unsigned int *ticket, mrefsr_stream_t stream);

/* ---- the x8 geometric self-ensemble of test() (csrc/selfens.hip; val.self_ensemble) ------------------------------------------------
 * No reference counterpart: the "+" evaluation protocol of EDSR and its successors.  Copy j in 0..3 of a group has hf = j & 1,
 * vf = (j >> 1) & 1; a group is untransposed (tr = 0) or transposed (tr = 1).  Copy j of src [..., H, W] is, in torch,
 *     s = src;  if hf: s = s.flip(-1);  if vf: s = s.flip(-2);  if tr: s = s.transpose(-1, -2)
 * (the order of data/multi_ref_dataset.py: augment), and the inverse x' of an output x of that copy is
 *     o = x;    if tr: o = o.transpose(-1, -2);  if vf: o = o.flip(-2);  if hf: o = o.flip(-1).
 * Contiguous fp32 at any 4-byte boundary, any H, W >= 1 with H W <= 2^30, at most 2^31 - 1 tiles of 32 x 32 per launch; 16-byte
 * accesses when the pointers are 16-byte aligned, W % 4 == 0 and (tr = 1, merge) H % 4 == 0, 4-byte accesses otherwise; the
 * transposed group goes through a 32 x 33-word LDS tile (global reads and writes both along rows).  Nothing is allocated, nothing
 * is synchronised.
 *
 * mrefsr_dihedral_expand_f32: src [outer][inner][C][H][W] -> dst [outer][4][inner][C][Ho][Wo], (Ho, Wo) = tr ? (W, H) : (H, W);
 *   dst[o][j][i] is copy j of src[o][i].  outer = K turns the k-major reference stack [K][B] into the k-major stack [K][4][B] of
 *   the expanded batch in one launch; images and LR inputs take outer = 1.  A pure copy of 32-bit words: bit-identical to the
 *   torch statement, NaN payloads, infinities and -0 included.  dst must not overlap src.
 * mrefsr_dihedral_merge_f32: a [4][N][C][H][W] (outputs of the untransposed group), b [4][N][C][W][H] (of the transposed group)
 *   -> out [N][C][H][W] = (((((((a0' + a1') + a2') + a3') + b0') + b1') + b2') + b3') * 0.125f: fp32 adds in exactly this order, one
 *   multiply behind them; bit-identical to the same chain written in torch.  out must not overlap a or b. */
int mrefsr_dihedral_expand_f32(const float *src, float *dst, int outer, int inner, int C, int H, int W, int tr, mrefsr_stream_t stream);
int mrefsr_dihedral_merge_f32(const float *a, const float *b, float *out, int N, int C, int H, int W, mrefsr_stream_t stream);

/* ---- colour correction of test() outputs towards the LQ image (csrc/color_fix.hip; val.color_fix) ----------------------------------
 * No reference counterpart: the "color fix" of StableSR (Wang et al., IJCV 2024).  x the output, s the colour source, out, all fp32
 * [B][C][H][W] at any 4-byte boundary, every (b, c) plane on its own; out must not alias x or s, which are only read.  sizes: NULL
 * (whole planes) or [B][2] int32 (h_b, w_b) in DEVICE memory, read by the kernels: the top-left h_b x w_b rectangle of sample b is
 * the image -- statistics and filters see it alone, with its border as the image border --, and every pixel outside it keeps x's
 * bits.  The caller checks 1 <= h_b <= H, 1 <= w_b <= W (the kernels clamp the values into that range, so no access leaves the
 * buffers).  Nothing is clamped to [0, 1].  16-byte accesses when the pointers are 16-byte aligned and W % 4 == 0, 4-byte accesses
 * otherwise, the same bits either way.  The same bits from call to call.
 *
 * mrefsr_color_fix_wavelet_f32: out = x + low_L(s - x), L = levels in 1..5; low_0(v) = v, low_i(v) = low_{i-1}(v) filtered with
 *   [1,2,1]^T [1,2,1] / 16 at dilation 2^(i-1), reads clamped to the rectangle at every stage (replicate padding).  One launch, one
 *   block per 64 x 64 tile of a plane; the tile and a halo of 2^L - 1 pixels of s - x in LDS, the 2 L separable passes there in
 *   place, each  0.25f * (a + c) + 0.5f * b  with two fp32 roundings; where the filtered difference is 0 the output is x's bits (so
 *   s bit-equal to x returns x).  |out - exact| <= (4 L + 1) 2^-24 max |s - x| + 2^-24 |exact|.
 *   H, W >= 1, H W <= 2^30, at most 2^31 - 1 tiles; MREFSR_E_INVALID for a null pointer, a non-positive dimension or levels
 *   outside 1..5.
 * mrefsr_color_fix_adain_f32: out = (x - mu_x) (sigma_s / sigma_x) + mu_s; mu the mean and sigma = sqrt(var + 1e-5), var the
 *   unbiased variance, over the plane's rectangle (one pixel has none: MREFSR_E_INVALID for H W = 1 without sizes; with sizes the
 *   caller checks).  Two launches: per-block (count, mean, M2) of x and of s in double and, by the block that arrives last, their
 *   merge per plane in ascending block order into `workspace` (mrefsr_color_fix_adain_workspace_bytes(B, C, H, W) bytes, 8-byte
 *   aligned, the caller's; -1 for a shape outside B C in 1..65535, H W in 1..2^30); then the apply pass, in double with ONE
 *   rounding to fp32.  `ticket`: one zeroed word that every call leaves zero again.  No float atomics, no readback. */
int mrefsr_color_fix_wavelet_f32(const float *x, const float *s, float *out, int B, int C, int H, int W, const int32_t *sizes, int levels,
                                 mrefsr_stream_t stream);
int64_t mrefsr_color_fix_adain_workspace_bytes(int B, int C, int H, int W);
int mrefsr_color_fix_adain_f32(const float *x, const float *s, float *out, int B, int C, int H, int W, const int32_t *sizes, void *workspace,
                               int64_t workspace_bytes, uint32_t *ticket, mrefsr_stream_t stream);

/* ---- homography views of image batches and the matcher's score against a known homography (csrc/warp.hip; mrefsr_amd/views.py) ---
 * The reference makes its views on the host (image_pair_generation_perspective of basicsr/data/ref_cufed_dataset.py:190-272:
 * cv2.warpPerspective, INTER_CUBIC); bit parity with OpenCV is not claimed and its uint8 round trip is not reproduced.
 *
 * mrefsr_warp_persp_f32: x [N][C][H][W] fp32 -> y [N][C][Ho][Wo], y not x.  S [N][9] DOUBLE in device memory, row-major: the SAMPLING
 *   matrix of image n, destination -> source, in integer pixel coordinates (pixel (x, y) is at (x, y)) -- cv2.warpPerspective's
 *   dst(x, y) = src(M^-1 (x, y, 1)) with S = M^-1.  (u, v, t) = S (xo, yo, 1), sx = u / t, sy = v / t in double; floor and the
 *   fraction in double, the fraction rounded once to fp32.  interp 1: the 4 x 4 cubic convolution with A = -0.75 (OpenCV's and
 *   torch.grid_sample's kernel); interp 0: bilinear.  Weights and the separable sum (along x, then along y) in fp32 in the order
 *   csrc/warp.hip spells out; a fraction of 0 gives the weights exactly [0, 1, 0, 0], of 1 exactly [0, 0, 1, 0].  Taps outside the
 *   image contribute 0.  The output is exactly 0 where t is not > 0, where a coordinate is not finite and where no tap is inside
 *   the image.  clamp 1: the result clamped to [0, 1]; 0: not.  For finite inputs the identity returns the input's bits (-0 as +0),
 *   an integer translation shifted bits and exact zeros, a zero image zeros.  |y - exact| <= 70 2^-24 max |x|, bilinear 7.  One
 *   launch; coordinate and weights once per pixel for all C channels; no atomics, no readback; the same bits from call to call.
 *   MREFSR_E_INVALID for a null pointer, y == x, a non-positive size, an interp or clamp that is not 0 or 1, H W or Ho Wo > 2^30, Ho > 524280, N > 65535.
 * mrefsr_match_stats_f64: max_idx [N][h-2][w-2] int64, the matcher's output (my = idx / (w - 2), mx = idx % (w - 2), as
 *   mrefsr_offsets_from_idx_f32 decodes it); M [N][9] double in device memory maps a QUERY position to its true REFERENCE position
 *   in feature coordinates; thr [T] doubles in HOST memory, T in 0..4; stats [N][2 + T] double in device memory.  For the query patch
 *   with top-left (qx, qy): centre c = (qx + 1, qy + 1), true top-left t = M c - 1 (M's third coordinate at c must be > 0); it
 *   counts if (qx, qy) and t both satisfy margin <= x <= x_hi - margin and margin <= y <= y_hi - margin (x_hi <= w - 3, y_hi <=
 *   h - 3: the last top-left of the valid rectangle).  stats[n] = (count, sum of |(mx, my) - t|_2, per threshold the number of
 *   counted queries with an error <= thr).  All in double; one block per n, the fixed halving tree of reduce.h; no atomics. */
int mrefsr_warp_persp_f32(const float *x, const double *S, float *y, int N, int C, int H, int W, int Ho, int Wo, int interp, int clamp,
                          mrefsr_stream_t stream);
int mrefsr_match_stats_f64(const int64_t *max_idx, const double *M, const double *thr, double *stats, int N, int h, int w, int y_hi, int x_hi,
                           int margin, int T, mrefsr_stream_t stream);

/* ---- the texture loss of the training step and its swapped reference maps (csrc/texture.hip; train.texture_opt) ---------------------
 * TextureLoss.forward(x, maps, weights) of basicsr/models/losses.py:430-532 with use_weights and a tensor `weights`; the maps and
 * weights themselves have no reference counterpart (the reference model reads them, nothing sets them): DESIGN 3.13.
 * LR map h x w at relu3_1, match grid gh x gw = (h - 2) x (w - 2), P = gh gw, scales s = 1, 2, 4.
 *
 * mrefsr_texture_select_f32: idx (int64), val [K][B][P] -> sel [B][P] = the reference k whose bit is set in valid_bits[b] (NULL: all
 *   present) with the largest val, the lowest such k among equal values; weights [B][P] = that value; pidx [B][P] = idx[sel].
 * mrefsr_texture_swap_nhwc_f32: feat [K][B][s h][s w][C] (C % 4 == 0, 16-byte aligned) -> out [B][s h][s w][C]: every match position
 *   (y, x) pastes the 3 s x 3 s reference patch at (s iy, s ix), (iy, ix) = divmod(pidx, gw), of reference sel over (s y, s x);
 *   out = (sum of the 1..9 patches that cover the pixel, added in ascending (y, x) order in fp32) / their number, the division
 *   correctly rounded.  sel and pidx are clamped to their ranges: no read leaves feat.
 * mrefsr_texture_coeff_f32: weights [B][gh][gw] -> c_s [B][s h][s w] = sigmoid(-20 u + 0.65), u = bicubic resize by s with
 *   align_corners (torch's upsample_bicubic2d: A = -0.75, clamped taps) of the weights replicate-padded by 1; evaluated in fp64 and
 *   rounded once.  Any of c1, c2, c4 may be NULL.
 * mrefsr_texture_scale_nhwc_f32: out [n_px][C] = f [n_px][C] * coeff [n_px].
 * mrefsr_texture_crit_f32: per layer norms[l] = ||gx - gm||_F over its n = N C C elements (fp64 sums in a fixed order through
 *   partial, a workspace of MREFSR_TEXTURE_MAX_LAYERS * MREFSR_TEXTURE_CRIT_BLOCKS doubles),
 *   terms[l] = norms[l] / 4 / div, total = ((sum_l terms[l]) / 3) * loss_weight (fp32, layers in the given order).
 * mrefsr_texture_gram_bwd_nhwc_f32: df [N][HW][C] (+)= coeff (.) (2 Fc (gx - gm)) * ((gup * scale) / norm), all zeros where
 *   *norm == 0; fc = f (.) coeff, gx = its raw Gram matrix, scale = loss_weight / 3 / 4 / div of the layer, gup device (NULL = 1);
 *   v_mfma_f32_16x16x4_f32, C a multiple of 64; amax (may be NULL): max |df| into a zeroed word. */
#define MREFSR_TEXTURE_MAX_LAYERS 3
#define MREFSR_TEXTURE_CRIT_BLOCKS 64
typedef struct mrefsr_texture_layer {
    const float *gx, *gm;
    int64_t n;
    float div;
} mrefsr_texture_layer;
int mrefsr_texture_select_f32(const int64_t *idx, const float *val, const int32_t *valid_bits, int32_t *sel, float *weights, int32_t *pidx, int K,
                              int B, int64_t P, mrefsr_stream_t stream);
int mrefsr_texture_swap_nhwc_f32(const float *feat, const int32_t *sel, const int32_t *pidx, float *out, int K, int B, int h, int w, int s, int C,
                                 mrefsr_stream_t stream);
int mrefsr_texture_coeff_f32(const float *weights, float *c1, float *c2, float *c4, int B, int h, int w, mrefsr_stream_t stream);
int mrefsr_texture_scale_nhwc_f32(const float *f, const float *coeff, float *out, int64_t n_px, int C, mrefsr_stream_t stream);
int mrefsr_texture_crit_f32(const mrefsr_texture_layer *layers, int n_layers, float loss_weight, double *partial, float *norms, float *terms,
                            float *total, mrefsr_stream_t stream);
int mrefsr_texture_gram_bwd_nhwc_f32(const float *fc, const float *gx, const float *gm, const float *coeff, const float *norm, const float *gup,
                                     float *df, int N, int HW, int C, float scale, int accumulate, float *amax, mrefsr_stream_t stream);

/* ---- reference pools: each sample's K best of N candidate references (csrc/refselect.hip; ref_select) -----------------------------
 * No reference counterpart.  val [N][B][P]: the matcher's winning correlation of candidate n, sample b at match
 * position p (k-major, as mrefsr_corr_top1_f32 writes it for the pool stack).  valid_bits [B] (NULL: all present): bit n of word b
 * = candidate n of sample b is present; N = 32 uses bit 31.
 *
 * mrefsr_ref_select_f32: scores [B][N], sel [B][K], slot_bits [B]; workspace of mrefsr_ref_select_workspace_bytes(N, B, P) bytes.
 *   score, mode MREFSR_REF_SCORE_MEAN: (sum_p val[n][b][p]) / P in fp32.  The sum's order depends on P alone, not on N, B or the
 *     grid: chunks of MREFSR_REF_SELECT_CHUNK positions; inside a chunk thread t of 256 adds its positions t, t + 256, .. in
 *     ascending order, the 256 sums are added by the tree a[t] += a[t + w], w = 128 .. 1, the chunks' results in ascending order;
 *     one correctly rounded division by (float)P.  No float atomics: two calls return the same bits.
 *   score, mode MREFSR_REF_SCORE_WINS: the number of positions at which n is the present candidate with the largest val, the lowest
 *     n among equal values (the rule of mrefsr_texture_select_f32); a NaN never wins a position.  An exact integer (P <= 2^24).
 *   scores[b][n] of an absent candidate is -inf.  The present candidates are ordered by (score descending, n ascending), a NaN
 *   score behind every number; the first min(K, present) are kept and written to sel[b][0..] in ASCENDING n, -1 behind them;
 *   slot_bits[b] has one bit set per filled slot ((1 << kept) - 1).  N, K in 1..32 (K may exceed N), B <= 65535.
 * mrefsr_ref_gather: src [N][B] rows, dst [K][B] rows of row_bytes bytes each (whole 4-byte words): dst row k B + b = src row
 *   sel[b][k] B + b, or zeros where sel[b][k] is outside 0..N-1 (no read leaves src).  Exactly the K B rows of dst are written.  16-byte
 *   accesses when src, dst and row_bytes are multiples of 16, else 8-byte ones when they are multiples of 8 (int64 index maps with an
 *   odd P), else 4-byte ones.  A copy of words: every bit pattern survives.  dst must not overlap src.  K B <= 65535. */
#define MREFSR_REF_SELECT_CHUNK 1024
#define MREFSR_REF_SCORE_MEAN 0
#define MREFSR_REF_SCORE_WINS 1
int64_t mrefsr_ref_select_workspace_bytes(int N, int B, int64_t P);
int mrefsr_ref_select_f32(const float *val, const int32_t *valid_bits, float *scores, int32_t *sel, int32_t *slot_bits, int N, int B, int64_t P,
                          int K, int mode, void *workspace, int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_ref_gather(const void *src, void *dst, const int32_t *sel, int N, int B, int K, int64_t row_bytes, mrefsr_stream_t stream);

/* ---- SSIM loss of the training step (csrc/ssim_loss.hip; losses.SSIMLoss, train.ssim_opt) -------------------------------------
 * No reference counterpart: loss_weight (1 - mean m), m the SSIM map of the validation metric (11-tap Gaussian window,
 * sigma 1.5, valid region, C1 = (0.01 255)^2, C2 = (0.03 255)^2) in fp32 on the images as they are (nominal range [0, 1], nothing
 * clamped or quantised).  pred, target [batch][3][h][w] contiguous; rgb = 0: one plane per image, X = 65.481 R + 128.553 G +
 * 24.966 B + 16; rgb = 1: three planes per image, X = 255 x.  planes = (rgb ? 3 : 1) batch; the map is (h - 10) x (w - 10).
 * batch <= 21845, 11 <= h, w <= 2^19, h w <= 2^30.
 *
 * mrefsr_ssim_loss_blocks: the blocks of the forward launch = the floats of `partial` (16 x 32 map positions per block); -1 for a
 *   shape outside the limits.
 * mrefsr_ssim_loss_fwd_f32: loss[0] = fl32(loss_weight (1 - sum m / count)).  Second moments are taken about a per-tile reference
 *   value, so flat regions do not cancel at 255 scale.  The sum: fixed order inside a block (fp32), one partial per block, the
 *   partials in ascending block order in double by the block that draws the last `ticket` (one zeroed word; left zero): no float
 *   atomics, the same bits from call to call.  a, b, c (all three or all NULL): the coefficient maps [planes][h - 10][w - 10]
 *   dm/d mu_x, dm/d E[x^2], dm/d E[xy] the backward reads.  pred and target are only read.
 * mrefsr_ssim_loss_bwd_f32: grad_pred [batch][3][h][w], every element written once: (-loss_weight / count) grad_loss[0] times
 *   ((G^T a) + 2 X (G^T b) + Y (G^T c)) mapped back to R, G, B with the plane's coefficients; G^T = the window over the maps
 *   zero-extended by 10.  grad_loss: the upstream gradient, one float in device memory.  One launch. */
int mrefsr_ssim_loss_blocks(int batch, int h, int w, int rgb);
int mrefsr_ssim_loss_fwd_f32(const float *pred, const float *target, int batch, int h, int w, int rgb, float loss_weight, float *a, float *b,
                             float *c, float *partial, uint32_t *ticket, float *loss, mrefsr_stream_t stream);
int mrefsr_ssim_loss_bwd_f32(const float *pred, const float *target, const float *a, const float *b, const float *c, const float *grad_loss,
                             int batch, int h, int w, int rgb, float loss_weight, float *grad_pred, mrefsr_stream_t stream);

/* ---- Multi-scale SSIM: loss of the training step and metric of validation (csrc/msssim.hip; losses.MSSSIMLoss, train.msssim_opt,
 * metrics.validation_metrics(msssim=True)) ----------------------------------------------------------------------------
 * No reference counterpart.  MS-SSIM of Wang, Simoncelli and Bovik (2003) with the window and constants of mrefsr_ssim_loss_* at
 * every level, in fp32 on the images as they are.  pred, target [batch][3][h][w] contiguous; planes as in the SSIM loss (rgb = 0: Y,
 * one per image; rgb = 1: 255 x, three per image).  Level 1 is the plane, level j + 1 the 2 x 2 mean of level j with stride 2 (a
 * trailing odd row or column is dropped): h_j = h >> (j - 1).  F[p][j] = mean of cs = (2 sigma_xy + C2) / (sigma_x^2 + sigma_y^2 +
 * C2) over level j's (h_j - 10) x (w_j - 10) map for j < levels, mean of l cs (the SSIM map) at j = levels; v[p] = prod_j
 * F[p][j]^weights[j] when every F[p][j] > 0, otherwise 0 with gradient exactly 0; loss = loss_weight (1 - mean_p v[p]).
 * Limits: 1 <= levels <= MREFSR_MSSSIM_MAX_LEVELS, min(h, w) >> (levels - 1) >= 11, batch <= 21845, h, w <= 2^19, h w <= 2^30, at
 * most 2^30 blocks; weights[0 .. levels) (host memory) finite and > 0, used as given.
 *
 * mrefsr_msssim_pyramid_floats / _map_floats: the floats of `pyramid` (pred's levels, then target's; level j as [planes][h_j][w_j])
 *   and of `maps` (the sets a, b, c; level j as [planes][h_j - 10][w_j - 10]); mrefsr_msssim_workspace_bytes: the bytes of the
 *   forward's (backward = 0) or the backward's (backward = 1; 0 bytes when levels = 1) workspace.  Each -1 for a shape outside the
 *   limits.  A workspace is dead when the call's launches are enqueued; pyramid, maps and mult carry the forward to the backward.
 * mrefsr_msssim_loss_fwd_f32: three launches (pyramid; window statistics of all levels, moments about a per-tile reference value,
 *   one fp32 partial per block; one block that adds each (plane, level)'s partials in double in a fixed order and forms v, the loss
 *   and the multipliers).  loss[0] = fl32(loss_weight (1 - sum_p v[p] / planes)).  maps and mult [planes][levels] (both or both
 *   NULL): the coefficient maps d cs/d mu_x, d cs/d E[x^2], d cs/d E[xy] (level `levels`: those of the SSIM map) and mult[p][j] =
 *   weights[j] v[p] / F[p][j] / count_j (0 under the zero rule).  values (or NULL): v[p] in double, [planes].  No float atomics: the
 *   same bits from call to call.  pred and target are only read.
 * mrefsr_msssim_loss_bwd_f32: grad_pred [batch][3][h][w], every element written once.  Level j's own term g_j = mult[p][j] ((G^T a)
 *   + 2 X_j (G^T b) + Y_j (G^T c)), G^T = the window over the maps zero-extended by 10 (exactly 0 where mult is 0); d_j = g_j +
 *   d_{j+1}(y >> 1, x >> 1) / 4 inside the pooled region; grad = (-loss_weight / planes) grad_loss[0] d_1 mapped back to R, G, B.
 *   grad_loss: the upstream gradient, one float in device memory.  Two launches (own terms of the levels 2 .. levels into the
 *   workspace; level 1 and the sum), one when levels = 1. */
#define MREFSR_MSSSIM_MAX_LEVELS 5
int64_t mrefsr_msssim_pyramid_floats(int batch, int h, int w, int rgb, int levels);
int64_t mrefsr_msssim_map_floats(int batch, int h, int w, int rgb, int levels);
int64_t mrefsr_msssim_workspace_bytes(int batch, int h, int w, int rgb, int levels, int backward);
int mrefsr_msssim_loss_fwd_f32(const float *pred, const float *target, int batch, int h, int w, int rgb, int levels, const double *weights,
                               float loss_weight, float *pyramid, float *maps, float *mult, double *values, void *workspace,
                               int64_t workspace_bytes, float *loss, mrefsr_stream_t stream);
int mrefsr_msssim_loss_bwd_f32(const float *pyramid, const float *maps, const float *mult, const float *grad_loss, int batch, int h, int w,
                               int rgb, int levels, float loss_weight, void *workspace, int64_t workspace_bytes, float *grad_pred,
                               mrefsr_stream_t stream);

/* ---- LDL artifact loss of the training step (csrc/ldl_loss.hip; losses.LDLLoss, train.ldl_opt) -----------------------
 * basicsr/losses/loss_util.py:99-145 as used by basicsr/models/realesrgan_model.py:211-226, the weight map NOT detached.  pred,
 * target, ema [batch][3][h][w] contiguous fp32; r = sum_c |target - pred|, r_e = sum_c |target - ema| (channels added 0, 1, 2);
 * g_b = Var(r_b)^(1/5) (unbiased over h w; 0 for a variance of exactly 0), v = the unbiased variance of r over the 7 x 7 window of
 * the image reflect-padded by 3, m = [r >= r_e]; loss = loss_weight / (3 batch h w) sum_b g_b sum_p v m r.
 * batch <= 65535, 4 <= h, w <= 2^19, h w <= 2^30.
 *
 * mrefsr_ldl_loss_blocks: the blocks of the forward launch (16 x 32 pixels each); `partial` holds 4 floats per block.  -1 for a
 *   shape outside the limits.
 * mrefsr_ldl_loss_fwd_f32: one launch.  Window variances in two passes over the 49 taps (the mean from the deviations about the
 *   centre tap, then the squares about it); per block
 *   (count, mean, M2) of r and sum v m r in fp32 by a fixed tree, merged per sample in ascending block order in double (the mean, then
 *   M2 about it) by the block that
 *   draws the last `ticket` (one zeroed word; left zero), which writes stats [batch][4] = (g_b, mean(r_b), k_b, S_b) with
 *   S_b = sum_p v m r and k_b = S_b (1/5) Var_b^(-4/5) 2 / (h w - 1) (0 for a variance of 0), and loss[0].  No float atomics, the
 *   same bits from call to call.  mr, mu (both or both NULL): the maps [batch][h][w] m r and the window means the backward reads;
 *   vm (or NULL): v m, read by the backward and by mrefsr_ldl_loss_map_f32.  The inputs are only read.
 * mrefsr_ldl_loss_bwd_f32: one launch; grad_pred [batch][3][h][w], every element written once:
 *   sign(pred_c - target_c) s [g v m + (2 / 48) g sum_q mult(q, p) (m r)_q (r_p - mu_q) + k_b (r_p - mean_b)], s = loss_weight /
 *   (3 batch h w) grad_loss[0]; mult(q, p): the positions of q's padded window that reflect onto p.  grad_loss: the upstream
 *   gradient, one float in device memory.  A sample with a variance of 0 gets a gradient of 0.
 * mrefsr_ldl_loss_map_f32: w [batch][h][w] = g_b (v m), the artifact map.  One launch. */
int mrefsr_ldl_loss_blocks(int batch, int h, int w);
int mrefsr_ldl_loss_fwd_f32(const float *pred, const float *target, const float *ema, int batch, int h, int w, float loss_weight, float *mr,
                            float *mu, float *vm, float *stats, float *partial, uint32_t *ticket, float *loss, mrefsr_stream_t stream);
int mrefsr_ldl_loss_bwd_f32(const float *pred, const float *target, const float *mr, const float *mu, const float *vm, const float *stats,
                            const float *grad_loss, int batch, int h, int w, float loss_weight, float *grad_pred, mrefsr_stream_t stream);
int mrefsr_ldl_loss_map_f32(const float *vm, const float *stats, int batch, int h, int w, float *wmap, mrefsr_stream_t stream);

/* ---- Real-ESRGAN second-order degradation (csrc/degrade.hip; mrefsr_amd/degradation.py, opt['degradation']) ------------
 * Forward only.  Images [batch][c][h][w] contiguous fp32; batch c <= 65535, h, w <= 2^19, h w <= 2^30.  Every shape is checked
 * before any launch.  No entry works in place.
 *
 * mrefsr_degrade_filter2d_f32: filter2D of basicsr/utils/img_process_util.py:7-31: the k x k correlation (k odd, 3 ... 21) of the
 *   image reflect-padded by k / 2 (by index arithmetic; h, w > k / 2), kernels [batch][k][k], or [1][k][k] with shared != 0.
 *   One launch, a halo tile in LDS.
 * mrefsr_degrade_usm_f32: USMSharp.forward of img_process_util.py:63-83: blur = the separable Gaussian `taps` (k floats in HOST
 *   memory, k odd, 3 ... 51, h, w > k / 2; cv2.getGaussianKernel(k, 0)'s values) over the reflect-padded image, r = img - blur,
 *   soft = blur([|r| 255 > threshold]), out = soft clip(img + weight r, 0, 1) + (1 - soft) img.  Two launches; `residual`
 *   (the image's size) holds r between them.
 * mrefsr_degrade_resize_f32: F.interpolate(align_corners=False, no antialiasing) to oh x ow as realesrgan_model.py:95, 126, 151,
 *   164 call it; mode 0 area (adaptive_avg_pool2d's windows floor(i in / out) ... ceil((i + 1) in / out); the scales are not read),
 *   1 bilinear, 2 bicubic (A = -0.75).  scale_h, scale_w map output to input coordinates, src = scale (dst + 0.5) - 0.5: torch takes
 *   1 / scale_factor when it is called with scale_factor, in / out when it is called with size.
 * mrefsr_degrade_noise_f32: basicsr/data/degradations.py:461-514 (mode 0) and :610-684 (mode 1) on c = 3 images, in the
 *   reference's operation order.  noise [batch][3][h][w], noise_gray [batch][1][h][w]; param, gray [batch] (sigma_b or scale_b; the
 *   gray flag 0 or 1).  mode 0: out = clamp(img + ((n sigma / 255) (1 - gray) + (n_gray sigma / 255) gray), 0, 1), n standard
 *   normal draws.  mode 1: n, n_gray are Poisson draws of rate l vals_b0 and l_gray vals_b1, l = clamp(round(img 255), 0, 255) / 255
 *   (l_gray: of 0.2989 R + 0.587 G + 0.114 B); out = clamp(img + ((n / vals_b0 - l) (1 - gray) + (n_gray / vals_b1 - l_gray) gray)
 *   scale, 0, 1); vals [batch][2] from mrefsr_degrade_levels_f32.
 * mrefsr_degrade_levels_f32: vals[b] = (2^ceil(log2(#distinct levels of the three channels)), the same of the gray image), what
 *   degradations.py:630-648 reads back per sample with len(torch.unique(...)).  One launch, no readback.  sets:
 *   mrefsr_degrade_levels_workspace_words(batch) 32-bit words, zero on entry and left zero.
 * mrefsr_degrade_jpeg_f32: DiffJPEG(differentiable=False) of basicsr/utils/diffjpeg.py:449-491 on c = 3 images in [0, 1];
 *   quality [batch] in device memory (0 < quality <= 100; the factor as diffjpeg.py:32-45).  One launch, one block per 16 x 16
 *   macroblock, nothing intermediate in device memory; the zero padding to multiples of 16 is a predicate. */
int mrefsr_degrade_filter2d_f32(const float *img, const float *kernels, int batch, int c, int h, int w, int k, int shared, float *out,
                                mrefsr_stream_t stream);
int mrefsr_degrade_usm_f32(const float *img, const float *taps, int batch, int c, int h, int w, int k, float weight, float threshold,
                           float *residual, float *out, mrefsr_stream_t stream);
int mrefsr_degrade_resize_f32(const float *in, int batch, int c, int h, int w, int oh, int ow, int mode, float scale_h, float scale_w,
                              float *out, mrefsr_stream_t stream);
int mrefsr_degrade_noise_f32(const float *img, const float *noise, const float *noise_gray, const float *param, const float *gray,
                             const float *vals, int batch, int h, int w, int mode, float *out, mrefsr_stream_t stream);
int64_t mrefsr_degrade_levels_workspace_words(int batch);
int mrefsr_degrade_levels_f32(const float *img, int batch, int h, int w, uint32_t *sets, float *vals, mrefsr_stream_t stream);
int mrefsr_degrade_jpeg_f32(const float *img, const float *quality, int batch, int h, int w, float *out, mrefsr_stream_t stream);

/* ---- Frequency-domain losses of the training step (csrc/freq_loss.hip; losses.FFTLoss, losses.FocalFrequencyLoss, train.freq_opt;
 * DESIGN 3.18).  No reference counterpart.  pred, target [planes][h][w] contiguous fp32 (planes = batch x channels), X = pred -
 * target; D = the 2-D DFT of every plane of X, computed densely on the f32 MFMA for the wh = w/2 + 1 non-redundant columns, the
 * others counted through the multiplicity mult (1 for column 0 and for column w/2 with w even, 2 otherwise).  1 <= h, w <= 1024,
 * planes <= 65535, planes h w <= 2^30.  tab_h / tab_w: the twiddle tables [h][2] / [w][2] in device memory, tab_n[r] = (cos, sin)
 * (2 pi r / n) as the fp32 rounding of the float64 values (both may be one table when h = w).
 *
 * mrefsr_freq_loss_blocks: planes ceil(h / 32) ceil(wh / 32), the blocks of the column pass; `partial` holds TWICE as many floats.
 *   -1 for a shape outside the limits.
 * mrefsr_freq_loss_fwd_f32: t: scratch of planes h wh 2 floats (the row pass T = X F_W).
 *   focal = 0 (FFTLoss): loss[0] = fl32(loss_weight s sum mult (|Re D| + |Im D|) / (2 planes h w)), s = 1 (ortho = 0, the
 *     unnormalised transform) or 1 / sqrt(h w) (ortho = 1); with write_g the map g [planes][h][wh][2] = sign(D) mult s /
 *     (2 planes h w) (sign(0) = 0); g may be NULL without write_g.  Two launches.
 *   focal = 1 (FocalFrequencyLoss, the ortho transform; `ortho` is not read): m = |D|^2, w = sqrt(m)^alpha over its maximum in the
 *     plane, NaN -> 0, clamped to [0, 1]; loss[0] = fl32(loss_weight sum mult w m / (planes h w)).  g is always needed (it holds D
 *     between the launches); with write_g it leaves as 2 w D mult / (planes h w sqrt(h w)).  alpha finite, >= 0.  Three launches.
 *   The imaginary part of a self-conjugate bin (ky in {0, h/2}, kx in {0, w/2}) counts as exactly 0.  Sums: fixed order inside a
 *   block, one partial per block, the partials in ascending block order in double by the block that draws the last `ticket` (one
 *   zeroed word; left zero): no float atomics, the same bits from call to call.  pred and target are only read.
 * mrefsr_freq_loss_bwd_f32: grad_pred [planes][h][w], every element written once: loss_weight grad_loss[0] Re(F_H^H g F_W^H) over
 *   the wh stored columns.  grad_loss: the upstream gradient, one float in device memory.  u: scratch of planes h wh 2 floats.
 *   Two launches. */
int mrefsr_freq_loss_blocks(int planes, int h, int w);
int mrefsr_freq_loss_fwd_f32(const float *pred, const float *target, int planes, int h, int w, int focal, int ortho, float alpha,
                             float loss_weight, const float *tab_h, const float *tab_w, float *t, float *g, int write_g, float *partial,
                             uint32_t *ticket, float *loss, mrefsr_stream_t stream);
int mrefsr_freq_loss_bwd_f32(const float *g, const float *grad_loss, int planes, int h, int w, float loss_weight, const float *tab_h,
                             const float *tab_w, float *u, float *grad_pred, mrefsr_stream_t stream);

/* ---- Contextual loss of the training step (csrc/contextual.hip; losses.ContextualLoss, train.contextual_opt; Mechrez
 * et al., ECCV 2018).  No reference counterpart.  One tap: x (features of the output) and y (of the target), NHWC [B][N][C]
 * contiguous fp32, N = h w; i runs over positions of x, j over positions of y.  1 <= B <= 65535, 2 <= N <= MREFSR_CX_MAX_N (one N x N
 * fp32 matrix per sample is materialised in the workspace), C of 64, 128, 256, 512.
 *   mu[b][c] = mean_p y[b][p][c];  xn = (x - mu) / max(|x - mu|_2, 1e-12) per position, yn the same from y;
 *   d[i][j] = 1 - <xn_i, yn_j> (v_mfma_f32_16x16x4_f32);  m[i] = min_j d[i][j] at jmin[i] (the lowest j on ties);
 *   w = exp((1 - d / (m + 1e-5)) / band_width), Z[i] = sum_j w[i][j];
 *   cxmax[j] = max_i w[i][j] / Z[i] at imax[j] (the lowest i on ties);
 *   cx[b] = mean_j cxmax[b][j];  tap_loss[0] = mean_b -log(cx[b] + 1e-5).
 * mrefsr_contextual_workspace_bytes: bytes of `workspace` for the forward (backward = 0) or the backward call; MREFSR_E_INVALID /
 *   MREFSR_E_UNSUPPORTED for a shape outside the limits (N over the bound: MREFSR_E_UNSUPPORTED).
 * mrefsr_contextual_fwd_f32: writes xn, yn [B][N][C], rnorm [B][N] (1 / max(|x - mu|, 1e-12)), rowf [2][B][N] = m, Z,
 *   jmin [B][N], cxmax [B][N], imax [B][N], cx [B], tap_loss [1] -- what the backward call reads -- and the running
 *   total of a loss over several taps: run[0] = (first ? 0 : run[0]) + tap_loss weight, total[0] = run[0] loss_weight.  x and y are
 *   only read.  Six launches; every sum in a fixed order (no float atomics), the same bits from call to call.
 * mrefsr_contextual_bwd_f32: dx [B][N][C] = (accumulate ? dx : 0) + d (gup[0] coef tap_loss) / d x, from the forward's outputs (d is
 *   recomputed); gup: one float in device memory or NULL (= 1); amax (may be NULL): a zeroed word raised to max |dx|.  The gradient
 *   passes through the selected element of each column, the row normaliser Z, the row minimum at jmin, the normalisation and the
 *   centring (mu is a constant of y).  Four launches, fixed orders.
 * A shape outside the limits is refused before any launch. */
#define MREFSR_CX_MAX_N 4096
int64_t mrefsr_contextual_workspace_bytes(int B, int N, int C, int backward);
int mrefsr_contextual_fwd_f32(const float *x, const float *y, int B, int N, int C, float band_width, float *xn, float *yn, float *rnorm,
                              float *rowf, int32_t *jmin, float *cxmax, int32_t *imax, float *cx, float *tap_loss, float weight,
                              float loss_weight, int first, float *run, float *total, void *workspace, int64_t workspace_bytes,
                              mrefsr_stream_t stream);
int mrefsr_contextual_bwd_f32(const float *xn, const float *yn, const float *rnorm, int B, int N, int C, float band_width,
                              const float *rowf, const int32_t *jmin, const float *cxmax, const int32_t *imax, const float *cx,
                              const float *gup, float coef, float *dx, int accumulate, float *amax, void *workspace,
                              int64_t workspace_bytes, mrefsr_stream_t stream);

/* ---- CoBi, the contextual bilateral loss (Zhang et al., "Zoom to Learn, Learn to Zoom", ICCV 2019; csrc/contextual.hip).
 * mrefsr_contextual_fwd_sp_f32 / mrefsr_contextual_bwd_sp_f32: the two calls above on a tap whose N = h w positions lie on an h x w
 *   grid (i = r_i w + c_i), with a spatial term in the distance:
 *     d[i][j] = (1 - weight_sp) (1 - <xn_i, yn_j>) + weight_sp ((r_i - r_j)^2 + (c_i - c_j)^2) / (h^2 + w^2)
 *   (raw distances are mixed, then made relative; the squared offset is an integer, divided once in fp32).  Every later statistic runs
 *   on this d.  With weight_sp > 0 the position norms and the product are taken in double (v_mfma_f64_16x16x4_f64; xn, yn and d each
 *   rounded to fp32 once): the term leaves row minima of 1e-3 and less on repetitive texture, where fp32 norms and an fp32
 *   accumulator near 1 cost the loss a digit.  The term is a constant: the backward is that of the plain call on the combined d, times (1 - weight_sp).  Arguments,
 *   outputs, workspace (mrefsr_contextual_workspace_bytes(B, h w, C, .)), launch counts and checks are those of the plain calls, plus:
 *   h, w >= 1 (else MREFSR_E_INVALID), h w <= MREFSR_CX_MAX_N (else MREFSR_E_UNSUPPORTED), weight_sp a number in [0, 1) (else
 *   MREFSR_E_INVALID).  weight_sp = 0 launches the kernels of the plain calls: the same bits.
 * mrefsr_cx_patch_channels: the channel count Cpad of size x size RGB patches as features, the smallest of 64, 128, 256, 512 that is
 *   >= 3 size^2; MREFSR_E_INVALID for size < 1, MREFSR_E_UNSUPPORTED for size > 13.
 * mrefsr_cx_patches_f32: img NCHW [B][3][H][W] -> out NHWC [B][oh ow][Cpad], oh = (H - size) / stride + 1, ow likewise: channel
 *   (c size + dy) size + dx of patch (pr, pc) is img[b][c][pr stride + dy][pc stride + dx] (F.unfold's order; norm != 0: (v + 1) * 0.5
 *   first), the channels from 3 size^2 on are zeros.  One launch.
 * mrefsr_cx_patches_bwd_f32: its adjoint, dimg [B][3][H][W] = (accumulate ? dimg : 0) + scale * the sum of the at most
 *   ceil(size / stride)^2 entries of g [B][oh ow][Cpad] that cover the pixel, added in ascending (patch row, patch column) order in
 *   fp32 (gather form: no atomics); a pixel no patch covers gets scale * 0.  One launch.
 * mrefsr_cx_subsample_f32: f NHWC [B][h][w][C] (C a multiple of 4) -> out [B][hs][ws][C], hs = ceil(h / s), ws = ceil(w / s), the
 *   positions (r s, c s).  One launch.
 * mrefsr_cx_subsample_bwd_f32: its adjoint into the tap's gradient buffer g [B][h][w][C]: accumulate = 0 writes gs at the sampled
 *   positions and zeros elsewhere; accumulate != 0 adds gs at the sampled positions only.  amax (may be NULL): a zeroed word raised to
 *   max |g| over the whole buffer.  One launch. */
int mrefsr_contextual_fwd_sp_f32(const float *x, const float *y, int B, int h, int w, int C, float band_width, float weight_sp, float *xn,
                                 float *yn, float *rnorm, float *rowf, int32_t *jmin, float *cxmax, int32_t *imax, float *cx,
                                 float *tap_loss, float weight, float loss_weight, int first, float *run, float *total, void *workspace,
                                 int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_contextual_bwd_sp_f32(const float *xn, const float *yn, const float *rnorm, int B, int h, int w, int C, float band_width,
                                 float weight_sp, const float *rowf, const int32_t *jmin, const float *cxmax, const int32_t *imax,
                                 const float *cx, const float *gup, float coef, float *dx, int accumulate, float *amax, void *workspace,
                                 int64_t workspace_bytes, mrefsr_stream_t stream);
int mrefsr_cx_patch_channels(int size);
int mrefsr_cx_patches_f32(const float *img, int B, int H, int W, int size, int stride, int norm, float *out, int Cpad,
                          mrefsr_stream_t stream);
int mrefsr_cx_patches_bwd_f32(const float *g, int B, int H, int W, int size, int stride, int Cpad, float scale, float *dimg, int accumulate,
                              mrefsr_stream_t stream);
int mrefsr_cx_subsample_f32(const float *f, int B, int h, int w, int C, int s, float *out, mrefsr_stream_t stream);
int mrefsr_cx_subsample_bwd_f32(const float *gs, int B, int h, int w, int C, int s, float *g, int accumulate, float *amax,
                                mrefsr_stream_t stream);

/* Fingerprints of n device tensors of 32-bit words: table[2t] = address, table[2t+1] = word count (device memory);
 * sums[t] = sum_i word_i * (2 i + 1) mod 2^64 (exact integer arithmetic: independent of the summation order); `done` is n words
 * of scratch.  With `ref` given, `*flag |= flag_bits` (device memory) where sums[t] != ref[t].  No reference counterpart: the host
 * side keeps packed copies of the convolution weights and uses this to notice parameters edited behind autograd's back
 * (`.data` writes); one launch per forward pass. */
int mrefsr_weights_checksum(const int64_t *table, int n, uint64_t *sums, uint32_t *done, const uint64_t *ref, int *flag, int flag_bits,
                            mrefsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MREFSR_HIP_H */
