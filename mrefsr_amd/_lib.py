"""Loader for libmrefsr_hip.so (the C ABI of include/mrefsr_hip.h).  Fails loudly."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MREFSR_HIP_LIB: another build of the same library (A/B measurements of kernel variants)
LIB_PATH = os.environ.get('MREFSR_HIP_LIB') or os.path.join(_HERE, 'lib', 'libmrefsr_hip.so')
ABI_VERSION = 1

_vp, _i, _f, _i64 = C.c_void_p, C.c_int, C.c_float, C.c_int64


class DcnShape(C.Structure):
    """mirror of mrefsr_dcn_shape"""
    _fields_ = [(n, C.c_int) for n in ('B', 'C', 'H', 'W', 'Co', 'kh', 'kw', 'stride_h', 'stride_w', 'pad_h', 'pad_w',
                                       'dil_h', 'dil_w', 'groups', 'dg')]


class ConvDesc(C.Structure):
    """mirror of mrefsr_conv_desc"""
    _fields_ = [(n, C.c_int32) for n in ('N', 'H', 'W', 'ksize', 'C1', 'ld1', 'N1', 'C2', 'ld2', 'N2', 'Cout', 'ld_out', 'ld_res',
                                         'pre_N', 'act', 'epilogue', 'terms')] + [('slope', C.c_float), ('wscale', C.c_float)]


class ConvPackJob(C.Structure):
    """mirror of mrefsr_conv_pack_job"""
    _fields_ = [('weight', C.c_void_p), ('packed', C.c_void_p), ('stride_o', C.c_int64), ('stride_i', C.c_int64), ('Cout', C.c_int32),
                ('Cin', C.c_int32), ('ksize', C.c_int32), ('terms', C.c_int32), ('flip', C.c_int32), ('wscale', C.c_float)]


class TapJob(C.Structure):
    """mirror of mrefsr_tap_job"""
    _fields_ = [('x', C.c_void_p), ('y', C.c_void_p), ('grad', C.c_void_p), ('n', C.c_int64), ('inv_n', C.c_float), ('weight', C.c_float),
                ('group', C.c_int32)]


class TextureLayer(C.Structure):
    """mirror of mrefsr_texture_layer"""
    _fields_ = [('gx', C.c_void_p), ('gm', C.c_void_p), ('n', C.c_int64), ('div', C.c_float)]


class OptimJob(C.Structure):
    """mirror of mrefsr_optim_job"""
    _fields_ = [('p', C.c_void_p), ('g', C.c_void_p), ('m', C.c_void_p), ('v', C.c_void_p), ('ema', C.c_void_p), ('n', C.c_int64),
                ('first_chunk', C.c_int32), ('group', C.c_int32)]


class AdamGroup(C.Structure):
    """mirror of mrefsr_adam_group"""
    _fields_ = [(n, C.c_double) for n in ('lr', 'beta1', 'beta2', 'eps', 'weight_decay')] + [('step', C.c_int64)]


class GradClipState(C.Structure):
    """mirror of mrefsr_grad_clip_state"""
    _fields_ = [(n, C.c_float) for n in ('total_norm', 'coef', 'found_inf', 'reserved')] + [('skipped', C.c_int64)]


# name -> (restype, argtypes): exactly the declarations of include/mrefsr_hip.h
SIGNATURES = {
    'mrefsr_abi_version': (_i, []),
    'mrefsr_last_error': (C.c_char_p, []),
    'mrefsr_corr_padded_channels': (_i, [_i]),
    'mrefsr_pixnorm_f32': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    'mrefsr_patch_norm_f32': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    'mrefsr_corr_top1_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'mrefsr_feature_match_index_workspace_bytes': (_i64, [_i, _i, _i, _i]),
    'mrefsr_feature_match_index_f32': (_i, [_vp, _vp] + [_i] * 10 + [_vp, _vp, _vp, _i64, _vp]),
    'mrefsr_corr_workspace_bytes': (_i64, [_i, _i, _i]),
    'mrefsr_corr_prefilter_info': (_i64, [_i, _i, _i, _i, C.c_char_p, _i, C.POINTER(C.c_int)]),
    'mrefsr_corr_top1_prefilter_f32': (_i, [_vp] * 9 + [_i64, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    'mrefsr_offsets_from_idx_f32': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    'mrefsr_dynagg_prep_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'mrefsr_dynagg_prep_bwd_f32': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'mrefsr_dynagg_prep_bwd_nhwc_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'mrefsr_dynagg_prep_bwd_blocks': (_i, [_i, _i, _i, _i]),
    'mrefsr_dynagg_prep_bwd_det_workspace_bytes': (_i64, [_i, _i, _i, _i]),
    'mrefsr_dynagg_prep_bwd_nhwc_det_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp, _vp]),
    'mrefsr_dcn_fwd_workspace_bytes': (_i64, [C.POINTER(DcnShape)]),
    'mrefsr_dcn_fwd_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(DcnShape), _f, _i, _vp, _i64, _vp, _vp]),
    'mrefsr_dcn_fwd_amax_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(DcnShape), _f, _i, _vp, _i64, _vp, _vp, _vp]),
    'mrefsr_dcn_im2col_f32': (_i, [_vp, _vp, _vp, _vp, C.POINTER(DcnShape), _vp]),
    'mrefsr_dcn_col2im_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(DcnShape), _vp]),
    'mrefsr_dcn_bwd_data_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, C.POINTER(DcnShape), _vp]),
    'mrefsr_dcn_bwd_weight_workspace_bytes': (_i64, [C.POINTER(DcnShape)]),
    'mrefsr_conv_wgrad1x1_workspace_bytes': (_i64, [_i64, _i, _i]),
    'mrefsr_conv_wgrad1x1_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _vp, _vp]),
    'mrefsr_dcn_bwd_weight_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, C.POINTER(DcnShape), _vp, _vp]),
    'mrefsr_mrattn_fwd_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'mrefsr_mrattn_fwd_nhwc_f32': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'mrefsr_mrattn_fwd_nhwc_scaled_f32': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    'mrefsr_mrattn_bwd_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'mrefsr_mrattn_fwd_masked_f32': (_i, [_vp] * 6 + [_i] * 6 + [_vp]),
    'mrefsr_mrattn_bwd_masked_f32': (_i, [_vp] * 9 + [_i] * 6 + [_vp]),
    'mrefsr_mrattn_fwd_nhwc_masked_f32': (_i, [_vp] * 5 + [_i, _i, _i, _i, _f, _vp]),
    'mrefsr_mrattn_fwd_nhwc_masked_bf16': (_i, [_vp] * 5 + [_i, _i, _i, _i, _vp]),
    'mrefsr_mrattn_prob_nhwc_f32': (_i, [_vp] * 4 + [_i, _i, _i, _i, _f, _vp]),
    'mrefsr_mrattn_blend_conv_f32': (_i, [_vp] * 8 + [_i, _i, _i, _i, _i, _f, _vp]),
    'mrefsr_fused_bias_act': (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _f, _f, _i, _vp]),
    'mrefsr_bias_act_res_f32': (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _i, _i64, _f, _vp]),
    'mrefsr_tail_bilinear_add_f32': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'mrefsr_conv_packed_bytes': (_i64, [_i, _i, _i, _i]),
    'mrefsr_conv_pack_weight_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp]),
    'mrefsr_conv_pack_weight_view_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _f, _i64, _i64, _i, _vp]),
    'mrefsr_conv_pack_weights_multi_f32': (_i, [_vp, _i, _vp, _vp]),
    'mrefsr_conv_compose_1x1_3x3_f32': (_i, [_vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    'mrefsr_act_bwd_blocks': (_i, [_i64, _i]),
    'mrefsr_act_bwd_nhwc_f32': (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i64, _i, _i, _f, _vp, _vp, _vp]),
    'mrefsr_act_bwd_det_workspace_bytes': (_i64, [_i64, _i]),
    'mrefsr_act_bwd_nhwc_det_f32': (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i64, _i, _i, _f, _vp, _vp, _vp, _i64, _vp, _vp]),
    'mrefsr_conv_nhwc_scaled_f32': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'mrefsr_conv_nhwc_amax_f32': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'mrefsr_conv_nhwc_bwd_f32': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'mrefsr_conv_nhwc_bwd_det_workspace_bytes': (_i64, [C.POINTER(ConvDesc)]),
    'mrefsr_conv_nhwc_bwd_det_f32': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    'mrefsr_conv_wgrad3x3_workspace_bytes': (_i64, [_i, _i, _i, _i, _i]),
    'mrefsr_conv_wgrad3x3_f32': (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _i64, _i64, _i, _vp, _i, _i, _i, _vp, _i64, _vp, _vp]),
    'mrefsr_conv_wgrad3x3_batch_workspace_bytes': (_i64, [_i, _i, _i, _i, _i, _i]),
    'mrefsr_conv_wgrad3x3_batch_f32': (_i, [_i, _vp, _i, _i, _vp, _i, _i, _vp, _i64, _i64, _i, _vp, _i, _i, _i, _vp, _i64, _vp, _vp]),
    'mrefsr_mrattn_bwd_nhwc_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'mrefsr_mrattn_bwd_nhwc_masked_f32': (_i, [_vp] * 8 + [_i, _i, _i, _i, _vp]),
    'mrefsr_attn_modulate_bwd_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'mrefsr_reflect_pad_nhwc_f32': (_i, [_vp, _vp] + [_i] * 6 + [_vp]),
    'mrefsr_reflect_pad_bwd_nhwc_f32': (_i, [_vp, _vp] + [_i] * 6 + [_vp]),
    'mrefsr_crop_nhwc_f32': (_i, [_vp, _vp, _vp] + [_i] * 6 + [_vp]),
    'mrefsr_crop_bwd_nhwc_f32': (_i, [_vp, _vp] + [_i] * 6 + [_vp]),
    'mrefsr_conv_nhwc_f32': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'mrefsr_dcn_fwd': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(DcnShape), _f, _i, _vp]),
    'mrefsr_dcn_im2col': (_i, [_vp, _vp, _vp, _vp, C.POINTER(DcnShape), _i, _vp]),
    'mrefsr_dcn_col2im': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(DcnShape), _i, _vp]),
    'mrefsr_conv_dynagg_f32': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    'mrefsr_mrattn_fwd_nhwc_bf16': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'mrefsr_attn_modulate_bf16': (_i, [_vp, _vp, _vp, _i64, _vp]),
    'mrefsr_attn_modulate_f32': (_i, [_vp, _vp, _vp, _i64, _vp]),
    'mrefsr_bias_relu_pool2_f32': (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _vp]),
    'mrefsr_image_to_nhwc4_f32': (_i, [_vp, _vp, _i64, _i64, _i, _vp, _vp, _vp]),
    'mrefsr_weights_checksum': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    'mrefsr_maxpool2_nhwc_f32': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'mrefsr_maxpool2_bwd_nhwc_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'mrefsr_tap_crit_blocks': (_i, [_i64]),
    'mrefsr_tap_crit_workspace_bytes': (_i, [C.POINTER(TapJob), _i]),
    'mrefsr_tap_crit_f32': (_i, [C.POINTER(TapJob), _i, _i, _f, _f, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    'mrefsr_gram_splits': (_i, [_i, _i, _i]),
    'mrefsr_gram_workspace_bytes': (_i64, [_i, _i, _i]),
    'mrefsr_gram_nhwc_f32': (_i, [_vp, _i, _i, _i, _vp, _vp, _i64, _vp]),
    'mrefsr_gram_nhwc_scaled_f32': (_i, [_vp, _i, _i, _i, _f, _vp, _vp, _i64, _vp]),
    'mrefsr_gram_bwd_nhwc_f32': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _f, _f, _i, _vp, _vp]),
    'mrefsr_image_to_nhwc4_bwd_f32': (_i, [_vp, _i, _vp, _i64, _i64, _i, _vp, _vp]),
    'mrefsr_disc_pack_image_f32': (_i, [_vp, _vp, _i, _i, _i, _vp]),
    'mrefsr_disc_unpack_image_f32': (_i, [_vp, _vp, _i, _i, _i, _vp]),
    'mrefsr_disc_conv_pack_weight_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    'mrefsr_disc_conv3x3_f32': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'mrefsr_disc_conv3x3_dgrad_f32': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'mrefsr_disc_conv3x3_wgrad_workspace_bytes': (_i64, [_i, _i, _i, _i, _i, _i]),
    'mrefsr_disc_conv3x3_wgrad_f32': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp]),
    'mrefsr_disc_chan_workspace_bytes': (_i64, [_i64, _i]),
    'mrefsr_disc_bias_grad_f32': (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp]),
    'mrefsr_disc_bn_lrelu_f32': (_i, [_vp] * 9 + [_i64, _i, _f, _f, _f, _vp, _i64, _vp]),
    'mrefsr_disc_bn_lrelu_bwd_f32': (_i, [_vp] * 9 + [_i64, _i, _f, _vp, _i64, _vp]),
    'mrefsr_disc_bn_lrelu_dbl_f32': (_i, [_vp] * 12 + [_i64, _i, _f, _vp, _i64, _vp]),
    'mrefsr_disc_head_workspace_bytes': (_i64, [_i, _i, _i]),
    'mrefsr_disc_head_fwd_f32': (_i, [_vp] * 8 + [_i, _i, _i, _i, _f, _vp]),
    'mrefsr_disc_head_bwd_f32': (_i, [_vp] * 11 + [_i, _i, _i, _i, _f, _vp, _i64, _vp]),
    'mrefsr_disc_head_dbl_f32': (_i, [_vp] * 13 + [_i, _i, _i, _i, _f, _vp, _i64, _vp]),
    'mrefsr_disc_vconv_pack_weight_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'mrefsr_disc_vconv_workspace_bytes': (_i64, [_i] * 7),
    'mrefsr_disc_vconv_f32': (_i, [_vp] * 4 + [_i] * 7 + [_f, _vp, _i64, _vp]),
    'mrefsr_disc_vconv_dgrad_f32': (_i, [_vp] * 3 + [_i] * 6 + [_vp, _i64, _vp]),
    'mrefsr_disc_vconv_wgrad_workspace_bytes': (_i64, [_i] * 6),
    'mrefsr_disc_vconv_wgrad_f32': (_i, [_vp] * 3 + [_i] * 7 + [_vp, _i64, _vp]),
    'mrefsr_disc_lrelu_mask_f32': (_i, [_vp, _vp, _vp, _i64, _f, _vp]),
    'mrefsr_disc_linear_head_fwd_f32': (_i, [_vp] * 7 + [_i, _i, _i, _i, _f, _vp]),
    'mrefsr_disc_linear_head_bwd_f32': (_i, [_vp] * 10 + [_i, _i, _i, _i, _f, _vp]),
    'mrefsr_disc_linear_head_workspace_bytes': (_i64, [_i, _i]),
    'mrefsr_disc_linear_head_dbl_f32': (_i, [_vp] * 8 + [_i, _i, _i, _i, _f, _vp, _i64, _vp]),
    'mrefsr_disc_sn_workspace_bytes': (_i64, [_vp, _vp, _i]),
    'mrefsr_disc_sn_power_f32': (_i, [_vp] * 5 + [_i, _i, _f] + [_vp] * 4 + [_i64, _vp]),
    'mrefsr_disc_sn_scale_f32': (_i, [_vp] * 4 + [_i, _vp, _vp]),
    'mrefsr_disc_sn_bwd_workspace_bytes': (_i64, [_vp, _vp, _i]),
    'mrefsr_disc_sn_bwd_f32': (_i, [_vp] * 5 + [_i] + [_vp] * 4 + [_i64, _vp]),
    'mrefsr_disc_up2_f32': (_i, [_vp] * 3 + [_i] * 4 + [_vp]),
    'mrefsr_disc_up2_adj_f32': (_i, [_vp] * 2 + [_i] * 4 + [_vp]),
    'mrefsr_disc_add_f32': (_i, [_vp] * 3 + [_i64, _vp]),
    'mrefsr_disc_conv9_f32': (_i, [_vp] * 4 + [_i] * 4 + [_vp]),
    'mrefsr_disc_conv9_dgrad_f32': (_i, [_vp] * 3 + [_i] * 4 + [_vp]),
    'mrefsr_disc_conv9_wgrad_workspace_bytes': (_i64, [_i] * 4),
    'mrefsr_disc_conv9_wgrad_f32': (_i, [_vp] * 3 + [_i] * 4 + [_vp, _i64, _vp]),
    'mrefsr_disc_sg2_fir_f32': (_i, [_vp, _vp] + [_i] * 4 + [_vp] + [_i] * 5 + [_vp]),
    'mrefsr_disc_sg2_pack_weight_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'mrefsr_disc_sg2_conv_workspace_bytes': (_i64, [_i] * 7),
    'mrefsr_disc_sg2_conv_f32': (_i, [_vp] * 5 + [_i] * 7 + [_f, _vp, _i64, _vp]),
    'mrefsr_disc_sg2_conv_dgrad_f32': (_i, [_vp] * 3 + [_i] * 6 + [_vp, _i64, _vp]),
    'mrefsr_disc_sg2_conv_wgrad_workspace_bytes': (_i64, [_i] * 6),
    'mrefsr_disc_sg2_conv_wgrad_f32': (_i, [_vp] * 3 + [_i] * 7 + [_vp, _i64, _vp]),
    'mrefsr_upfirdn2d_f32': (_i, [_vp, _vp, _vp] + [_i] * 14 + [_vp]),
    'mrefsr_upfirdn2d': (_i, [_vp, _vp, _vp] + [_i] * 15 + [_vp]),
    'mrefsr_tensor2img_u8': (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    'mrefsr_val_metrics_workspace_bytes': (_i64, [_i, _i, _i]),
    'mrefsr_optim_job_chunks': (_i, [_i64]),
    'mrefsr_ema_multi_f32': (_i, [_vp, _i, _f, _f, _vp]),
    'mrefsr_adam_multi_f32': (_i, [_vp, _i, _vp, _i, _f, _f, _vp]),
    'mrefsr_grad_norm_workspace_bytes': (_i64, []),
    'mrefsr_grad_sqnorm_multi_f32': (_i, [_vp, _i, _vp, _i64, _vp]),
    'mrefsr_grad_norm_finalize_f32': (_i, [_vp, _i64, _f, _i, _vp, _vp]),
    'mrefsr_grad_scale_multi_f32': (_i, [_vp, _i, _vp, _vp]),
    'mrefsr_adam_multi_clip_f32': (_i, [_vp, _i, _vp, _i, _f, _f, _vp, _i, _vp]),
    'mrefsr_val_metrics_f32': (_i, [_vp, _vp] + [_i] * 5 + [_vp, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    'mrefsr_r1_sqnorm_row_blocks': (_i, [_i64]),
    'mrefsr_r1_sqnorm_workspace_bytes': (_i64, [_i, _i64]),
    'mrefsr_r1_sqnorm_f32': (_i, [_vp, _i, _i64, _vp, _vp, _i64, _vp]),
    'mrefsr_r1_sqnorm_bwd_f32': (_i, [_vp, _vp, _i, _i64, _vp, _vp]),
    'mrefsr_dihedral_expand_f32': (_i, [_vp, _vp] + [_i] * 6 + [_vp]),
    'mrefsr_dihedral_merge_f32': (_i, [_vp, _vp, _vp] + [_i] * 4 + [_vp]),
    'mrefsr_color_fix_wavelet_f32': (_i, [_vp, _vp, _vp] + [_i] * 4 + [_vp, _i, _vp]),
    'mrefsr_color_fix_adain_workspace_bytes': (_i64, [_i] * 4),
    'mrefsr_color_fix_adain_f32': (_i, [_vp, _vp, _vp] + [_i] * 4 + [_vp, _vp, _i64, _vp, _vp]),
    'mrefsr_warp_persp_f32': (_i, [_vp, _vp, _vp] + [_i] * 8 + [_vp]),
    'mrefsr_match_stats_f64': (_i, [_vp] * 4 + [_i] * 7 + [_vp]),
    'mrefsr_texture_select_f32': (_i, [_vp] * 6 + [_i, _i, _i64, _vp]),
    'mrefsr_texture_swap_nhwc_f32': (_i, [_vp] * 4 + [_i] * 6 + [_vp]),
    'mrefsr_texture_coeff_f32': (_i, [_vp] * 4 + [_i, _i, _i, _vp]),
    'mrefsr_texture_scale_nhwc_f32': (_i, [_vp, _vp, _vp, _i64, _i, _vp]),
    'mrefsr_texture_crit_f32': (_i, [C.POINTER(TextureLayer), _i, _f, _vp, _vp, _vp, _vp, _vp]),
    'mrefsr_texture_gram_bwd_nhwc_f32': (_i, [_vp] * 7 + [_i, _i, _i, _f, _i, _vp, _vp]),
    'mrefsr_ref_select_workspace_bytes': (_i64, [_i, _i, _i64]),
    'mrefsr_ref_select_f32': (_i, [_vp] * 5 + [_i, _i, _i64, _i, _i, _vp, _i64, _vp]),
    'mrefsr_ref_gather': (_i, [_vp, _vp, _vp, _i, _i, _i, _i64, _vp]),
    'mrefsr_ssim_loss_blocks': (_i, [_i, _i, _i, _i]),
    'mrefsr_ssim_loss_fwd_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _f] + [_vp] * 7),
    'mrefsr_ssim_loss_bwd_f32': (_i, [_vp] * 6 + [_i, _i, _i, _i, _f, _vp, _vp]),
    'mrefsr_msssim_pyramid_floats': (_i64, [_i] * 5),
    'mrefsr_msssim_map_floats': (_i64, [_i] * 5),
    'mrefsr_msssim_workspace_bytes': (_i64, [_i] * 6),
    'mrefsr_msssim_loss_fwd_f32': (_i, [_vp, _vp] + [_i] * 5 + [C.POINTER(C.c_double), _f] + [_vp] * 5 + [_i64, _vp, _vp]),
    'mrefsr_msssim_loss_bwd_f32': (_i, [_vp] * 4 + [_i] * 5 + [_f, _vp, _i64, _vp, _vp]),
    'mrefsr_ldl_loss_blocks': (_i, [_i, _i, _i]),
    'mrefsr_ldl_loss_fwd_f32': (_i, [_vp, _vp, _vp, _i, _i, _i, _f] + [_vp] * 8),
    'mrefsr_ldl_loss_bwd_f32': (_i, [_vp] * 7 + [_i, _i, _i, _f, _vp, _vp]),
    'mrefsr_ldl_loss_map_f32': (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    'mrefsr_freq_loss_blocks': (_i, [_i, _i, _i]),
    'mrefsr_freq_loss_fwd_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    'mrefsr_freq_loss_bwd_f32': (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    'mrefsr_contextual_workspace_bytes': (_i64, [_i, _i, _i, _i]),
    'mrefsr_contextual_fwd_f32': (_i, [_vp, _vp, _i, _i, _i, _f] + [_vp] * 9 + [_f, _f, _i, _vp, _vp, _vp, _i64, _vp]),
    'mrefsr_contextual_bwd_f32': (_i, [_vp, _vp, _vp, _i, _i, _i, _f] + [_vp] * 6 + [_f, _vp, _i, _vp, _vp, _i64, _vp]),
    'mrefsr_contextual_fwd_sp_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f] + [_vp] * 9 + [_f, _f, _i, _vp, _vp, _vp, _i64, _vp]),
    'mrefsr_contextual_bwd_sp_f32': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _f] + [_vp] * 6 + [_f, _vp, _i, _vp, _vp, _i64, _vp]),
    'mrefsr_cx_patch_channels': (_i, [_i]),
    'mrefsr_cx_patches_f32': (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    'mrefsr_cx_patches_bwd_f32': (_i, [_vp, _i, _i, _i, _i, _i, _i, _f, _vp, _i, _vp]),
    'mrefsr_cx_subsample_f32': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    'mrefsr_cx_subsample_bwd_f32': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp]),
    'mrefsr_degrade_filter2d_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    'mrefsr_degrade_usm_f32': (_i, [_vp, C.POINTER(C.c_float), _i, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp]),
    'mrefsr_degrade_resize_f32': (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _f, _f, _vp, _vp]),
    'mrefsr_degrade_noise_f32': (_i, [_vp] * 6 + [_i, _i, _i, _i, _vp, _vp]),
    'mrefsr_degrade_levels_workspace_words': (_i64, [_i]),
    'mrefsr_degrade_levels_f32': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    'mrefsr_degrade_jpeg_f32': (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    'mrefsr_disc_augment_workspace_bytes': (_i64, [_i, _i, _i]),
    'mrefsr_disc_augment_f32': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _vp]),
    'mrefsr_disc_augment_adj_f32': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _vp]),
}

_lib = None


class MrefsrHipError(RuntimeError):
    pass


def load():
    """dlopen the library and bind every symbol of the header.  Needs no GPU."""
    global _lib
    if _lib is not None:
        return _lib
    if os.environ.get('BASICSR_JIT') == 'True' and not os.environ.get('MREFSR_HIP_LIB'):
        # the reference's run-time build (basicsr/ops/dcn/deform_conv.py:10-21, fused_act.py:9-19, upfirdn2d.py:9-19:
        # torch.utils.cpp_extension.load of the CUDA sources at import), retargeted at hipcc: the library's own Makefile, incremental
        # (nothing to do when the sources are older than the .so), before the first dlopen.  BASICSR_EXT=True at `setup.py develop`
        # time (setup.py:118-136) corresponds to `make -C mrefsr_amd/csrc` / __graft_entry__.build() done once.
        import shutil
        import subprocess
        if shutil.which('hipcc') is None:
            raise MrefsrHipError('BASICSR_JIT=True asks for a run-time build of libmrefsr_hip.so, but hipcc is not on PATH')
        # one builder at a time: under torchrun / DDP every rank imports at once, and concurrent makes in the same _obj/ and lib/
        # would leave a rank dlopen-ing a half-written library (the reference's cpp_extension.load serialises with a file baton)
        import fcntl
        with open(os.path.join(_HERE, 'csrc', '.build.lock'), 'w') as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                subprocess.check_call(['make', '-C', os.path.join(_HERE, 'csrc'), '-s'])
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
    if not os.path.exists(LIB_PATH):
        raise MrefsrHipError(
            f'{LIB_PATH} is not built. Build it with `make -C mrefsr_amd/csrc` (or '
            '`python -c "import __graft_entry__ as g; g.build()"`). There is no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header / library mismatch
        fn.restype, fn.argtypes = res, args
    got = lib.mrefsr_abi_version()
    if got != ABI_VERSION:
        raise MrefsrHipError(f'libmrefsr_hip.so ABI {got} != expected {ABI_VERSION}: rebuild')
    _lib = lib
    return lib


_TRACE = os.environ.get('MREFSR_TRACE_CALLS', '0') == '1'   # debugging: name every entry point on stderr before it runs (with
                                                            # AMD_SERIALIZE_KERNEL=3 the last name printed is the faulting launch)


def call(name, *args):
    lib = load()
    if _TRACE:
        import sys

        def show(a):
            o = getattr(a, '_obj', None)
            if isinstance(o, C.Structure):
                return '{' + ' '.join(f'{f}={getattr(o, f)}' for f, _ in o._fields_) + '}'
            return hex(a.value or 0) if isinstance(a, C.c_void_p) else str(getattr(a, 'value', a))
        print('[mrefsr]', name, ' '.join(show(a) for a in args), file=sys.stderr, flush=True)
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise MrefsrHipError(f'{name} failed ({rc}): {lib.mrefsr_last_error().decode()}')
