"""CPU: the identity behind MRAPAFusion.FOLD_ADD2 -- feat_fusion (1x1, linear) composed with spatial_attn_add2 (3x3, nothing
non-linear between them) is one 3x3 convolution 2C -> nf -- in float64 against MRAPAFusion._fuse itself (its attention kernel
replaced by a torch restatement: the module has no CPU kernels), the gating predicate, and the argument checks of the compose
entry point."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

P = ctypes.c_void_p(8)   # a non-null pointer: every call below is refused before it could be read


def attention64(q, emb, ass, t, want_prob=True, t_major=False):
    """hip.mrattn_fwd in torch: softmax_t(<q, emb_t>) . ass_t per pixel (ref :321-335), (out, prob [n,t,h,w])"""
    n = q.shape[0]
    split = (lambda x: x.view(t, n, *x.shape[1:])) if t_major else (lambda x: x.view(n, t, *x.shape[1:]).transpose(0, 1))
    p = torch.softmax((q[None] * split(emb)).sum(2), dim=0)
    return (p[:, :, None] * split(ass)).sum(0), p.permute(1, 0, 2, 3)


def folded_form(m, target, refs, t):
    """_fuse (refs stacked t-major) with add2 folded into feat_fusion: W' = Wf_r o W2, b' = b_f + Wf_r b2, the composed convolution
    of a1 added in front of the activation"""
    lrelu = lambda x: F.leaky_relu(x, 0.1)
    h, w = target.shape[-2:]
    target, refs = m.spatial_padding(target), m.spatial_padding(refs)
    r, _ = attention64(m.conv_emb1(target) * m.scale, m.conv_emb2(refs), m.conv_ass(refs), t, t_major=True)
    attn = lrelu(m.spatial_attn(torch.cat([target, r], dim=1)))
    mul = m.spatial_attn_mul2(lrelu(m.spatial_attn_mul1(attn)))
    a1 = lrelu(m.spatial_attn_add1(attn))
    ff, add2, nf = m.feat_fusion, m.spatial_attn_add2, target.shape[1]
    wf_r = ff.weight[:, nf:, 0, 0]
    w_fold = torch.einsum('om,mikl->oikl', wf_r, add2.weight)
    b_fold = torch.zeros(ff.out_channels, dtype=target.dtype) if ff.bias is None else ff.bias
    if add2.bias is not None:
        b_fold = b_fold + wf_r @ add2.bias
    pre = F.conv2d(a1, w_fold, None, padding=1)
    feat = lrelu(F.conv2d(torch.cat([target, r * torch.sigmoid(mul) * 2], dim=1), ff.weight, b_fold) + pre)
    return feat[:, :, :h, :w]


@pytest.mark.parametrize('absent', [None, 'spatial_attn_add2', 'feat_fusion'])
@pytest.mark.parametrize('h,w', [(4, 4), (12, 20), (10, 14)])   # 10 x 14: reflect pad and crop
@pytest.mark.parametrize('c', [64, 128, 256])
def test_folded_form_equals_fuse_float64(monkeypatch, c, h, w, absent):
    from mrefsr_amd import hip
    from mrefsr_amd.archs.ref_mrapa_restoration_arch import MRAPAFusion
    monkeypatch.setattr(hip, 'mrattn_fwd', attention64)
    torch.manual_seed(c + h)
    n, t = 1, 2
    m = MRAPAFusion(nf=64, ref_nf=c).double()
    with torch.no_grad():
        for conv in (m.spatial_attn_add2, m.feat_fusion):
            conv.bias.normal_()   # (biases of order 1: an absent or misplaced one shows)
    if absent is not None:
        getattr(m, absent).bias = None
    target = torch.randn(n, 64, h, w, dtype=torch.float64)
    refs = torch.randn(t * n, c, h, w, dtype=torch.float64)
    want = m.forward_stacked(target, refs, t).detach()
    got = folded_form(m, target, refs, t).detach()
    assert want.shape == (n, 64, h, w) and float(want.abs().max()) > 0.1
    err = float((got - want).abs().max() / want.abs().max())
    print(f'c={c} {h}x{w} absent={absent}: max|folded - _fuse| / max|_fuse| = {err:.2e}')
    assert err <= 1e-12


def test_the_fold_is_gated_to_fp32_inference_with_a_matching_feat_fusion():
    from mrefsr_amd.archs import nhwc
    from mrefsr_amd.archs.ref_mrapa_restoration_arch import MRAPAFusion
    m = MRAPAFusion(nf=64, ref_nf=64)
    target = torch.zeros(2, 4, 4, 64)   # channels-last, as forward_nhwc sees it
    assert MRAPAFusion.FOLD_ADD2 and m.fold_add2(False, target)
    assert not m.fold_add2(True, target)                      # a graph is being recorded: training keeps add2
    nhwc.set_arithmetic('bf16')
    try:
        assert not m.fold_add2(False, target)                 # the bf16 arithmetic: its rounding points are fixed
        assert not m.fold_add2(False, target.bfloat16())
    finally:
        nhwc.set_arithmetic('fp32')
    assert not m.fold_add2(False, torch.zeros(2, 4, 4, 32))   # feat_fusion.in_channels != nf + add2.out_channels
    for other in (torch.nn.Conv2d(64 + 128, 64, 3, padding=1), torch.nn.Conv2d(64 + 64, 64, 1), torch.nn.Conv2d(64 + 128, 64, 1, stride=2)):
        m2 = MRAPAFusion(nf=64, ref_nf=64)
        m2.feat_fusion = other
        assert not m2.fold_add2(False, target)
    m2 = MRAPAFusion(nf=64, ref_nf=64)
    m2.spatial_attn_add2 = torch.nn.Conv2d(128, 128, 3, padding=1, padding_mode='reflect')   # not a convolution of the engine
    assert not m2.fold_add2(False, target)
    m.FOLD_ADD2 = False                                       # instance or class attribute: tests flip it
    assert not m.fold_add2(False, target)
    assert MRAPAFusion.FOLD_ADD2 and nhwc.TERMS == 16 and not nhwc.BF16


def test_compose_entry_point_validates_its_arguments_without_gpu():
    from mrefsr_amd import _lib, hip
    lib = _lib.load()
    i64 = ctypes.c_int64
    good = [P, i64(192), 64, P, None, None, P, None, 64, 128, 128, None]   # w1x1, ld, offset, w3x3, b3x3, b1x1, out_w, out_b, Cout, Cmid, Cin
    for i in (0, 3, 6):
        bad = list(good)
        bad[i] = None
        assert lib.mrefsr_conv_compose_1x1_3x3_f32(*bad) != 0 and b'null pointer' in lib.mrefsr_last_error(), i
    for i, v in ((8, 0), (9, 0), (10, -1), (2, -1), (2, 65), (1, i64(100))):   # sizes; columns that leave the 1x1 row
        bad = list(good)
        bad[i] = v
        assert lib.mrefsr_conv_compose_1x1_3x3_f32(*bad) != 0, (i, v)
    with pytest.raises(NotImplementedError):
        hip.conv_compose_1x1_3x3(torch.zeros(8, 40, 1, 1), torch.zeros(24, 20, 3, 3), cin_offset=16)   # CPU tensors
    with pytest.raises(NotImplementedError):
        hip.attn_modulate_(torch.zeros(4, 4), torch.zeros(4, 4), None)
