"""CPU: the identity behind csrc/mrattn_conv.hip -- the softmax blend of the references commutes with conv_ass -- in float64 against
the reference formulation (ref_mrapa_restoration_arch.py:321-335), and the argument checks of the two entry points."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

P = ctypes.c_void_p(8)   # a non-null pointer: every call below is refused before it could be read


def reference_form(refs, prob, weight, bias):
    """conv_ass on every reference, then the weighted sum: refs [t,n,c,h,w], prob [n,t,h,w] -> [n,2c,h,w]"""
    t, n = refs.shape[:2]
    ass = F.conv2d(refs.flatten(0, 1), weight, bias, padding=1).view(t, n, -1, *refs.shape[-2:])
    return (prob.permute(1, 0, 2, 3)[:, :, None] * ass).sum(0)


def blend_first_form(refs, prob, weight, bias):
    """r(x) = sum_d W_d u_d(x) + b sum_t p_t(x), u_d(x) = sum_t p_t(x) s_t(x + d): the blend needs the tap's shifted map, so it is
    formed per tap on the zero-padded maps"""
    t, n, c, h, w = refs.shape
    pad = F.pad(refs, (1, 1, 1, 1))
    out = torch.zeros(n, weight.shape[0], h, w, dtype=refs.dtype)
    for dy in range(3):
        for dx in range(3):
            u = (prob.permute(1, 0, 2, 3)[:, :, None] * pad[..., dy:dy + h, dx:dx + w]).sum(0)
            out += torch.einsum('oc,nchw->nohw', weight[:, :, dy, dx], u)
    return out + bias[None, :, None, None] * prob.sum(1, keepdim=True)


def masked_softmax(logit, present):
    on = present[:, :, None, None].expand_as(logit)
    p = torch.softmax(logit.masked_fill(~on, float('-inf')), dim=1)
    return torch.where(on, p, torch.zeros_like(p)).nan_to_num(0.0)   # (a sample without a present reference: all zeros)


def test_blend_commutes_with_conv_ass_float64():
    g = torch.Generator().manual_seed(0)
    n, t, c, h, w = 3, 5, 6, 12, 20
    refs = torch.randn(t, n, c, h, w, generator=g, dtype=torch.float64)
    weight = torch.randn(2 * c, c, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(2 * c, generator=g, dtype=torch.float64)
    logit = torch.randn(n, t, h, w, generator=g, dtype=torch.float64)
    # sample 0: every reference; sample 1: one masked; sample 2: none
    present = torch.tensor([[1, 1, 1, 1, 1], [1, 0, 1, 1, 1], [0, 0, 0, 0, 0]], dtype=torch.bool)
    prob = masked_softmax(logit, present)
    assert torch.equal(prob[1, 1], torch.zeros(h, w, dtype=torch.float64)) and not prob[2].any()
    want, got = reference_form(refs, prob, weight, bias), blend_first_form(refs, prob, weight, bias)
    assert float(want.abs().max()) > 1
    torch.testing.assert_close(got, want, rtol=0, atol=1e-12)   # borders included: both sides see the same zero padding
    # the bias is weighted by sum_t p_t: a sample without a reference gives exact zeros, in both forms
    assert not got[2].any() and not want[2].any()
    # an absent map's values reach nothing
    refs2 = refs.clone()
    refs2[1, 1] = 1e30
    assert torch.equal(blend_first_form(refs2, prob, weight, bias), got)


def test_border_counts_of_the_blended_form():
    """all-ones maps and weights, uniform weights, no bias: c * {4, 6, 9} by corner / edge / interior"""
    n, t, c, h, w = 1, 4, 3, 5, 7
    out = blend_first_form(torch.ones(t, n, c, h, w, dtype=torch.float64), torch.full((n, t, h, w), 0.25, dtype=torch.float64),
                           torch.ones(2 * c, c, 3, 3, dtype=torch.float64), torch.zeros(2 * c, dtype=torch.float64))
    assert out[0, 0, 0, 0] == 4 * c and out[0, 0, 0, 3] == 6 * c and out[0, 0, 2, 3] == 9 * c and out[0, 1, h - 1, w - 1] == 4 * c


def test_entry_points_validate_their_arguments_without_gpu():
    from mrefsr_amd import _lib
    lib = _lib.load()
    f = ctypes.c_float
    # (arguments, indices of the pointers that must not be null, index of T, index of c)
    calls = {
        'mrefsr_mrattn_prob_nhwc_f32': ([P, P, None, P, 2, 3, 64, 35, f(0.125), None], (0, 1, 3), 5, 6),
        'mrefsr_mrattn_blend_conv_f32': ([P, P, P, None, None, None, None, P, 2, 3, 5, 7, 64, f(8192.0), None], (0, 1, 2, 7), 9, 12),
    }
    for name, (args, ptrs, t, c) in calls.items():
        fn = getattr(lib, name)
        for i in ptrs:
            bad = list(args)
            bad[i] = None
            assert fn(*bad) != 0 and b'null pointer' in lib.mrefsr_last_error(), (name, i)
        bad = list(args)
        bad[t] = 17
        assert fn(*bad) != 0 and b'T=17' in lib.mrefsr_last_error(), name
        bad = list(args)
        bad[t] = 0
        assert fn(*bad) != 0, name
        for width in (96, 32, 512):
            bad = list(args)
            bad[c] = width
            assert fn(*bad) != 0 and f'c={width}'.encode() in lib.mrefsr_last_error(), (name, width)
    bad = list(calls['mrefsr_mrattn_blend_conv_f32'][0])
    bad[13] = f(0.0)
    assert lib.mrefsr_mrattn_blend_conv_f32(*bad) != 0 and b'wscale' in lib.mrefsr_last_error()
    with pytest.raises(_lib.MrefsrHipError):
        _lib.call('mrefsr_mrattn_prob_nhwc_f32', P, None, None, P, 2, 3, 64, 35, f(1.0), None)


def test_wrappers_refuse_cpu_tensors_and_the_dispatch_keeps_training_and_bf16_on_the_parent_path():
    from mrefsr_amd import hip
    from mrefsr_amd.archs import nhwc
    from mrefsr_amd.archs.ref_mrapa_restoration_arch import MRAPAFusion
    q, emb = torch.zeros(2, 5, 7, 64), torch.zeros(6, 5, 7, 64)
    with pytest.raises(NotImplementedError):
        hip.mrattn_prob_nhwc(q, emb, 3)
    with pytest.raises(NotImplementedError):
        hip.mrattn_blend_conv(emb, torch.zeros(2, 5, 7, 3), hip.PackedWeight(torch.zeros(8, dtype=torch.uint8), 1.0, 16), None, 3)
    m = MRAPAFusion(nf=64, ref_nf=64)
    refs = torch.zeros(15, 4, 4, 64)
    assert MRAPAFusion.BLEND_FIRST and m.blend_first(True, refs, 5)
    assert not m.blend_first(False, refs, 5)             # a recorded graph / bf16 arithmetic or storage: `fold` is off
    assert not m.blend_first(True, refs, 17)
    assert not m.blend_first(True, torch.zeros(15, 4, 4, 96), 5)
    assert not m.blend_first(True, refs.bfloat16(), 5)
    with hip.range_free():                                # the re-run of a batch that left the fp16 range
        assert not m.blend_first(True, refs, 5)
    m.BLEND_FIRST = False                                 # instance or class attribute: tests flip it
    assert not m.blend_first(True, refs, 5)
    assert nhwc.TERMS == 16
