"""GPU: the attention head with the blend of the references moved in front of conv_ass (csrc/mrattn_conv.hip, the softmax-weights
entry of csrc/mrattn.hip) against a float64 restatement of ref_mrapa_restoration_arch.py:321-335 -- conv_ass on every reference,
then the softmax-weighted sum.  Bar of the fp32-equivalent forward kernels: rtol = atol = 1e-4 (test_dcn_forward_vs_oracle)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BAR = dict(rtol=1e-4, atol=1e-4)
MAPS = ((4, 4), (12, 20), (36, 44))   # smaller than a tile; ragged both ways; across tile boundaries (tiles are 8 x 32)


@pytest.fixture(scope='module')
def hip():
    from mrefsr_amd import hip as h
    return h


def gen(seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return g


def operands(c, t, n, h, w, seed):
    """refs [t*n,h,w,c] t-major, q, emb, conv_ass weight (outputs of order 1) and bias"""
    g = gen(seed)
    r = lambda *s: torch.randn(*s, device='cuda', generator=g)
    return r(t * n, h, w, c), r(n, h, w, c), r(t * n, h, w, c), r(2 * c, c, 3, 3) / (9 * c) ** 0.5, r(2 * c)


def want64(refs, prob, weight, bias, t, present=None):
    """the reference formulation in float64: ass_t = conv_ass(s_t); r = sum_t p_t ass_t over the present t"""
    n = prob.shape[0]
    ass = F.conv2d(refs.double().permute(0, 3, 1, 2), weight.double(), None if bias is None else bias.double(), padding=1)
    ass = ass.permute(0, 2, 3, 1).reshape(t, n, *ass.shape[2:], ass.shape[1])
    out = torch.zeros_like(ass[0])
    for k in range(t):
        for i in range(n):
            if present is None or present[i][k]:
                out[i] += prob[i, ..., k:k + 1].double() * ass[k, i]
    return out


def bits(present):
    return torch.tensor([sum(1 << k for k, v in enumerate(row) if v) for row in present], dtype=torch.int32, device='cuda')


def new_path(hip, refs, q, emb, weight, bias, t, vb=None, in_amax=None):
    prob = hip.mrattn_prob_nhwc(q, emb, t, vb, q_scale=q.shape[3] ** -0.5)
    return hip.mrattn_blend_conv(refs, prob, hip.conv_pack_weight(weight, 16), bias, t, vb, in_amax=in_amax), prob


def parent_path(hip, refs, q, emb, weight, bias, t):
    """conv_ass through the engine's convolution (the kernel the model picks), then mrattn_fwd_nhwc"""
    from mrefsr_amd.archs import nhwc
    c = refs.shape[3]
    mod = torch.nn.Conv2d(c, 2 * c, 3, 1, 1).cuda()
    with torch.no_grad():
        mod.weight.copy_(weight), mod.bias.copy_(bias)
        return hip.mrattn_fwd_nhwc(q, emb, nhwc.conv(mod, refs, amax=False), t, q_scale=c ** -0.5)


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('t', [1, 2, 5])
@pytest.mark.parametrize('c', [64, 128, 256])
def test_blend_conv_vs_float64(hip, c, t, n):
    for i, (h, w) in enumerate(MAPS):
        refs, q, emb, weight, bias = operands(c, t, n, h, w, 1000 * c + 10 * t + n + i)
        got, prob = new_path(hip, refs, q, emb, weight, bias, t)
        want = want64(refs, prob, weight, bias, t)
        err = float((got.double() - want).abs().max())
        err_parent = float((parent_path(hip, refs, q, emb, weight, bias, t).double() - want).abs().max())
        print(f'c={c} t={t} n={n} {h}x{w}: max|err| new {err:.3e} parent {err_parent:.3e} (max|want| {float(want.abs().max()):.2f})')
        torch.testing.assert_close(got.double(), want, **BAR)
    assert not hip.conv_range_tripped()


def test_blend_conv_sixteen_references(hip):
    """T = 16 > the five maps a pass stages: four groups, each group's partial blend split and multiplied on its own"""
    c, t, n = 64, 16, 2
    for i, (h, w) in enumerate(MAPS):
        refs, q, emb, weight, bias = operands(c, t, n, h, w, 77 + i)
        got, prob = new_path(hip, refs, q, emb, weight, bias, t)
        want = want64(refs, prob, weight, bias, t)
        print(f'c={c} t={t} n={n} {h}x{w}: max|err| {float((got.double() - want).abs().max()):.3e}')
        torch.testing.assert_close(got.double(), want, **BAR)


@pytest.mark.parametrize('c,t', [(64, 2), (128, 4), (256, 2)])
def test_closed_form_ones(hip, c, t):
    """all-ones maps and weights, uniform prob 1 / t (a power of two: the blend is exactly 1), no bias: C * {4, 6, 9} by corner / edge / interior"""
    for h, w in MAPS:
        refs = torch.ones(t * 2, h, w, c, device='cuda')
        prob = torch.full((2, h, w, t), 1.0 / t, device='cuda')
        got = hip.mrattn_blend_conv(refs, prob, hip.conv_pack_weight(torch.ones(2 * c, c, 3, 3, device='cuda'), 16), None, t)
        cnt = F.conv2d(torch.ones(1, 1, h, w, device='cuda'), torch.ones(1, 1, 3, 3, device='cuda'), padding=1)[0, 0]
        assert set(cnt.flatten().tolist()) <= {4.0, 6.0, 9.0}
        assert torch.equal(got, (c * cnt)[None, :, :, None].expand(2, h, w, 2 * c))


def test_one_hot_prob_is_the_plain_convolution(hip):
    c, t, n, (h, w) = 128, 5, 3, MAPS[2]
    refs, _, _, weight, bias = operands(c, t, n, h, w, 5)
    pick = torch.randint(0, t, (n, h, w), device='cuda', generator=gen(6))
    prob = F.one_hot(pick, t).float()
    got = hip.mrattn_blend_conv(refs, prob, hip.conv_pack_weight(weight, 16), bias, t)
    conv = F.conv2d(refs.double().permute(0, 3, 1, 2), weight.double(), bias.double(), padding=1).permute(0, 2, 3, 1).reshape(t, n, h, w, 2 * c)
    want = torch.gather(conv, 0, pick[None, ..., None].expand(1, n, h, w, 2 * c))[0]
    torch.testing.assert_close(got.double(), want, **BAR)


@pytest.mark.parametrize('c', [64, 256])
def test_masks(hip, c):
    """an absent reference full of NaN / Inf reaches nothing and the result is the run without it, bit for bit; a sample without a
    present reference gives exact zeros"""
    t, n, (h, w) = 5, 3, MAPS[1]
    refs, q, emb, weight, bias = operands(c, t, n, h, w, 31 + c)
    refs, emb = refs.view(t, n, h, w, c).clone(), emb.view(t, n, h, w, c).clone()
    refs[2, :, ::2], refs[2, :, 1::2], emb[2] = float('nan'), float('inf'), float('nan')
    present = [[1, 1, 0, 1, 1]] * n
    got, prob = new_path(hip, refs.view(-1, h, w, c), q, emb.view(-1, h, w, c), weight, bias, t, bits(present))
    assert torch.isfinite(got).all() and not prob[..., 2].any()
    keep = [0, 1, 3, 4]
    got4, prob4 = new_path(hip, refs[keep].reshape(-1, h, w, c), q, emb[keep].reshape(-1, h, w, c), weight, bias, 4)
    assert torch.equal(prob[..., keep], prob4) and torch.equal(got, got4)
    torch.testing.assert_close(got.double(), want64(refs.view(-1, h, w, c).nan_to_num(0, 0, 0), prob, weight, bias, t, present), **BAR)
    assert not hip.conv_range_tripped()   # (the absent map was never staged)
    present = [[1, 0, 0, 0, 1], [0, 0, 0, 0, 0], [0, 1, 0, 1, 0]]
    got, prob = new_path(hip, refs.view(-1, h, w, c), q, emb.view(-1, h, w, c), weight, bias, t, bits(present))
    assert not got[1].any() and not prob[1].any() and torch.isfinite(got).all()
    torch.testing.assert_close(got.double(), want64(refs.view(-1, h, w, c).nan_to_num(0, 0, 0), prob, weight, bias, t, present), **BAR)


@pytest.mark.parametrize('c', [64, 128, 256])
def test_softmax_weights_entry(hip, c):
    """fp32 dot products of c terms (4-wide partial sums, then a shuffle tree) against float64: the logit error is below
    (log2(c) + 3) eps sum|q e| scale ~ 7e-6 for these operands, and so is the relative error of a weight: rtol = atol = 1e-5"""
    t, n, (h, w) = 5, 3, MAPS[1]
    _, q, emb, _, _ = operands(c, t, n, h, w, 9 + c)
    present = [[1, 1, 1, 1, 1], [0, 1, 0, 1, 1], [1, 0, 0, 0, 0]]
    for vb, pres in ((None, [[1] * t] * n), (bits(present), present)):
        prob = hip.mrattn_prob_nhwc(q, emb, t, vb, q_scale=c ** -0.5)
        logit = torch.einsum('nhwc,tnhwc->nhwt', q.double() * c ** -0.5, emb.view(t, n, h, w, c).double())
        on = torch.tensor(pres, dtype=torch.bool, device='cuda')[:, None, None, :].expand_as(logit)
        want = torch.softmax(logit.masked_fill(~on, float('-inf')), dim=-1)
        torch.testing.assert_close(prob.double(), want, rtol=1e-5, atol=1e-5)
        # each weight carries the roundings of the denominator (t - 1 adds), the reciprocal and one product; the check's own sum adds its
        assert float((prob.double().sum(-1) - 1).abs().max()) <= (t + 2) * np.finfo(np.float32).eps
        assert not prob[~on].any()
    # the weights are the ones mrattn_fwd_nhwc applies: with ass = one-hot channels the parent kernel returns them
    ass = torch.zeros(t, n, h, w, 2 * c, device='cuda')
    for k in range(t):
        ass[k, ..., k] = 1
    prob = hip.mrattn_prob_nhwc(q, emb, t, q_scale=c ** -0.5)
    assert torch.equal(hip.mrattn_fwd_nhwc(q, emb, ass.view(-1, h, w, 2 * c), t, q_scale=c ** -0.5)[..., :t], prob)


def test_two_launches_give_the_same_bits(hip):
    c, t, n, (h, w) = 128, 5, 3, MAPS[2]
    refs, q, emb, weight, bias = operands(c, t, n, h, w, 3)
    a, pa = new_path(hip, refs, q, emb, weight, bias, t)
    b, pb = new_path(hip, refs, q, emb, weight, bias, t)
    assert torch.equal(a, b) and torch.equal(pa, pb)


def test_range_flag_and_input_scale(hip):
    c, t, n, (h, w) = 64, 2, 1, MAPS[1]
    refs, q, emb, weight, bias = operands(c, t, n, h, w, 4)
    refs = refs * 1e5 / 4
    refs[0, 3, 5, 7] = 1e5
    assert not hip.conv_range_tripped()
    new_path(hip, refs, q, emb, weight, bias, t)
    assert hip.conv_range_tripped()                       # 1e5 staged as it is: outside fp16
    got, prob = new_path(hip, refs, q, emb, weight, bias, t, in_amax=refs.abs().amax().reshape(1))
    assert not hip.conv_range_tripped()                   # scaled by the tensor's power of two: inside
    want = want64(refs, prob, weight, bias, t)
    m = float(want.abs().max())
    torch.testing.assert_close(got.double() / m, want / m, **BAR)


def test_module_scales_references_beyond_the_fp16_range_in_one_pass(hip):
    """forward_nhwc hands the blend-conv launch max |refs| (measured on demand for a tensor without a live word, as conv_ass's
    Winograd launch had it): references of 1e5 neither trip the range flag nor cost the range-free re-run"""
    from mrefsr_amd.archs.ref_mrapa_restoration_arch import MRAPAFusion
    torch.manual_seed(1)
    m = MRAPAFusion(nf=64, ref_nf=64).cuda().eval()
    g = gen(8)
    target = torch.randn(2, 12, 20, 64, device='cuda', generator=g)
    refs = torch.randn(10, 12, 20, 64, device='cuda', generator=g) * 2.5e4
    refs[3, 5, 7, 9] = 1e5
    hip.conv_range_tripped()
    with torch.no_grad():
        m.conv_ass.weight.mul_(1e-4)   # (the assembled features, which the 1x1 layers behind read unscaled, stay of order 1)
        out = m.forward_nhwc(target, refs, 5)
    assert not hip.conv_range_tripped() and torch.isfinite(out).all()


@pytest.mark.parametrize('c,h,w', [(64, 12, 20), (128, 10, 14), (256, 8, 12)])
@pytest.mark.parametrize('masked', [False, True])
def test_module_new_path_against_parent_path(c, h, w, masked):
    """MRAPAFusion.forward_nhwc with the blend in front of conv_ass against conv_ass + mrattn_fwd_nhwc (the class attribute flipped);
    10 x 14 goes through the reflect pad and the crop"""
    from mrefsr_amd.archs.ref_mrapa_restoration_arch import MRAPAFusion
    torch.manual_seed(c + h)
    t, n = 5, 3
    m = MRAPAFusion(nf=64, ref_nf=c).cuda().eval()
    g = gen(c)
    target = torch.randn(n, h, w, 64, device='cuda', generator=g)
    refs = torch.randn(t * n, h, w, c, device='cuda', generator=g)
    valid = torch.tensor([[1, 1, 1, 1, 1], [0, 1, 0, 1, 1], [1, 0, 0, 0, 0]], dtype=torch.bool, device='cuda') if masked else None
    assert MRAPAFusion.BLEND_FIRST
    with torch.no_grad():
        new = m.forward_nhwc(target, refs, t, ref_valid=valid)
        MRAPAFusion.BLEND_FIRST = False
        try:
            old = m.forward_nhwc(target, refs, t, ref_valid=valid)
        finally:
            MRAPAFusion.BLEND_FIRST = True
    assert new.shape == (n, h, w, 64)
    print(f'c={c} {h}x{w} masked={masked}: max|new - parent| {float((new - old).abs().max()):.3e} (max|parent| {float(old.abs().max()):.2f})')
    torch.testing.assert_close(new, old, **BAR)
