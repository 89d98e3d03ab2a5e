"""GPU: the attention core under per-sample reference masks (mrefsr_mrattn_*_masked_*; csrc/mrattn.hip, csrc/train.hip).

The comparison is the literal permute / matmul / softmax formulation of ref_mrapa_restoration_arch.py:321-335 in torch fp64 on the
CPU, applied to each sample with that sample's valid references only.  Tolerances are those test_mrattn_fwd_bwd_vs_oracle holds the
unmasked kernels to (forward rtol 1e-5 / atol 1e-5, prob atol 1e-6, gradients rtol 1e-4 / atol 1e-5); as a control, the unmasked
kernel on the compacted references of one sample is held to the same numbers in the same test.

Shapes: H x W = 5 x 7 (HW = 35 is no multiple of the 4 / 2 pixels a wave holds at c = 64 / 128: waves straddle two samples with
different masks and end in clamped tail lanes); N = 3, T = 5 with the first valid t not 0; N = 1, T = 16 with only the last slot
valid (the maximum's initial value); N = 2, T = 1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H, W = 5, 7
CASES = {
    'n3t5': (3, 5, [[1, 1, 1, 1, 1], [0, 1, 0, 0, 1], [1, 0, 0, 0, 0]]),
    'n1t16_last': (1, 16, [[0] * 15 + [1]]),
    'n2t1': (2, 1, [[1], [1]]),
}
FWD = dict(rtol=1e-5, atol=1e-5)
PROB = dict(rtol=1e-5, atol=1e-6)
GRAD = dict(rtol=1e-4, atol=1e-5)
SENTINEL = 777.0


@pytest.fixture(scope='module')
def hip():
    from mrefsr_amd import hip as h
    return h


def _words(masks, garbage=0):
    w = [sum(int(v) << t for t, v in enumerate(row)) | garbage for row in masks]
    return torch.from_numpy(np.array(w, dtype=np.uint32).view(np.int32)).cuda()


def _formulation(q, emb, ass):
    """ref :321-335 for one sample: q [1,c,h,w], emb [1,t,c,h,w], ass [1,t,2c,h,w] -> (refs [1,2c,h,w], prob [1,t,h,w])"""
    n, _, h, w = q.shape
    et = q.permute(0, 2, 3, 1).unsqueeze(3).contiguous().flatten(0, 2)
    e2 = emb.permute(0, 3, 4, 2, 1).contiguous().flatten(0, 2)
    a2 = ass.permute(0, 3, 4, 1, 2).contiguous().flatten(0, 2)
    prob = F.softmax(torch.matmul(et, e2), dim=2)
    refs = torch.matmul(prob, a2).squeeze(1).unflatten(0, (n, h, w)).permute(0, 3, 1, 2).contiguous()
    return refs, prob.squeeze(1).unflatten(0, (n, h, w)).permute(0, 3, 1, 2)


_cache = {}


def _case(name, c):
    """inputs (fp32, NCHW, references [N][T]) and the fp64 reference of every output, computed once per (case, c)"""
    if (name, c) in _cache:
        return _cache[name, c]
    n, t, masks = CASES[name]
    rng = np.random.default_rng(1000 * n + 100 * t + c)
    q = torch.from_numpy((rng.standard_normal((n, c, H, W)) * c ** -0.5).astype(np.float32))
    emb = torch.from_numpy(rng.standard_normal((n, t, c, H, W)).astype(np.float32))
    ass = torch.from_numpy(rng.standard_normal((n, t, 2 * c, H, W)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((n, 2 * c, H, W)).astype(np.float32))
    out, prob = torch.zeros(n, 2 * c, H, W, dtype=torch.float64), torch.zeros(n, t, H, W, dtype=torch.float64)
    gq, gemb, gass = torch.zeros(q.shape, dtype=torch.float64), torch.zeros(emb.shape, dtype=torch.float64), torch.zeros(ass.shape, dtype=torch.float64)
    for i in range(n):
        keep = [k for k in range(t) if masks[i][k]]
        qi = q[i:i + 1].double().requires_grad_()
        ei = emb[i:i + 1, keep].double().requires_grad_()
        ai = ass[i:i + 1, keep].double().requires_grad_()
        o, p = _formulation(qi, ei, ai)
        o.backward(g[i:i + 1].double())
        out[i], prob[i, keep] = o.detach()[0], p.detach()[0]
        gq[i], gemb[i, keep], gass[i, keep] = qi.grad[0], ei.grad[0], ai.grad[0]
    want = dict(out=out, prob=prob, gq=gq, gemb=gemb, gass=gass)
    _cache[name, c] = (q, emb, ass, g, masks, {k: v.numpy() for k, v in want.items()})
    return _cache[name, c]


def _fill_absent(x, masks, value):
    """x [N,T,...] with the slots of absent references overwritten"""
    x = x.clone()
    for i, row in enumerate(masks):
        for k, v in enumerate(row):
            if not v:
                x[i, k] = value
    return x


def _absent(masks):
    return [(i, k) for i, row in enumerate(masks) for k, v in enumerate(row) if not v]


# ---- layouts: [N,T,C,H,W] <-> what the kernels take
def _nchw_stack(x, t_major):
    x = x.transpose(0, 1) if t_major else x
    return x.reshape(-1, *x.shape[2:]).contiguous().cuda()


def _nchw_unstack(y, n, t, t_major):
    y = y.cpu()
    return y.view(t, n, *y.shape[1:]).transpose(0, 1) if t_major else y.view(n, t, *y.shape[1:])


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def _nhwc_stack(x):
    return x.permute(1, 0, 3, 4, 2).reshape(-1, H, W, x.shape[2]).contiguous().cuda()


def _nhwc_unstack(y, n, t):
    return y.cpu().view(t, n, *y.shape[1:]).permute(1, 0, 4, 2, 3)


def _sentinels(*like):
    return tuple(torch.full_like(v, SENTINEL) for v in like)


def _check(got, want, tol, what):
    got = got.detach().cpu().numpy()
    err = np.abs(got - want)
    print(f'{what}: max abs err {err.max():.3e} (largest |want| {np.abs(want).max():.3e})')
    np.testing.assert_allclose(got, want, err_msg=what, **tol)


@pytest.mark.parametrize('t_major', [False, True], ids=['n_major', 't_major'])
@pytest.mark.parametrize('name', list(CASES))
def test_masked_nchw_kernels_vs_the_reference_formulation_on_the_valid_references(hip, name, t_major):
    c = 32
    q, emb, ass, g, masks, want = _case(name, c)
    n, t = emb.shape[:2]
    vb = _words(masks)
    runs = []
    for fill in (0.0, float('nan')):
        e, a = _nchw_stack(_fill_absent(emb, masks, fill), t_major), _nchw_stack(_fill_absent(ass, masks, fill), t_major)
        out, prob = hip.mrattn_fwd_masked(q.cuda(), e, a, t, vb, t_major=t_major)
        bufs = _sentinels(q.cuda(), e, a)
        gq, gemb, gass = hip.mrattn_bwd_masked(q.cuda(), e, a, prob, g.cuda(), t, vb, t_major=t_major, out=bufs)
        runs.append((out, prob, gq, _nchw_unstack(gemb, n, t, t_major), _nchw_unstack(gass, n, t, t_major)))
    out, prob, gq, gemb, gass = runs[0]
    _check(out, want['out'], FWD, 'out')
    _check(prob, want['prob'], PROB, 'prob')
    _check(gq, want['gq'], GRAD, 'g_q')
    _check(gemb, want['gemb'], GRAD, 'g_emb')
    _check(gass, want['gass'], GRAD, 'g_ass')
    for i, k in _absent(masks):   # exact zeros, written over the sentinel
        assert not prob[i, k].any() and not gemb[i, k].any() and not gass[i, k].any(), (i, k)
    for zero_filled, nan_filled in zip(*runs):   # NaN in the absent slots reaches nothing
        assert torch.isfinite(nan_filled).all() and torch.equal(zero_filled, nan_filled)
    # control: the unmasked kernels on the compacted references of one sample, same bars
    i = min(1, n - 1)
    keep = [k for k in range(t) if masks[i][k]]
    qc, ec, ac = q[i:i + 1].cuda(), _nchw_stack(emb[i:i + 1, keep], t_major), _nchw_stack(ass[i:i + 1, keep], t_major)
    o1, p1 = hip.mrattn_fwd(qc, ec, ac, len(keep), t_major=t_major)
    q1, e1, a1 = hip.mrattn_bwd(qc, ec, ac, p1, g[i:i + 1].cuda(), len(keep), t_major)
    _check(o1, want['out'][i:i + 1], FWD, 'control out')
    _check(p1, want['prob'][i:i + 1, keep], PROB, 'control prob')
    _check(q1, want['gq'][i:i + 1], GRAD, 'control g_q')
    _check(_nchw_unstack(e1, 1, len(keep), t_major), want['gemb'][i:i + 1, keep], GRAD, 'control g_emb')
    _check(_nchw_unstack(a1, 1, len(keep), t_major), want['gass'][i:i + 1, keep], GRAD, 'control g_ass')


@pytest.mark.parametrize('c', [64, 128, 256])
@pytest.mark.parametrize('name', list(CASES))
def test_masked_channels_last_kernels_vs_the_reference_formulation_on_the_valid_references(hip, name, c):
    q, emb, ass, g, masks, want = _case(name, c)
    n, t = emb.shape[:2]
    vb = _words(masks)
    ql, gl = _nhwc(q), _nhwc(g)
    runs = []
    for fill in (0.0, float('nan')):
        e, a = _nhwc_stack(_fill_absent(emb, masks, fill)), _nhwc_stack(_fill_absent(ass, masks, fill))
        out = hip.mrattn_fwd_nhwc_masked(ql, e, a, t, vb)
        bufs = _sentinels(ql, e, a)
        gq, gemb, gass = hip.mrattn_bwd_nhwc_masked(ql, e, a, gl, t, vb, out=bufs)
        runs.append((out.permute(0, 3, 1, 2), gq.permute(0, 3, 1, 2), _nhwc_unstack(gemb, n, t), _nhwc_unstack(gass, n, t)))
    out, gq, gemb, gass = runs[0]
    _check(out, want['out'], FWD, 'out')
    _check(gq, want['gq'], GRAD, 'g_q')
    _check(gemb, want['gemb'], GRAD, 'g_emb')
    _check(gass, want['gass'], GRAD, 'g_ass')
    for i, k in _absent(masks):
        assert not gemb[i, k].any() and not gass[i, k].any(), (i, k)
    for zero_filled, nan_filled in zip(*runs):
        assert torch.isfinite(nan_filled).all() and torch.equal(zero_filled, nan_filled)
    # control: the unmasked kernels on the compacted references of one sample, same bars
    i = min(1, n - 1)
    keep = [k for k in range(t) if masks[i][k]]
    qc, ec, ac = _nhwc(q[i:i + 1]), _nhwc_stack(emb[i:i + 1, keep]), _nhwc_stack(ass[i:i + 1, keep])
    o1 = hip.mrattn_fwd_nhwc(qc, ec, ac, len(keep))
    q1, e1, a1 = hip.mrattn_bwd_nhwc(qc, ec, ac, _nhwc(g[i:i + 1]), len(keep))
    _check(o1.permute(0, 3, 1, 2), want['out'][i:i + 1], FWD, 'control out')
    _check(q1.permute(0, 3, 1, 2), want['gq'][i:i + 1], GRAD, 'control g_q')
    _check(_nhwc_unstack(e1, 1, len(keep)), want['gemb'][i:i + 1, keep], GRAD, 'control g_emb')
    _check(_nhwc_unstack(a1, 1, len(keep)), want['gass'][i:i + 1, keep], GRAD, 'control g_ass')


def _run_all(hip, q, emb, ass, g, t, vb, c_nhwc=True):
    """every masked kernel on one set of inputs -> list of result tensors"""
    res = []
    for t_major in (False, True):
        e, a = _nchw_stack(emb, t_major), _nchw_stack(ass, t_major)
        out, prob = hip.mrattn_fwd_masked(q.cuda(), e, a, t, vb, t_major=t_major)
        res += [out, prob, *hip.mrattn_bwd_masked(q.cuda(), e, a, prob, g.cuda(), t, vb, t_major=t_major)]
    if c_nhwc:
        ql, e, a = _nhwc(q), _nhwc_stack(emb), _nhwc_stack(ass)
        res += [hip.mrattn_fwd_nhwc_masked(ql, e, a, t, vb), *hip.mrattn_bwd_nhwc_masked(ql, e, a, _nhwc(g), t, vb)]
    return res


@pytest.mark.parametrize('c', [64, 256])
def test_bits_at_and_above_t_are_ignored(hip, c):
    q, emb, ass, g, masks, _ = _case('n3t5', c)
    clean = _run_all(hip, q, emb, ass, g, 5, _words(masks))
    for garbage in (0xffffffe0, 0x80000020, 0x0000ffe0):
        dirty = _run_all(hip, q, emb, ass, g, 5, _words(masks, garbage))
        assert all(torch.equal(u, v) for u, v in zip(clean, dirty)), hex(garbage)


@pytest.mark.parametrize('c', [64, 128, 256])
def test_a_word_without_a_valid_bit_gives_zeros_for_that_sample_only(hip, c):
    q, emb, ass, g, masks, _ = _case('n3t5', c)
    n, t = 3, 5
    full = _run_all(hip, q, emb, ass, g, t, _words(masks))
    none = [[1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0]]
    got = _run_all(hip, q, _fill_absent(emb, none, float('nan')), _fill_absent(ass, none, float('nan')), g, t, _words(none, 0xffe0))
    # (out, prob, g_q, g_emb, g_ass) x two NCHW stackings, then (out, g_q, g_emb, g_ass) channels-last: sample index of every row
    per_sample = lambda v, stacked, t_major: (v.view(t, n, *v.shape[1:]).transpose(0, 1) if t_major else v.view(n, t, *v.shape[1:])) if stacked else v  # noqa: E731
    layout = [(False, False), (False, False), (False, False), (True, False), (True, False),
              (False, False), (False, False), (False, False), (True, True), (True, True),
              (False, False), (False, False), (True, True), (True, True)]
    for u, v, (stacked, t_major) in zip(full, got, layout):
        u, v = per_sample(u, stacked, t_major), per_sample(v, stacked, t_major)
        assert not v[1].any()                                   # exact zeros, no 0 / 0
        assert torch.equal(u[0], v[0]) and torch.equal(u[2], v[2])


@pytest.mark.parametrize('c', [64, 128, 256])
def test_masked_bf16_forward_is_the_masked_f32_forward_rounded(hip, c):
    """the bar of test_kernels_gpu.py for the unmasked bf16 core: on bf16-representable inputs the bf16 kernel's result is the
    f32 kernel's, rounded to bf16"""
    q, emb, ass, _, masks, _ = _case('n3t5', c)
    b = lambda v: v.bfloat16()  # noqa: E731
    ql, e, a = (b(v).float() for v in (_nhwc(q), _nhwc_stack(_fill_absent(emb, masks, float('nan'))), _nhwc_stack(_fill_absent(ass, masks, float('inf')))))
    vb = _words(masks)
    a32 = hip.mrattn_fwd_nhwc_masked(ql, e, a, 5, vb)
    a16 = hip.mrattn_fwd_nhwc_masked(b(ql), b(e), b(a), 5, vb)
    assert a16.dtype == torch.bfloat16 and torch.isfinite(a32).all()
    assert torch.equal(a16.float(), a32.bfloat16().float())


@pytest.mark.parametrize('c', [64, 128, 256])
def test_masked_q_scale_equals_the_separate_pass_over_q(hip, c):
    q, emb, ass, _, masks, _ = _case('n3t5', c)
    ql, e, a, vb = _nhwc(q), _nhwc_stack(emb), _nhwc_stack(ass), _words(masks)
    scale = float(c) ** -0.5
    assert torch.equal(hip.mrattn_fwd_nhwc_masked(ql, e, a, 5, vb, q_scale=scale), hip.mrattn_fwd_nhwc_masked(ql * scale, e, a, 5, vb))
