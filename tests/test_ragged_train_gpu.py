"""GPU: net_g trains on the channels-last engine when the LR sides are not multiples of 4.  MRAPAFusion's reflect pad to a
multiple of 4 and the crop back (ref_mrapa_restoration_arch.py:306-311, 348) are autograd nodes on the kernels of csrc/pad.hip
(archs/nhwc_train.py _Pad / _Crop), so the whole step runs without the generic torch path: checked node by node against fp64
autograd, as a whole step against the generic engine and the reference's own step (tests/golden/e2e_ragged.npz: B = 2, K = 3,
LR 45 x 39), and under hipGraph replay."""
import copy

import numpy as np
import pytest
import torch

import synth
from test_configs_gpu import _check_forward_against_reference, _check_train_step_against_reference, _golden_model

pytestmark = pytest.mark.gpu


def _close(got, want, tol=2e-5):
    got, want = got.detach().double().cpu(), want.detach().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = float(want.abs().max()) + 1e-30
    err = float((got - want).abs().max()) / scale
    assert err <= tol, err


class _Fp64Attention:
    """the attention core of _fuse (:321-335) restated in torch ops, for CPU fp64 autograd (the module's own is a HIP kernel)"""

    @staticmethod
    def apply(q, emb, ass, t, t_major):
        n = q.shape[0]
        e = emb.view(t, n, *emb.shape[1:]) if t_major else emb.view(n, t, *emb.shape[1:]).transpose(0, 1)
        a = ass.view(t, n, *ass.shape[1:]) if t_major else ass.view(n, t, *ass.shape[1:]).transpose(0, 1)
        p = torch.softmax(torch.einsum('nchw,tnchw->nthw', q, e), 1)
        return torch.einsum('nthw,tnchw->nchw', p, a)


def _fusion(ref_nf, seed):
    from mrefsr_amd.archs.ref_mrapa_restoration_arch import MRAPAFusion
    torch.manual_seed(seed)
    return MRAPAFusion(nf=64, ref_nf=ref_nf)


@pytest.mark.parametrize('geom', [(2, 19, 13, 256), (1, 45, 39, 128), (2, 45, 39, 64)], ids=lambda g: 'x'.join(map(str, g)))
def test_fusion_node_at_ragged_sizes_matches_fp64_autograd_of_the_generic_form(geom, monkeypatch):
    from mrefsr_amd.archs import ref_mrapa_restoration_arch as arch
    n, h, w, c = geom
    t = 3
    m = _fusion(c, h * w + c)
    torch.manual_seed(h + w)
    target, refs = torch.randn(n, h, w, 64), torch.randn(t * n, h, w, c)
    mg = copy.deepcopy(m).cuda()
    tg, rg = target.cuda().requires_grad_(), refs.cuda().requires_grad_()
    out = mg.forward_nhwc(tg, rg, t)
    assert type(out.grad_fn).__name__ == '_CropBackward'        # recorded on the engine's nodes, not ATen's
    # fp64 CPU autograd of the generic form (NCHW, F.pad / slice)
    monkeypatch.setattr(arch, '_MultiRefAttention', _Fp64Attention)
    md = copy.deepcopy(m).double()
    tr = target.permute(0, 3, 1, 2).double().requires_grad_()
    rr = refs.permute(0, 3, 1, 2).double().requires_grad_()
    want = md._fuse(tr, rr, t, t_major=True)
    _close(out.permute(0, 3, 1, 2), want)
    gout = torch.randn(want.shape, dtype=torch.float64)
    want.backward(gout)
    out.backward(gout.permute(0, 2, 3, 1).float().contiguous().cuda())
    _close(tg.grad.permute(0, 3, 1, 2), tr.grad)
    _close(rg.grad.permute(0, 3, 1, 2), rr.grad)
    for (name, pg), (_, pd) in zip(mg.named_parameters(), md.named_parameters()):
        assert pg.grad is not None, name
        # (a PReLU slope's gradient is ONE fp32 sum over every product of its layer -- 5e5 of them for conv_emb2 at 2 x 19 x 13,
        # t = 3 -- with cancellation: 2.4e-5 of the result against fp64 was measured there; every other gradient holds 2e-5)
        _close(pg.grad, pd.grad, 1e-4 if pg.numel() == 1 else 2e-5)


@pytest.mark.parametrize('geom', [(2, 19, 13, 256), (1, 45, 39, 128), (2, 90, 78, 64), (1, 10, 11, 64)], ids=lambda g: 'x'.join(map(str, g)))
def test_fusion_inference_at_ragged_sizes_is_bit_equal_to_the_f_pad_round_trip(geom):
    from mrefsr_amd.archs import nhwc
    n, h, w, c = geom
    t = 3
    m = _fusion(c, h + w).cuda()
    torch.manual_seed(h * w)
    target, refs = torch.randn(n, h, w, 64, device='cuda'), torch.randn(t * n, h, w, c, device='cuda')
    with torch.no_grad():
        got = m.forward_nhwc(target, refs, t)
        # the form before the pad kernels: as_nchw / F.pad / to_nhwc, the aligned body, slice + copy
        tp = nhwc.to_nhwc(m.spatial_padding(nhwc.as_nchw(target)))
        rp = nhwc.to_nhwc(m.spatial_padding(nhwc.as_nchw(refs)))
        want = m.forward_nhwc(tp, rp, t)[:, :h, :w, :].contiguous()
    assert torch.equal(got, want)
    word = nhwc.amax_word(got)                                    # the crop measured the result's own max |x|
    assert float(word) == float(got.abs().max())


def _net_g_grads(model):
    return {n: p.grad.detach().double().cpu() for n, p in model.get_bare_model(model.net_g).named_parameters()}


def _synth_data(b, k, lr_h, lr_w, key):
    samples = [synth.sr_sample(f'{key}/s{i}', k, lr_h, lr_w) for i in range(b)]
    return {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}


@pytest.mark.parametrize('lr', [(45, 39), (40, 40)], ids=['lr45x39', 'lr40x40_control'])
def test_training_step_at_a_ragged_size_calls_no_library_convolution(golden, monkeypatch, lr):
    """B = 2, K = 3: the whole optimisation step (extractor, matching, net_g forward and backward, Adam) without F.conv2d -- at
    45 x 39 net_g went to the generic torch path before the pad / crop nodes existed; 40 x 40 is the control"""
    g = golden('e2e_ragged')
    model, data, _ = _golden_model(g, True)
    if lr != (45, 39):
        data = _synth_data(2, 3, *lr, 'e2e_ragged/control')

    def no_library_conv(*a, **k):
        raise AssertionError('F.conv2d called: the step left the channels-last engine')

    monkeypatch.setattr(torch.nn.functional, 'conv2d', no_library_conv)
    model.feed_data(data)
    model.optimize_parameters(1)
    assert np.isfinite(model.get_current_log()['l_g_pix'])
    assert all(v is not None for v in _net_g_grads(model).values())


@pytest.mark.parametrize('shape', [(2, 3, 45, 39), (2, 3, 75, 53)], ids=lambda s: f'b{s[0]}k{s[1]}lr{s[2]}x{s[3]}')
def test_training_step_at_a_ragged_size_on_both_engines(golden, monkeypatch, shape):
    """the channels-last engine and the generic NCHW autograd path give the same loss and gradients, parameter by parameter"""
    from mrefsr_amd.archs import nhwc_train
    b, k, lr_h, lr_w = shape
    g = golden('e2e_ragged')
    grads, losses = [], []
    for enabled in (True, False):
        monkeypatch.setattr(nhwc_train, 'ENABLED', enabled)
        model, data, _ = _golden_model(g, True)
        if (lr_h, lr_w) != (45, 39):
            data = _synth_data(b, k, lr_h, lr_w, 'ragged_both')
        model.feed_data(data)
        model.optimize_parameters(1)
        losses.append(float(model.get_current_log()['l_g_pix']))
        grads.append(_net_g_grads(model))
        del model
    assert abs(losses[0] - losses[1]) <= 1e-5 * abs(losses[1])
    for n in grads[0]:
        a, b_ = grads[0][n], grads[1][n]
        # a bias or PReLU-slope gradient is a sum over every pixel of its layer (168 k per channel for head_large.conv_emb2 at the 4x
        # scale of this step, a scale that needs no padding), with cancellation: the two engines' fp32 reductions were measured up to
        # 1.5e-3 of the largest element apart there -- and as far apart at the aligned 44 x 40, where no pad or crop runs
        tol = 5e-3 if b_.dim() == 1 else 1e-3
        assert float((a - b_).abs().max()) <= tol * float(b_.abs().max()) + 1e-9, n


def test_ragged_size_forward_and_train_step_vs_reference(golden):
    """B = 2, K = 3, LR 45 x 39 (pads 3 x 1 at the small scale, 2 x 2 at the medium one): test() output and the reference's own
    optimisation step (loss, per-parameter gradient fingerprints, post-Adam parameter sums)"""
    g = golden('e2e_ragged')
    model, data, _ = _golden_model(g, True)
    _check_forward_against_reference(g, model, data)
    _check_train_step_against_reference(g, model)


def test_graph_replayed_training_steps_at_a_ragged_size_equal_eager_steps(golden, monkeypatch):
    """MREFSR_TRAIN_GRAPH=1 at LR 45 x 39: the pad / crop nodes are captured with the rest of the step; six steps (three eager, then
    replays) leave the same parameters as six eager steps (the bulk criterion of test_train_engine_gpu.py's graph test)"""
    from mrefsr_amd.archs import nhwc_train
    monkeypatch.setenv('MREFSR_TRAIN_GRAPH', '1')
    g = golden('e2e_ragged')
    finals, losses = [], []
    for graphed in (True, False):
        model, data, _ = _golden_model(g, True)
        if not graphed:
            monkeypatch.setattr(type(model), '_optimize_graphed', lambda self, step: False)
        for it in range(1, 7):
            model.feed_data(data)
            model.optimize_parameters(it)
        if graphed:
            assert model._tgraph['fb'] is not None
        losses.append(float(model.get_current_log()['l_g_pix']))
        finals.append({n: p.detach().double().cpu() for n, p in model.get_bare_model(model.net_g).named_parameters()})
        del model
    assert nhwc_train.ENABLED
    assert abs(losses[0] - losses[1]) <= 1e-3 * abs(losses[1]), losses
    bad = tot = 0
    for n in finals[0]:
        a, b = finals[0][n], finals[1][n]
        bad += int(((a - b).abs() > 2e-5 * float(b.abs().max()) + 1e-7).sum())
        tot += a.numel()
        assert float((a - b).abs().max()) <= 6 * 2.5e-4, n
    print(f'graph vs eager after 6 steps at 45 x 39: {bad} of {tot} elements differ, losses {losses}')
    assert bad <= 0.05 * tot, (bad, tot)
