"""GPU: per-sample reference masks through the network and the model (`ref_valid`: mixed reference counts in one batch).

The property under test: with reference k of sample b marked absent, sample b's output -- and its share of every gradient -- is
what the network gives for sample b fed alone with only its valid references, through the unmasked path (which the existing
goldens pin to the reference implementation); and nothing depends on what sits in an absent slot.

One model serves the whole module: its learning rates are set to 0, so optimize_parameters() leaves the weights as they are and
every step computes its gradients on the same network."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
from test_configs_gpu import _golden_model

pytestmark = pytest.mark.gpu

MASK = [[1, 1, 1], [0, 1, 0]]


# ------------------------------------------------------------------------------------------------ the fusion node
def _close(got, want, tol, what):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)
    print(f'{what}: {err:.3e} of the largest element (bar {tol:.0e})')
    assert err <= tol, (what, err)


class _Fp64MaskedAttention:
    """the attention core of _fuse (:321-335) restated in torch ops under the mask, for CPU fp64 autograd: an absent reference's
    logit is -inf, its weight and its gradients exact zeros"""

    @staticmethod
    def apply(q, emb, ass, t, t_major, valid_bits=None):
        n = q.shape[0]
        e = emb.view(t, n, *emb.shape[1:]) if t_major else emb.view(n, t, *emb.shape[1:]).transpose(0, 1)
        a = ass.view(t, n, *ass.shape[1:]) if t_major else ass.view(n, t, *ass.shape[1:]).transpose(0, 1)
        logits = torch.einsum('nchw,tnchw->nthw', q, e)
        if valid_bits is not None:
            valid = ((valid_bits[:, None] >> torch.arange(t, dtype=torch.int32)) & 1).bool()
            logits = logits.masked_fill(~valid[:, :, None, None], float('-inf'))
        return torch.einsum('nthw,tnchw->nchw', torch.softmax(logits, 1), a)


@pytest.mark.parametrize('geom', [(2, 19, 13, 256), (2, 10, 11, 64)], ids=lambda g: 'x'.join(map(str, g)))
def test_masked_fusion_node_matches_fp64_autograd_on_both_engines(geom, monkeypatch):
    """bars of test_fusion_node_at_ragged_sizes_matches_fp64_autograd_of_the_generic_form: 2e-5 of the largest element, 1e-4 for a
    PReLU slope; the reflect-pad recursion of forward_nhwc carries the mask (19 x 13 and 10 x 11 are no multiples of 4)"""
    from mrefsr_amd.archs import nhwc_train
    from mrefsr_amd.archs import ref_mrapa_restoration_arch as arch
    n, h, w, c = geom
    t = 3
    mask = torch.tensor([[1, 0, 1], [0, 1, 0]], dtype=torch.bool)
    absent = [k * n + i for i in range(n) for k in range(t) if not mask[i, k]]          # t-major image index
    torch.manual_seed(h * w + c)
    m = arch.MRAPAFusion(nf=64, ref_nf=c)
    torch.manual_seed(h + w)
    target, refs = torch.randn(n, h, w, 64), torch.randn(t * n, h, w, c)
    gout = torch.randn(n, 64, h, w, dtype=torch.float64)
    engines = {}
    for enabled in (True, False):
        monkeypatch.setattr(nhwc_train, 'ENABLED', enabled)
        mg = copy.deepcopy(m).cuda()
        if enabled:     # the channels-last nodes (masked _Attention)
            tg, rg = target.cuda().requires_grad_(), refs.cuda().requires_grad_()
            out = mg.forward_nhwc(tg, rg, t, ref_valid=mask)
            assert type(out.grad_fn).__name__ == '_CropBackward'
            out.backward(gout.permute(0, 2, 3, 1).float().contiguous().cuda())
            res = [out.permute(0, 3, 1, 2), tg.grad.permute(0, 3, 1, 2), rg.grad.permute(0, 3, 1, 2)]
        else:           # the generic NCHW form (masked _MultiRefAttention)
            tg, rg = target.permute(0, 3, 1, 2).contiguous().cuda().requires_grad_(), refs.permute(0, 3, 1, 2).contiguous().cuda().requires_grad_()
            out = mg.forward_stacked(tg, rg, t, ref_valid=mask.cuda())
            out.backward(gout.float().cuda())
            res = [out, tg.grad, rg.grad]
        engines[enabled] = res + [p.grad for p in mg.parameters()]
    monkeypatch.setattr(arch, '_MultiRefAttention', _Fp64MaskedAttention)
    md = copy.deepcopy(m).double()
    tr = target.permute(0, 3, 1, 2).double().requires_grad_()
    rr = refs.permute(0, 3, 1, 2).double().requires_grad_()
    want = md._fuse(tr, rr, t, t_major=True, ref_valid=mask)
    want.backward(gout)
    assert not rr.grad[absent].any() and rr.grad.abs().max() > 0
    names = ['out', 'd target', 'd refs'] + [k for k, _ in md.named_parameters()]
    wants = [want, tr.grad, rr.grad] + [p.grad for p in md.parameters()]
    for enabled, res in engines.items():
        assert not res[2][absent].any(), 'an absent reference received a gradient'
        for name, got, ref in zip(names, res, wants):
            _close(got, ref, 1e-4 if ref.numel() == 1 else 2e-5, f'engine {"nhwc" if enabled else "generic"} {name}')


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope='module')
def shared(golden):
    model, data, _ = _golden_model(golden('e2e_ragged'), True)     # B = 2, K = 3, LR 45 x 39
    for group in model.optimizer_g.param_groups:
        group['lr'] = 0.0
    return model, data


def _synth_data(b, k, lr_h, lr_w, key):
    samples = [synth.sr_sample(f'{key}/s{i}', k, lr_h, lr_w) for i in range(b)]
    return {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}


def _subset(data, i, keep):
    d = {k: v[i:i + 1].clone() for k, v in data.items()}
    d['img_ref_list'] = d['img_ref_list'][:, keep].contiguous()
    return d


def _masked(data, mask=MASK, filler=None):
    d = {k: v.clone() for k, v in data.items()}
    valid = torch.tensor(mask, dtype=torch.bool)
    if filler is not None:
        d['img_ref_list'][~valid] = filler(d['img_ref_list'][~valid])
    d['ref_valid'] = valid
    return d


def _test(model, data):
    model.feed_data(data)
    model.test()
    model.check_numeric_range()
    return model.output.detach().double().cpu()


def _residual_err(out, ref, lq):
    """max |difference| of the residuals output - bilinear(lq), relative to the largest residual of `ref`"""
    base = F.interpolate(lq.double(), None, 4, 'bilinear', False)
    return float(((out - base) - (ref - base)).abs().max()) / float((ref - base).abs().max())


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.get_bare_model(model.net_g).named_parameters()}


def _step(model, data, deterministic=False):
    model.opt['train']['deterministic'] = deterministic
    try:
        model.feed_data(data)
        model.optimize_parameters(1)
    finally:
        model.opt['train'].pop('deterministic')
    return _grads(model), float(model.get_current_log()['l_g_pix'])


@pytest.mark.parametrize('lr', [(45, 39), (16, 20)], ids=['lr45x39', 'lr16x20'])
def test_masked_batch_restores_each_sample_as_if_fed_alone_with_its_valid_references(shared, lr):
    """B = 2, K = 3, mask [[1,1,1],[0,1,0]].  The bar is 4 x the noise floor of the batch-wide input scales, measured here on the
    unmasked path: a sample run alone against the same sample inside the batch of two with all references valid (same mechanism;
    the factor because K differs as well).  Guard against a vacuous pass: with the mask ignored (absent slots zero images, all
    three attended) sample 1 is off by more than 100 x the bar."""
    model, data = shared
    if lr != (45, 39):
        data = _synth_data(2, 3, *lr, 'refmask')
    lq = data['img_in_lq']
    batch = _test(model, data)
    alone = [_test(model, _subset(data, i, [0, 1, 2])) for i in range(2)]
    floor = max(_residual_err(batch[i:i + 1], alone[i], lq[i:i + 1]) for i in range(2))
    masked = _test(model, _masked(data))
    assert model.ref_valid_bits is not None and model.ref_valid_bits.tolist() == [7, 2]
    subset = [alone[0], _test(model, _subset(data, 1, [1]))]
    errs = [_residual_err(masked[i:i + 1], subset[i], lq[i:i + 1]) for i in range(2)]
    zeroed = _masked(data, filler=torch.zeros_like)
    del zeroed['ref_valid']
    ignored = _residual_err(_test(model, zeroed)[1:2], subset[1], lq[1:2])
    bar = 4 * floor
    print(f'LR {lr}: noise floor (alone vs in an all-valid batch) {floor:.3e}; masked vs valid-subset {errs[0]:.3e} / {errs[1]:.3e} '
          f'(bar {bar:.3e}); mask ignored {ignored:.3e}')
    assert max(errs) <= bar, (errs, bar)
    assert ignored > 100 * bar, (ignored, bar)


def test_result_does_not_depend_on_what_sits_in_an_absent_slot(shared):
    """noise (and NaN) against zeros in the absent slots: equal outputs, and after one optimize_parameters() equal gradients
    (train.deterministic: two runs of one batch agree bit for bit only there)"""
    model, data = shared
    zeros = _masked(data, filler=torch.zeros_like)
    noise = _masked(data, filler=lambda v: torch.rand(v.shape, generator=torch.Generator().manual_seed(5)))
    nans = _masked(data, filler=lambda v: torch.full_like(v, float('nan')))
    out = _test(model, zeros)
    assert torch.isfinite(out).all()
    assert torch.equal(_test(model, noise), out) and torch.equal(_test(model, nans), out)
    g0, l0 = _step(model, zeros, deterministic=True)
    g1, l1 = _step(model, noise, deterministic=True)
    assert l0 == l1 and all(torch.equal(g0[n], g1[n]) for n in g0)


def test_all_true_mask_is_the_unmasked_path(shared, monkeypatch):
    from mrefsr_amd import hip
    model, data = shared
    want = _test(model, data)
    g_want, l_want = _step(model, data, deterministic=True)
    after_masked = _test(model, _masked(data))
    assert model.ref_valid_bits is not None and not torch.equal(after_masked, want)
    assert torch.equal(_test(model, data), want) and model.ref_valid_bits is None     # a batch without the key clears the mask

    def refuse(*a, **k):
        raise AssertionError('a masked kernel was called for an all-true mask')

    for name in ('mrattn_fwd_masked', 'mrattn_bwd_masked', 'mrattn_fwd_nhwc_masked', 'mrattn_bwd_nhwc_masked'):
        monkeypatch.setattr(hip, name, refuse)
    for dtype in (torch.bool, torch.uint8):
        full = dict(data, ref_valid=torch.ones(2, 3, dtype=dtype))
        assert torch.equal(_test(model, full), want) and model.ref_valid_bits is None
    g_full, l_full = _step(model, full, deterministic=True)
    assert l_full == l_want and all(torch.equal(g_full[n], g_want[n]) for n in g_want)


def test_masked_training_step_is_the_mean_of_the_single_sample_subset_steps(shared):
    """B = 2, K = 3, LR 45 x 39, L1 loss: every parameter gradient of the masked batch against (g0 + g1) / 2 of sample 0 stepped
    alone with its three references and sample 1 alone with its one valid reference.  Bars: those
    test_training_step_at_a_ragged_size_on_both_engines holds the two engines to (1e-3 of the largest element, 5e-3 for a 1-D
    parameter).  Under train.deterministic two masked steps give the same bits."""
    model, data = shared
    g, loss = _step(model, _masked(data), deterministic=True)
    again, loss2 = _step(model, _masked(data), deterministic=True)
    assert loss == loss2 and all(torch.equal(g[n], again[n]) for n in g)
    g, loss = _step(model, _masked(data))
    g0, l0 = _step(model, _subset(data, 0, [0, 1, 2]))
    g1, l1 = _step(model, _subset(data, 1, [1]))
    print(f'loss masked {loss:.6f}, mean of the subset steps {(l0 + l1) / 2:.6f}')
    assert abs(loss - (l0 + l1) / 2) <= 1e-4 * abs(loss)
    worst = {1: 0.0, 2: 0.0}
    for n in g:
        want = (g0[n].double() + g1[n].double()) / 2
        err = float((g[n].double() - want).abs().max()) / (float(want.abs().max()) + 1e-30)
        worst[1 if want.dim() == 1 else 2] = max(worst[1 if want.dim() == 1 else 2], err)
        assert err <= (5e-3 if want.dim() == 1 else 1e-3), (n, err)
    print(f'masked step vs mean of subset steps: worst 1-D parameter {worst[1]:.3e}, worst other {worst[2]:.3e} of the largest element')


def test_masked_batch_does_not_take_the_graph_path(shared, monkeypatch):
    model, data = shared
    want = _test(model, _masked(data))
    monkeypatch.setitem(model.opt['val'], 'hip_graph', True)
    model.__dict__.pop('_graphs', None)
    assert model._use_graph()
    got = _test(model, _masked(data))
    assert torch.equal(got, want) and not model.__dict__.get('_graphs')


def test_a_sample_without_a_valid_reference_is_refused_before_any_launch(shared, monkeypatch):
    from mrefsr_amd import _lib
    model, data = shared

    def no_launch(name, *a):
        raise AssertionError(f'{name} called')

    monkeypatch.setattr(_lib, 'call', no_launch)
    with pytest.raises(ValueError, match='no valid reference'):
        model.feed_data(_masked(data, [[1, 1, 1], [0, 0, 0]]))
    with pytest.raises(ValueError):
        model.feed_data(_masked(data, [[1, 1], [0, 1]]))
