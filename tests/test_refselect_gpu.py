"""GPU: reference pools (the ref_select option) at model level, against the same pipeline composed in the test.

The composed pipeline: net_extractor.forward_stacked on the whole pool, match_normalised_batch(..., want_val=True), the scores in
fp64 and the choice and the gathers in torch (the statement of DESIGN 3.14, shared with test_refselect_kernels_gpu), then
hip.offsets_from_idx, net_map.vgg and net_g on the gathered K-reference batch.  The model launches the same kernels on the same bits
in the same batch composition -- only the scoring, the choice and the gathers are its own kernels -- so outputs, losses and
gradients must EQUAL the composed ones: no tolerance.  The choice itself is compared under an asserted precondition: the K-th and
the (K+1)-th fp64 score of every sample differ by more than 1e-4 relative, far above the fp32 sum's error.

Pools: some candidates are synth.sr_sample's references of the sample's own key (rolled copies of its ground truth, noise added),
the others those of an unrelated key.  With synth weights the extractor's features correlate weakly (mean winning correlations of
+-0.02) and prefer neither kind; the mixtures below were kept because they separate the K-th from the (K+1)-th score by 28 % and more
(mean) and by whole win counts (wins) on an MI355X, and because the choice is not the first K candidates.  Models: two residual blocks, synth weights, LR 16 x 12 and 12 x 12, B <= 2."""
import logging

import numpy as np
import pytest
import torch

import synth
from test_refselect_kernels_gpu import _oracle

pytestmark = pytest.mark.gpu

_MAP = dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'], vgg_type='vgg19')
_TRAIN = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
              scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), total_iter=255000, warmup_iter=-1,
              net_g_pretrain_steps=0, pixel_criterion='L1Loss', pixel_weight=1.0, deterministic=True)


def _opt(kind):
    opt = dict(
        name='refselect', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, manual_seed=10, is_train=kind in ('l1', 'texture'),
        dist=False, rank=0, network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=2, groups=8), network_map=dict(_MAP),
        network_extractor=dict(type='ContrasMultiExtractorSep'),
        path=dict(pretrain_network_g=None, pretrain_network_feature_extractor=None, strict_load=True), val=dict(save_img=False))
    if kind != 'plain':
        opt['ref_select'] = dict(top_k=2)
    if kind == 'l1':
        opt['train'] = dict(_TRAIN)
    if kind == 'texture':
        opt['train'] = dict(_TRAIN, texture_opt=dict(use_weights=True, loss_weight=1.0))
    return opt


def _load_synth(net, seed=0):
    spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec, seed=seed).items()})


_models = {}


def _model(kind, score='mean'):
    """'pool' (inference, ref_select top_k 2), 'plain' (inference, no option), 'l1' / 'texture' (training, ref_select): built once"""
    if kind not in _models:
        from mrefsr_amd.models import build_model
        torch.manual_seed(10)
        model = build_model(_opt(kind))
        for name in ('net_g', 'net_extractor', 'net_map'):   # (a fresh restoration net has zero offset convolutions)
            _load_synth(model.get_bare_model(getattr(model, name)))
        if kind == 'texture':
            _load_synth(model.cri_texture)
        _models[kind] = model
    model = _models[kind]
    model.opt['val'] = dict(save_img=False)
    model.__dict__.pop('_graphs', None)
    if kind != 'plain':
        assert model.ref_select[0] == 2
        model.ref_select = (2, score)
    else:
        assert model.ref_select is None
    return model


# which candidates of a pool come from the sample's own key ('s') and which from an unrelated one ('u'), per sample
POOLS = {4: ['ussu', 'suus'], 3: ['sus'], 2: ['ss', 'ss']}


def _data(b, n, lr_h, lr_w, key, mask=None):
    samples = []
    for i in range(b):
        own, other = synth.sr_sample(f'{key}/s{i}', n, lr_h, lr_w), synth.sr_sample(f'{key}/unrelated{i}', n, lr_h, lr_w)
        refs = np.stack([(own if c == 's' else other)['img_ref_list'][j] for j, c in enumerate(POOLS[n][i])])
        samples.append(dict(own, img_ref_list=refs))
    d = {name: torch.from_numpy(np.stack([s[name] for s in samples])) for name in samples[0]}
    if mask is not None:
        d['ref_valid'] = torch.tensor(mask, dtype=torch.bool)
    return d


# ------------------------------------------------------------------------------------------------ the composed pipeline
def _rows(t, sel, n):
    """torch indexing: [n*B, ...] candidate-major -> [K*B, ...] slot-major by sel [B,K], zeros for -1"""
    b, k = sel.shape
    src = t.view(n, b, *t.shape[1:])
    out = torch.zeros((k, b, *t.shape[1:]), dtype=t.dtype, device=t.device)
    for i in range(b):
        for j in range(k):
            if sel[i, j] >= 0:
                out[j, i] = src[sel[i, j], i]
    return out.view(k * b, *t.shape[1:])


def _choose(model, data, k, score):
    """extractor and matcher on the pool, the scores and the choice in torch -> dict(sel [B,k] (CPU), scores fp32 [B,N], bits: the
    K-slot words on the device or None, pool, idx, val, hw); ASSERTS the score gap between the k-th and the (k+1)-th candidate"""
    from mrefsr_amd import hip
    from mrefsr_amd.archs.ref_map_util import match_normalised_batch
    dev = model.device
    refs = data['img_ref_list'].to(dev)
    b, n = refs.shape[:2]
    valid = data['ref_valid'] if 'ref_valid' in data else torch.ones(b, n, dtype=torch.bool)
    refs = torch.where(valid.to(dev)[:, :, None, None, None], refs, refs.new_zeros(()))
    pool = refs.transpose(0, 1).reshape(-1, *refs.shape[2:]).contiguous()
    hip.amax_pool_reset()
    with torch.no_grad():
        f1, f2 = model.net_extractor.forward_stacked(data['img_in_up'].to(dev), pool)
        idx, val = match_normalised_batch(f1, f2, want_val=True)
    v = val.view(n, b, -1).cpu()
    scores, sel, words = _oracle(v, valid, k, score)
    s64 = (v.double().sum(dim=2) / v.shape[2]).t() if score == 'mean' else scores.double()
    for i in range(b):
        ranked = sorted((float(s64[i, j]) for j in range(n) if valid[i, j]), reverse=True)
        print(f'{score} scores of sample {i}: {[float(x) for x in s64[i]]}')
        if len(ranked) > k:
            gap = abs(ranked[k - 1] - ranked[k]) / max(abs(ranked[k - 1]), abs(ranked[k]))
            assert gap > 1e-4, f'sample {i}: the scores {ranked} do not separate candidate {k} from candidate {k + 1}'
    bits = None if all(w == (1 << k) - 1 for w in words) else torch.tensor(words, dtype=torch.int32, device=dev)
    return dict(sel=sel, scores=scores, bits=bits, pool=pool, idx=idx, val=val, hw=tuple(f1.shape[2:]), n=n)


def _composed_forward(model, data, ch):
    """offsets, VGG19 maps and net_g on the torch-gathered batch; leaves what the losses read in the model"""
    from mrefsr_amd import hip
    k, (h, w) = ch['sel'].shape[1], ch['hw']
    with torch.no_grad():
        idx, val, refs = (_rows(t, ch['sel'], ch['n']) for t in (ch['idx'], ch['val'], ch['pool']))
        offs = hip.offsets_from_idx(idx.contiguous(), h, w)
        pre_offset = {'relu3_1': offs[1], 'relu2_1': offs[2], 'relu1_1': offs[4]}
        feat = model.net_map.vgg(refs)
    lq = data['img_in_lq'].to(model.device)
    if ch['bits'] is not None:
        out = model.net_g(lq, pre_offset, feat, k=k, ref_valid=ch['bits'])
    else:
        out = model.net_g(lq, pre_offset, feat, k=k)
    model.max_idx, model.max_val, model.img_ref_feat, model.num_refs, model.ref_valid_bits = idx, val, feat, k, ch['bits']
    return out


def _composed_test(model, data, k, score):
    ch = _choose(model, data, k, score)
    training = model.net_g.training
    model.net_g.eval()
    with torch.no_grad():
        out = _composed_forward(model, data, ch)
    model.net_g.train(training)
    model.check_numeric_range()
    return out.clone(), ch


def _run_test(model, data):
    model.feed_data(data)
    model.test()
    model.check_numeric_range()
    return model.output


def _check_choice(model, ch, b, n, k):
    assert model.ref_selection.dtype == torch.int32 and tuple(model.ref_selection.shape) == (b, k)
    assert torch.equal(model.ref_selection.cpu(), ch['sel']), (model.ref_selection.tolist(), ch['sel'].tolist())
    assert model.ref_scores.dtype == torch.float32 and tuple(model.ref_scores.shape) == (b, n)
    got, want = model.ref_scores.cpu().double(), ch['scores'].double()
    finite = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), finite) and torch.equal(got[~finite], want[~finite])
    assert ((got[finite] - want[finite]).abs() <= 1e-6 * want[finite].abs()).all(), (got, want)
    assert model.num_refs == k and model.max_idx.shape[0] == k * b and model.img_ref_stack.shape[0] == k * b


# ------------------------------------------------------------------------------------------------ test()
@pytest.mark.parametrize('score', ['mean', 'wins'])
def test_pool_of_four_equals_the_composed_pipeline(score):
    model = _model('pool', score)
    data = _data(2, 4, 16, 12, 'refselect/a')
    want, ch = _composed_test(model, data, 2, score)
    # (with synth weights the matcher prefers no key; what counts is that the choice is not simply the first two candidates)
    assert ch['bits'] is None and (ch['sel'] >= 0).all() and any(row != [0, 1] for row in ch['sel'].tolist())
    out = _run_test(model, data)
    assert out.shape == (2, 3, 64, 48) and torch.equal(out, want)
    _check_choice(model, ch, 2, 4, 2)
    assert model.ref_valid_bits is None
    assert torch.equal(model.max_idx, _rows(ch['idx'], ch['sel'], 4))
    assert torch.equal(model.img_ref_stack, _rows(ch['pool'], ch['sel'], 4))
    vis = model.get_current_visuals()
    assert sorted(vis) == ['gt', 'img_in_lq', 'rlt'] and torch.equal(vis['rlt'], want.cpu())
    # the pool survives the pass: the next test() selects again, the same bits
    assert model.ref_pool is not None and model.ref_pool['n'] == 4
    model.test()
    assert torch.equal(model.output, want)
    # the restored image does depend on the choice: the plain pass over the first two candidates differs
    plain = _run_test(_model('plain'), dict(data, img_ref_list=data['img_ref_list'][:, :2].contiguous()))
    assert not torch.equal(plain, want)


@pytest.mark.parametrize('score', ['mean', 'wins'])
def test_fewer_valid_candidates_than_k_runs_with_the_slot_mask(score):
    model = _model('pool', score)
    data = _data(2, 4, 16, 12, 'refselect/a', mask=[[1, 1, 1, 1], [0, 0, 1, 0]])
    want, ch = _composed_test(model, data, 2, score)
    assert ch['sel'][1].tolist() == [2, -1] and (ch['sel'][0] >= 0).all() and ch['bits'].tolist() == [3, 1]
    out = _run_test(model, data)
    assert torch.equal(out, want)
    _check_choice(model, ch, 2, 4, 2)
    assert model.ref_valid_bits.tolist() == [3, 1] and not model.img_ref_stack.view(2, 2, -1)[1, 1].any()
    assert torch.isinf(model.ref_scores[1, [0, 1, 3]]).all()


def test_pool_no_larger_than_top_k_is_the_plain_path(monkeypatch):
    from mrefsr_amd import hip
    data = _data(2, 2, 16, 12, 'refselect/b')
    masked = dict(data, ref_valid=torch.tensor([[1, 1], [0, 1]], dtype=torch.bool))
    plain = _model('plain')
    want, want_masked = _run_test(plain, data).clone(), _run_test(plain, masked).clone()
    model = _model('pool')

    def refuse(*a, **k):
        raise AssertionError('a selection kernel was launched for a pool no larger than top_k')

    monkeypatch.setattr(hip, 'ref_select', refuse)
    monkeypatch.setattr(hip, 'ref_gather', refuse)
    out = _run_test(model, data)
    assert torch.equal(out, want) and model.ref_selection is None and model.ref_scores is None and model.ref_pool is None
    out = _run_test(model, masked)
    assert torch.equal(out, want_masked) and model.ref_selection is None and model.ref_valid_bits.tolist() == [3, 2]


def test_self_ensemble_runs_on_the_selected_batch():
    model, plain = _model('pool'), _model('plain')
    data = _data(1, 3, 12, 12, 'refselect/c')
    ch = _choose(model, data, 2, 'mean')
    assert ch['sel'].tolist() != [[0, 1]]
    gathered = _rows(ch['pool'], ch['sel'], 3)                                  # [K*B,3,H,W] -> img_ref_list [B,K,3,H,W]
    two = dict(data, img_ref_list=gathered.view(2, 1, *gathered.shape[1:]).transpose(0, 1).contiguous().cpu())
    plain.opt['val'] = dict(save_img=False, self_ensemble=True)
    model.opt['val'] = dict(save_img=False, self_ensemble=True)
    try:
        want = _run_test(plain, two).clone()
        want_idx = plain.max_idx.clone()
        out = _run_test(model, data)
        assert torch.equal(out, want) and torch.equal(model.max_idx, want_idx)
        _check_choice(model, ch, 1, 3, 2)
        assert model.ref_pool is not None and model.ref_pool['n'] == 3
        model.test()
        assert torch.equal(model.output, want)
    finally:
        plain.opt['val'] = dict(save_img=False)
        model.opt['val'] = dict(save_img=False)
    single = _run_test(model, data)
    assert not torch.equal(single, want)


def test_pool_batches_do_not_take_the_graph_path(caplog):
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    model = _model('pool')
    data = _data(2, 4, 16, 12, 'refselect/a')
    want = _run_test(model, data).clone()
    model.opt['val']['hip_graph'] = True
    assert model._use_graph()
    MultiRefRestorationModel._pool_eager_logged = False
    with caplog.at_level(logging.INFO, logger='basicsr'):
        for _ in range(2):
            assert torch.equal(_run_test(model, data), want) and not model.__dict__.get('_graphs')
    lines = [r.getMessage() for r in caplog.records if r.name == 'basicsr']
    assert sum('reference pool' in ln and 'run eagerly' in ln for ln in lines) == 1, lines


# ------------------------------------------------------------------------------------------------ optimize_parameters
def _composed_step(model, data, k, score):
    """one step's forward and backward by the composed pipeline, without the update -> (log, gradients)"""
    from mrefsr_amd import hip
    from mrefsr_amd.archs import nhwc_train
    ch = _choose(model, data, k, score)
    model.gt = data['img_in'].to(model.device)
    with hip.deterministic(True):
        nhwc_train.check_scales()
        model.optimizer_g.zero_grad()
        nhwc_train.begin_step()
        model.output = _composed_forward(model, data, ch)
        assert model._loss_and_backward(1)
    model.check_numeric_range()
    log = {n: v.clone() for n, v in model.log_dict.items()}
    grads = {n: p.grad.detach().clone() for n, p in model.get_bare_model(model.net_g).named_parameters()}
    return ch, log, model.output.detach().clone(), grads


@pytest.mark.parametrize('kind', ['l1', 'texture'])
def test_training_step_equals_the_composed_step(kind):
    model = _model(kind)
    data = _data(2, 4, 16, 12, 'refselect/a')
    ch, log, out, grads = _composed_step(model, data, 2, 'mean')
    assert set(log) == ({'l_g_pix'} if kind == 'l1' else {'l_g_pix', 'l_g_texture'})
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and any(float(g.abs().max()) > 0 for g in grads.values())
    model.log_dict.clear()
    model.feed_data(data)
    model.optimize_parameters(1)
    assert model.range_fallbacks == 0
    assert torch.equal(model.output.detach(), out)
    for n in log:
        assert torch.equal(model.log_dict[n], log[n]), (n, model.log_dict[n], log[n])
    for n, p in model.get_bare_model(model.net_g).named_parameters():
        assert torch.equal(p.grad, grads[n]), n
    _check_choice(model, ch, 2, 4, 2)
    if kind == 'texture':   # _texture_targets saw the K gathered references: maps of K*B rows, indices and values of K*B rows
        assert model.max_val.shape == model.max_idx.shape == (4, 14, 10)
        assert all(v.shape[0] == 4 for v in model.img_ref_feat.values())
        assert torch.equal(model.max_val, _rows(ch['val'], ch['sel'], 4))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from mrefsr_amd.models import build_model
    model = _model('pool')
    data = _data(1, 3, 12, 12, 'refselect/c')
    big = dict(data, img_ref_list=torch.zeros(1, 33, 3, 48, 48))
    with pytest.raises(ValueError, match='33'):   # (refused on the host, before anything is copied or launched)
        model.feed_data(big)
    with pytest.raises(ValueError):   # a sample without a present candidate
        model.feed_data(dict(data, ref_valid=torch.tensor([[0, 0, 0]], dtype=torch.bool)))
    with pytest.raises(ValueError):   # a mask of the wrong width
        model.feed_data(dict(data, ref_valid=torch.ones(1, 4, dtype=torch.bool)))
    opt = _opt('pool')
    opt.update(model_type='RefRestorationModel', network_g=dict(type='RestorationNet', ngf=64, n_blocks=2, groups=8),
               network_extractor=dict(type='ContrasExtractorSep'))
    with pytest.raises(ValueError, match='ref_select'):
        build_model(opt)
    bad = _opt('pool')
    bad['ref_select'] = dict(top_k=17)
    with pytest.raises(ValueError, match='16'):
        build_model(bad)
