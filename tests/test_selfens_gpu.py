"""GPU: test() under val.self_ensemble (the x8 geometric self-ensemble) against an oracle made of torch ops and the unchanged plain
path.

The oracle: for each group tr in (0, 1) the batch-4 B data dict is built with torch (inputs transformed per the torch statement,
images in the order j B + b, img_ref_list [4 B, K, ...], ref_valid repeated), fed to feed_data + test() with the option off, the
outputs inverse-transformed in torch and added as (((((((a0 + a1) + a2) + a3) + b0) + b1) + b2) + b3) * 0.125.  The ensemble pass
launches the same kernels on the same bits in the same batch composition, so model.output must EQUAL the oracle: no tolerance.

Models: two residual blocks, synthetic weights (the set-up of test_optim_train_gpu); every case is a few 4 B passes at LR 16 x 12 or
12 x 12."""
import logging

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

DECAY = 0.999
_MAP = dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'], vgg_type='vgg19')
_TRAIN = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
              scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), total_iter=255000, warmup_iter=-1,
              net_g_pretrain_steps=0, pixel_criterion='L1Loss', pixel_weight=1.0)


def _opt(kind):
    single = kind == 'single'
    opt = dict(
        name='selfens', model_type='RefRestorationModel' if single else 'MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1,
        manual_seed=10, is_train=kind == 'ema', dist=False, rank=0,
        network_g=dict(type='RestorationNet' if single else 'MRAPARestorationNet', ngf=64, n_blocks=2, groups=8), network_map=dict(_MAP),
        network_extractor=dict(type='ContrasExtractorSep' if single else 'ContrasMultiExtractorSep'),
        path=dict(pretrain_network_g=None, pretrain_network_feature_extractor=None, strict_load=True), val=dict(save_img=False))
    if kind == 'ema':
        opt['train'] = dict(_TRAIN, ema_decay=DECAY)
    return opt


def _load_synth(net, seed=0):
    spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec, seed=seed).items()})


_models = {}


def _model(kind):
    """'multi', 'single' (RefRestorationModel) or 'ema' (a training model whose net_g_ema holds weights of its own): built once"""
    if kind not in _models:
        from mrefsr_amd.models import build_model
        torch.manual_seed(10)
        model = build_model(_opt(kind))
        for name in ('net_g', 'net_extractor', 'net_map'):   # (a fresh restoration net has zero offset convolutions)
            _load_synth(model.get_bare_model(getattr(model, name)))
        if kind == 'ema':
            _load_synth(model.net_g_ema, seed=1)
        _models[kind] = model
    model = _models[kind]
    model.opt['val'] = dict(save_img=False)
    model.__dict__.pop('_graphs', None)
    return model


def _data(b, k, lr_h, lr_w, key, single=False, mask=None):
    samples = [synth.sr_sample(f'{key}/s{i}', k, lr_h, lr_w) for i in range(b)]
    d = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    if single:
        d['img_ref'] = d.pop('img_ref_list')[:, 0].contiguous()
    if mask is not None:
        d['ref_valid'] = torch.tensor(mask, dtype=torch.bool)
    return d


CASES = {
    'b2_k2_lr16x12': lambda: ('multi', _data(2, 2, 16, 12, 'selfens/a')),
    'b1_k3_lr12x12': lambda: ('multi', _data(1, 3, 12, 12, 'selfens/b')),
    'masked_b2_k2_lr16x12': lambda: ('multi', _data(2, 2, 16, 12, 'selfens/a', mask=[[1, 1], [1, 0]])),
    'single_ref_b2_lr16x12': lambda: ('single', _data(2, 1, 16, 12, 'selfens/c', single=True)),
    'ema_b2_k2_lr16x12': lambda: ('ema', _data(2, 2, 16, 12, 'selfens/a')),
}


# ------------------------------------------------------------------------------------------------ the oracle
def _copy(t, j, tr):
    if j & 1:
        t = t.flip(-1)
    if j & 2:
        t = t.flip(-2)
    if tr:
        t = t.transpose(-1, -2)
    return t


def _inverse(t, j, tr):
    if tr:
        t = t.transpose(-1, -2)
    if j & 2:
        t = t.flip(-2)
    if j & 1:
        t = t.flip(-1)
    return t


def _group_batch(data, tr):
    """the data dict of batch 4 B of one group, in torch: images in the order j B + b"""
    d = {}
    for name, t in data.items():
        if name == 'ref_valid':
            d[name] = t.repeat(4, 1)
        elif name != 'img_in':   # (the ground truth takes no part in a pass)
            d[name] = torch.cat([_copy(t, j, tr) for j in range(4)]).contiguous()
    return d


def _plain(model, data):
    assert not model.check_self_ensemble(model.opt.get('val'))
    model.feed_data(data)
    model.test()
    model.check_numeric_range()
    return model.output.clone(), model.max_idx.clone()


def _oracle(model, data):
    """-> (the ensemble output, the match indices of the identity copy), by torch and the plain path alone"""
    b = data['img_in_lq'].shape[0]
    outs = []
    for tr in (0, 1):
        batch = _group_batch(data, tr)
        out, idx = _plain(model, batch)
        again, _ = _plain(model, batch)
        assert torch.equal(out, again), 'the plain pass is not reproducible from run to run: nothing below can be judged'
        outs.append(out.view(4, b, *out.shape[1:]))
        if tr == 0:
            k = model.num_refs
            idx0 = idx.view(k, 4, b, *idx.shape[1:])[:, 0].reshape(k * b, *idx.shape[1:])
    acc = _inverse(outs[0][0], 0, 0)
    for j in (1, 2, 3):
        acc = acc + _inverse(outs[0][j], j, 0)
    for j in range(4):
        acc = acc + _inverse(outs[1][j], j, 1)
    return acc * 0.125, idx0


def _ensemble(model, data):
    """feed_data + test() with the option on -> (output, the tensors feed_data left in the model)"""
    model.opt['val']['self_ensemble'] = True
    try:
        model.feed_data(data)
        fed = {n: getattr(model, n) for n in ('img_in_lq', 'match_img_in', 'img_ref_stack', 'ref_valid_bits', 'gt')}
        fed['img_ref_list'] = list(model.img_ref_list)
        if hasattr(model, 'img_ref'):
            fed['img_ref'] = model.img_ref
        model.test()
        model.check_numeric_range()
        return model.output, fed
    finally:
        model.opt['val'].pop('self_ensemble')


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize('case', list(CASES))
def test_ensemble_output_equals_the_batched_oracle(case):
    kind, data = CASES[case]()
    model = _model(kind)
    b, h, w = data['img_in_lq'].shape[0], *data['img_in_lq'].shape[2:]
    oracle, idx0 = _oracle(model, data)
    plain, plain_idx = _plain(model, data)
    assert plain.shape == oracle.shape == (b, 3, 4 * h, 4 * w)
    assert not torch.equal(plain, oracle), 'the ensemble would be indistinguishable from the plain pass: the test shows nothing'
    training = model.net_g.training
    out, fed = _ensemble(model, data)
    assert out.dtype == torch.float32 and out.is_contiguous()
    assert torch.equal(out, oracle)
    # what was fed is back in place: get_current_visuals() and the validation loop see it
    for n, t in fed.items():
        if n == 'img_ref_list':
            assert len(model.img_ref_list) == len(t) and all(x is y for x, y in zip(model.img_ref_list, t))
        else:
            assert getattr(model, n) is t, n
    if 'ref_valid' in data:
        assert model.ref_valid_bits.tolist() == [3, 1]
    assert torch.equal(model.gt.cpu(), data['img_in']) and torch.equal(model.img_in_lq.cpu(), data['img_in_lq'])
    vis = model.get_current_visuals()
    assert vis['img_in_lq'].shape == data['img_in_lq'].shape and torch.equal(vis['rlt'], oracle.cpu())
    # the match indices of the identity copy, in the plain pass's shape
    assert model.max_idx.shape == plain_idx.shape == (model.num_refs * b, h - 2, w - 2)
    assert torch.equal(model.max_idx, idx0)
    assert model.net_g.training == training
    if kind == 'ema':
        assert model.net_g_ema is not None and model.net_g is not model.net_g_ema and not model.net_g_ema.training
    # twice: the same bits
    again, _ = _ensemble(model, data)
    assert torch.equal(again, oracle)


def test_option_absent_or_false_is_the_plain_path(monkeypatch):
    from mrefsr_amd import hip
    kind, data = CASES['b2_k2_lr16x12']()
    model = _model(kind)

    def refuse(*a, **k):
        raise AssertionError('an ensemble kernel was launched with the option off')

    monkeypatch.setattr(hip, 'dihedral_expand', refuse)
    monkeypatch.setattr(hip, 'dihedral_merge', refuse)
    monkeypatch.setattr(type(model), '_test_self_ensemble', refuse)
    want, idx = _plain(model, data)
    for val in (None, {}, dict(save_img=False), dict(self_ensemble=None), dict(self_ensemble=False)):
        model.opt['val'] = val
        out, i = _plain(model, data)
        assert torch.equal(out, want) and torch.equal(i, idx), val
        assert '_graphs' not in model.__dict__


def test_ensemble_passes_do_not_take_the_graph_path(caplog):
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    kind, data = CASES['b1_k3_lr12x12']()
    model = _model(kind)
    oracle, _ = _oracle(model, data)
    model.opt['val']['hip_graph'] = True
    assert model._use_graph()
    MultiRefRestorationModel._self_ensemble_logged = MultiRefRestorationModel._self_ensemble_eager_logged = False
    with caplog.at_level(logging.INFO, logger='basicsr'):
        out, _ = _ensemble(model, data)
        assert torch.equal(out, oracle) and not model.__dict__.get('_graphs')
        out, _ = _ensemble(model, data)
        assert torch.equal(out, oracle) and not model.__dict__.get('_graphs')
    lines = [r.getMessage() for r in caplog.records if r.name == 'basicsr']
    assert sum('self-ensemble' in ln for ln in lines) == 1 and sum('run eagerly' in ln for ln in lines) == 1, lines


@pytest.mark.parametrize('on_device', [False, True], ids=['numpy', 'metrics_on_device'])
def test_validation_scores_the_ensemble_output_cropped_to_the_original_size(on_device):
    """two CUFED-style items (padding: True, an original_size smaller than the 48 x 48 canvas): nondist_validation returns the
    metrics of the ensemble output -- the oracle image -- cropped to original_size"""
    from mrefsr_amd.metrics import calculate_psnr, calculate_ssim, tensor2img
    model = _model('multi')
    items, sizes = [], [(40, 44), (37, 48)]
    for i, size in enumerate(sizes):
        d = _data(1, 3, 12, 12, f'selfens/val{i}')
        items.append(dict(d, padding=True, original_size=list(size), lq_path=[f'img{i}.png']))
    want = dict(psnr=[], psnr_y=[], ssim_y=[])
    for d, (oh, ow) in zip(items, sizes):
        oracle, _ = _oracle(model, {k: v for k, v in d.items() if torch.is_tensor(v)})
        sr, gt = tensor2img(oracle[:1].clone())[:oh, :ow], tensor2img(d['img_in'][:1].clone())[:oh, :ow]
        want['psnr'].append(calculate_psnr(sr, gt, crop_border=4))
        want['psnr_y'].append(calculate_psnr(sr, gt, crop_border=4, test_y_channel=True))
        want['ssim_y'].append(calculate_ssim(sr, gt, crop_border=4, test_y_channel=True))
    model.opt['val'] = dict(save_img=False, self_ensemble=True, metrics_on_device=on_device)
    try:
        res = model.nondist_validation(items, 0, None, False)
    finally:
        model.opt['val'] = dict(save_img=False)
    assert np.isfinite(want['psnr']).all()
    assert res['psnr'] == sum(want['psnr']) / 2
    for name in ('psnr_y', 'ssim_y'):   # (the device metrics agree with numpy to 1e-10: test_metrics_device_gpu)
        assert abs(res[name] - sum(want[name]) / 2) <= (1e-10 if on_device else 0), (name, res[name], want[name])
