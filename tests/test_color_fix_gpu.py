"""GPU: val.color_fix in test() -- the fix is the last step, once, on the final output with match_img_in as the colour source.

The smallest model the self-ensemble and reference-mask tests build (two residual blocks, synthetic weights) at LR 16 x 20, K = 2,
B = 2.  test() with the option must EQUAL hip.color_fix_*(the plain test() output, model.match_img_in): the passes in front of the fix
launch the same kernels on the same bits, so there is no tolerance anywhere below."""
import logging

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

_MAP = dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'], vgg_type='vgg19')
LR_H, LR_W, K, B = 16, 20, 2, 2
FIXES = {'wavelet': 'wavelet', 'adain': 'adain', 'wavelet_levels3': dict(type='wavelet', levels=3)}


def _opt(single, val=None):
    return dict(
        name='colorfix', model_type='RefRestorationModel' if single else 'MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1,
        manual_seed=10, is_train=False, dist=False, rank=0,
        network_g=dict(type='RestorationNet' if single else 'MRAPARestorationNet', ngf=64, n_blocks=2, groups=8), network_map=dict(_MAP),
        network_extractor=dict(type='ContrasExtractorSep' if single else 'ContrasMultiExtractorSep'),
        path=dict(pretrain_network_g=None, pretrain_network_feature_extractor=None, strict_load=True),
        val=dict(save_img=False) if val is None else val)


def _load_synth(net, seed=0):
    spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec, seed=seed).items()})


_models = {}


def _model(single=False):
    """built once per kind with the option off; _with() switches the option the way __init__ reads it"""
    if single not in _models:
        from mrefsr_amd.models import build_model
        torch.manual_seed(10)
        model = build_model(_opt(single))
        for name in ('net_g', 'net_extractor', 'net_map'):   # (a fresh restoration net has zero offset convolutions)
            _load_synth(model.get_bare_model(getattr(model, name)))
        _models[single] = model
    model = _models[single]
    _with(model, dict(save_img=False))
    return model


def _with(model, val):
    from mrefsr_amd.color_fix import parse_color_fix
    model.opt['val'] = val
    model.color_fix_cfg = parse_color_fix(val)
    model.__dict__.pop('_graphs', None)


def _data(single=False, key='colorfix/a', **extra):
    samples = [synth.sr_sample(f'{key}/s{i}', K, LR_H, LR_W) for i in range(B)]
    d = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    if single:
        d['img_ref'] = d.pop('img_ref_list')[:, 0].contiguous()
    d.update(extra)
    return d


def _run(model, data, val):
    _with(model, val)
    model.feed_data(data)
    model.test()
    model.check_numeric_range()
    return model.output.clone()


def _fixed(hip, kind, plain, src, sizes=None):
    spec = FIXES[kind]
    if spec == 'adain':
        return hip.color_fix_adain(plain, src, sizes)
    return hip.color_fix_wavelet(plain, src, sizes, levels=5 if spec == 'wavelet' else spec['levels'])


@pytest.mark.parametrize('kind', list(FIXES))
def test_the_option_is_the_fix_of_the_plain_output(kind, caplog):
    from mrefsr_amd import hip
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    model, data = _model(), _data()
    plain = _run(model, data, dict(save_img=False))
    assert model.valid_sizes is None and plain.shape == (B, 3, 4 * LR_H, 4 * LR_W)
    assert torch.equal(plain, _run(model, data, dict(save_img=False))), 'the plain pass is not reproducible: nothing below can be judged'
    assert torch.equal(model.match_img_in.cpu(), data['img_in_up'])
    want = _fixed(hip, kind, plain, model.match_img_in)
    assert not torch.equal(want, plain), 'the fix would be indistinguishable from the plain output: the test shows nothing'
    MultiRefRestorationModel._color_fix_logged = False
    with caplog.at_level(logging.INFO, logger='basicsr'):
        out = _run(model, data, dict(save_img=False, color_fix=FIXES[kind]))
        assert out.dtype == torch.float32 and torch.equal(out, want)
        assert torch.equal(_run(model, data, dict(save_img=False, color_fix=FIXES[kind])), want)   # twice: the same bits
    assert sum('val.color_fix' in r.getMessage() for r in caplog.records if r.name == 'basicsr') == 1   # logged once
    assert torch.equal(model.get_current_visuals()['rlt'], want.cpu())
    # with the replayed hipGraph in front of it (the fix is not part of the capture)
    out = _run(model, data, dict(save_img=False, hip_graph=True, color_fix=FIXES[kind]))
    assert model.__dict__.get('_graphs') and torch.equal(out, want)
    assert torch.equal(_run(model, data, dict(save_img=False, hip_graph=True, color_fix=FIXES[kind])), want)


@pytest.mark.parametrize('kind', ['wavelet', 'adain'])
def test_under_the_self_ensemble_the_merged_output_is_fixed_once(kind, monkeypatch):
    from mrefsr_amd import hip
    model, data = _model(), _data()
    ens = _run(model, data, dict(save_img=False, self_ensemble=True))
    want = _fixed(hip, kind, ens, model.match_img_in)
    assert not torch.equal(want, ens)
    calls = []
    for name in ('color_fix_wavelet', 'color_fix_adain'):
        fn = getattr(hip, name)
        monkeypatch.setattr(hip, name, lambda x, *a, _fn=fn, **k: (calls.append(tuple(x.shape)), _fn(x, *a, **k))[1])
    out = _run(model, data, dict(save_img=False, self_ensemble=True, color_fix=FIXES[kind]))
    assert torch.equal(out, want)
    assert calls == [(B, 3, 4 * LR_H, 4 * LR_W)], calls   # never on the eight members
    assert torch.equal(model.match_img_in.cpu(), data['img_in_up'])   # the fed tensors are back in place


@pytest.mark.parametrize('kind', ['wavelet', 'adain'])
def test_padded_batches_are_fixed_from_their_own_pixels(kind):
    from mrefsr_amd import hip
    model = _model()
    sizes = [[50, 77], [64, 41]]
    data = _data(padding=True, original_size=[torch.tensor([50, 64]), torch.tensor([77, 41])])
    plain = _run(model, data, dict(save_img=False))
    assert model.valid_sizes == sizes
    out = _run(model, data, dict(save_img=False, color_fix=FIXES[kind]))
    assert torch.equal(out, _fixed(hip, kind, plain, model.match_img_in, sizes))
    for b, (h, w) in enumerate(sizes):
        outside = torch.ones(plain.shape[2:], dtype=torch.bool, device=plain.device)
        outside[:h, :w] = False
        assert torch.equal(out[b][:, outside].view(torch.int32), plain[b][:, outside].view(torch.int32))
        assert not torch.equal(out[b, :, :h, :w], plain[b, :, :h, :w])
    # the same size for every sample, as a plain (h, w)
    out = _run(model, dict(data, original_size=(50, 77)), dict(save_img=False, color_fix=FIXES[kind]))
    assert model.valid_sizes == [[50, 77], [50, 77]]
    assert torch.equal(out, _fixed(hip, kind, plain, model.match_img_in, [(50, 77)] * B))
    model.feed_data(_data())
    assert model.valid_sizes is None


def test_without_the_option_nothing_is_launched_and_the_output_keeps_its_bits(monkeypatch):
    from mrefsr_amd import hip
    from mrefsr_amd.models import build_model
    model, data = _model(), _data()
    want = _run(model, data, dict(save_img=False))

    def refuse(*a, **k):
        raise AssertionError('a colour-fix kernel was launched with the option off')

    monkeypatch.setattr(hip, 'color_fix_wavelet', refuse)
    monkeypatch.setattr(hip, 'color_fix_adain', refuse)
    for val in (None, {}, dict(save_img=False), dict(color_fix=None), dict(color_fix=False)):
        assert torch.equal(_run(model, data, val), want), val
        assert model.valid_sizes is None
    # a model BUILT without the option, against one built with it
    monkeypatch.undo()
    torch.manual_seed(10)
    built = build_model(_opt(False, val=dict(save_img=False, color_fix=dict(type='wavelet', levels=2))))
    assert built.color_fix_cfg == dict(type='wavelet', levels=2)
    for name in ('net_g', 'net_extractor', 'net_map'):
        _load_synth(built.get_bare_model(getattr(built, name)))
    built.feed_data(data)
    built.test()
    assert torch.equal(built.output, hip.color_fix_wavelet(want, built.match_img_in, levels=2))


@pytest.mark.parametrize('kind', ['wavelet', 'adain'])
def test_the_single_reference_model_takes_the_option(kind):
    from mrefsr_amd import hip
    model, data = _model(single=True), _data(single=True, padding=True, original_size=(60, 80))
    plain = _run(model, data, dict(save_img=False))
    assert model.valid_sizes == [[60, 80], [60, 80]]
    out = _run(model, data, dict(save_img=False, color_fix=FIXES[kind]))
    want = _fixed(hip, kind, plain, model.match_img_in, model.valid_sizes)
    assert torch.equal(out, want) and not torch.equal(out, plain)
    assert torch.equal(out[:, :, 60:], plain[:, :, 60:])
