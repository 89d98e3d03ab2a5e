"""GPU: train.ref_augment, val.ref_perturb and val.match_probe in the models -- the two-block model of the other model-level tests
with tests/golden/synth.py weights at B = 1, K = 2, LR 16 x 20 -> 64 x 80.

The probe with a known answer: with the LR stack's weights copied into the reference stack and the view an integer translation of
match_img_in itself ((x, y) -> (x - 4, y + 8): one conv3_1 cell right, two up), the true match of every counted query is the same
content, up to the zero border the view brings into the receptive field.  oracle/pipeline.py on the synth weights (CPU, fp32) was
asked before relying on it: at margin 2 it finds 20 wrong matches of 104 for this test's image (6 of 104 for another), at margin 3
none of 66 for either -- so the zero is asserted at margin 3, the smallest margin at which the oracle gives it, and at margin 2 the
count alone."""
import numpy as np
import pytest
import torch

import synth
from mrefsr_amd import views

pytestmark = pytest.mark.gpu

_MAP = dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'], vgg_type='vgg19')
LR_H, LR_W, K, B = 16, 20, 2, 1
H, W = 4 * LR_H, 4 * LR_W
SEED = 10
TRAIN = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
             scheduler=dict(type='MultiStepLR', milestones=[300000], gamma=0.5), total_iter=255000, warmup_iter=-1,
             net_g_pretrain_steps=0, pixel_criterion='L1Loss', pixel_weight=1.0)
SHIFT = [[1.0, 0.0, -4.0], [0.0, 1.0, 8.0], [0.0, 0.0, 1.0]]   # the sampling matrix of (x, y) -> (x - 4, y + 8)


def _opt(is_train, single=False, train=None, val=None):
    return dict(
        name='refviews', model_type='RefRestorationModel' if single else 'MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1,
        manual_seed=SEED, is_train=is_train, dist=False, rank=0,
        network_g=dict(type='RestorationNet' if single else 'MRAPARestorationNet', ngf=64, n_blocks=2, groups=8), network_map=dict(_MAP),
        network_extractor=dict(type='ContrasExtractorSep' if single else 'ContrasMultiExtractorSep'),
        path=dict(pretrain_network_g=None, pretrain_network_feature_extractor=None, strict_load=True),
        train=dict(TRAIN, **(train or {})), val=dict(save_img=False, **(val or {})))


def _build(is_train, single=False, train=None, val=None):
    from mrefsr_amd.models import build_model
    torch.manual_seed(SEED)
    model = build_model(_opt(is_train, single, train, val))
    for name in ('net_g', 'net_extractor', 'net_map'):   # (a fresh restoration net has zero offset convolutions)
        net = model.get_bare_model(getattr(model, name))
        spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()})
    return model


_tester = {}


def _test_model(val=None, single=False):
    """the model that is not training, built once per kind; the options switched the way __init__ reads them"""
    if single not in _tester:
        _tester[single] = _build(False, single)
    model = _tester[single]
    model.opt['val'] = dict(save_img=False, **(val or {}))
    model._setup_ref_views(model.opt)
    return model


def _data(key='refviews/a', single=False, **extra):
    s = synth.sr_sample(f'{key}/s0', K, LR_H, LR_W)
    d = {n: torch.from_numpy(v[None]) for n, v in s.items()}
    if single:
        d['img_ref'] = d.pop('img_ref_list')[:, 0].contiguous()
    d.update(extra)
    return d


def _stack(data):
    """the k-major stack feed_data builds, absent references zeroed"""
    refs = data['img_ref_list'].clone()
    if data.get('ref_valid') is not None:
        refs[~data['ref_valid'].bool()] = 0
    return refs.transpose(0, 1).reshape(-1, *refs.shape[2:]).contiguous()


def _tested(model, data):
    model.feed_data(data)
    model.test()
    model.check_numeric_range()
    return model.output.clone()


def _step(model, data, it=1):
    model.feed_data(data)
    model.optimize_parameters(it)
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.get_bare_model(model.net_g).named_parameters() if p.grad is not None}
    return model.get_current_log(), grads


def _kernels(fn):
    """fn's value and the names of the kernels it launched, in order.  The runtime's own copies and fills (Memcpy..., Memset...) are
    left out: how many device-to-device copies a step makes follows the allocator's state (seen: seven more in one of two like runs)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = [e.name.replace(' ', '') for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return out, [n for n in names if not n.startswith(('Memcpy', 'Memset'))]


# ------------------------------------------------------------------ the options absent
def _gone(*a, **kw):
    raise AssertionError('a view was made with its option absent')


_NEW_PATHS = (('hip', 'warp_perspective'), ('hip', 'match_stats'), ('views', 'sample_ref_augment'), ('views', 'sample_corner_homographies'),
              ('views', 'similarity'))


def _without_the_new_paths(monkeypatch):
    import mrefsr_amd
    for mod, name in _NEW_PATHS:
        monkeypatch.setattr(getattr(mrefsr_amd, mod), name, _gone)


def _diff(a, b):
    import difflib
    return '\n'.join(line for line in difflib.unified_diff(a, b, lineterm='', n=1))[:4000]


def test_without_the_options_the_step_launches_what_it_launched(monkeypatch):
    """the second training step of a fresh model has the same kernel list while the new bindings and the samplers raise, and none of
    the new kernels is in it.  (The step's bits: the p: 0 test below.)  The traces follow test_r1_train_gpu.py's test of the same
    kind: each starts from the same process-wide state of nhwc_train, its cache of weight scales emptied and its count of range
    checks at 0; one run in front of them leaves the rest of the process's state (what earlier models left behind) settled."""
    from mrefsr_amd.archs import nhwc_train
    data = _data()

    def traced():
        nhwc_train.reset_scales()
        monkeypatch.setattr(nhwc_train._scales, 'checks', 0)
        model = _build(True, train=dict(deterministic=True))
        assert model.ref_augment is None and model.ref_perturb_cfg is None and model.match_probe_cfg is None and model._ref_aug_gen is None
        _step(model, data, 1)
        return model, _kernels(lambda: _step(model, data, 2))[1]
    traced()
    model, names = traced()
    assert len(names) > 100 and not [n for n in names if 'warp_persp' in n or 'match_stats' in n]
    _without_the_new_paths(monkeypatch)
    without = traced()[1]
    assert names == without, _diff(names, without)
    monkeypatch.undo()
    # (the names do show with the options on)
    model.opt['train']['ref_augment'] = dict(p=1, perturb=[3, 12])
    model.opt['val'] = dict(save_img=False, match_probe=dict(perturb=[3, 12]))
    model._setup_ref_views(model.opt)
    _, on = _kernels(lambda: (model.feed_data(data), model.match_probe()))
    assert sum('warp_persp' in n for n in on) == 2 and sum('match_stats' in n for n in on) == 1


def test_without_the_options_test_launches_what_it_launched_and_keeps_its_bits(monkeypatch):
    data = _data()
    model = _test_model()
    assert model.ref_augment is None and model.ref_perturb_cfg is None and model.match_probe_cfg is None
    for _ in range(2):   # (the second pass still builds tables over what the first one packed)
        _tested(model, data)
    out, names = _kernels(lambda: _tested(model, data))
    assert len(names) > 50 and not [n for n in names if 'warp_persp' in n or 'match_stats' in n]
    _without_the_new_paths(monkeypatch)
    for val in (None, {}, dict(ref_perturb=None, match_probe=False)):
        model.opt['val'] = val
        model._setup_ref_views(model.opt)
        out2, without = _kernels(lambda: _tested(model, data))
        assert names == without, _diff(names, without)
        assert torch.equal(out2.view(torch.int32), out.view(torch.int32))


# ------------------------------------------------------------------ train.ref_augment
def test_ref_augment_p0_gives_the_plain_steps_bits():
    data = _data()
    plain_log, plain = _step(_build(True, train=dict(deterministic=True)), data)
    model = _build(True, train=dict(deterministic=True, ref_augment=dict(p=0)))
    assert model.ref_augment == dict(p=0.0, perturb=(5, 20), window=None, interp='bicubic') and model._ref_aug_gen is not None
    log, grads = _step(model, data)
    assert 'l_g_pix' in log and log == plain_log, (log, plain_log)
    assert sorted(grads) == sorted(plain) and len(grads) > 20
    for n in grads:
        assert torch.equal(grads[n], plain[n]), n


def test_ref_augment_p1_feeds_the_views_drawn_from_the_seed_and_leaves_validation_alone(monkeypatch):
    from mrefsr_amd import hip
    cfg = dict(p=1, perturb=[3, 12], interp='bicubic')
    model = _build(True, train=dict(ref_augment=cfg))
    data = _data(ref_valid=torch.tensor([[True, False]]))
    calls, real = [], hip.warp_perspective
    monkeypatch.setattr(hip, 'warp_perspective', lambda x, *a, **k: (calls.append(tuple(x.shape)), real(x, *a, **k))[1])
    model.feed_data(data)
    assert calls == [(K * B, 3, H, W)]   # one launch for the batch
    fed = _stack(data).cuda()
    gen = torch.Generator().manual_seed(SEED)   # (the model's generator: seeded from manual_seed, as _d_aug_gen is)
    sampling = views.sample_ref_augment(K * B, H, W, views.parse_ref_augment(dict(ref_augment=cfg)), gen)
    assert sampling is not None and not torch.equal(sampling[0], torch.eye(3, dtype=torch.float64))
    want = real(fed, sampling, interp='bicubic', clamp=True)
    assert torch.equal(model.img_ref_stack.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(model.img_ref_stack[0], fed[0])
    assert torch.equal(model.img_ref_stack[1].view(torch.int32), torch.zeros_like(fed[1]).view(torch.int32))   # the absent slot stays zero
    assert torch.equal(model.img_ref_list[0], model.img_ref_stack[:B])
    assert float(model.img_ref_stack.min()) >= 0 and float(model.img_ref_stack.max()) <= 1
    # the input, the GT and img_in_up are untouched
    for name, key in (('img_in_lq', 'img_in_lq'), ('gt', 'img_in'), ('match_img_in', 'img_in_up')):
        assert torch.equal(getattr(model, name).cpu(), data[key]), name
    model.optimize_parameters(1)
    assert np.isfinite(model.get_current_log()['l_g_pix'])
    # validation right after a training step: not augmented; the next training batch is again
    del calls[:]
    plain = dict(_data('refviews/v'), lq_path=['v0.png'])
    result = model.validation([plain], 1, None)
    assert calls == [] and np.isfinite(result['psnr'])
    assert torch.equal(model.img_ref_stack.cpu(), _stack(plain))
    assert model._validating is False
    model.feed_data(data)
    assert len(calls) == 1 and not torch.equal(model.img_ref_stack, want)   # (fresh draws)


def test_ref_augment_acts_on_the_pool_stack_under_ref_select():
    from mrefsr_amd import hip
    from mrefsr_amd.models import build_model
    cfg = dict(p=1, perturb=[3, 12])
    torch.manual_seed(SEED)
    model = build_model(dict(_opt(True, train=dict(ref_augment=cfg)), ref_select=dict(top_k=1)))
    data = _data()
    model.feed_data(data)
    gen = torch.Generator().manual_seed(SEED)
    sampling = views.sample_ref_augment(K * B, H, W, views.parse_ref_augment(dict(ref_augment=cfg)), gen)
    want = hip.warp_perspective(_stack(data).cuda(), sampling, clamp=True)
    assert model.ref_pool is not None and torch.equal(model.ref_pool['stack'], want)


# ------------------------------------------------------------------ val.ref_perturb
def test_ref_perturb_by_the_identity_returns_the_plain_outputs_bits():
    data = _data()
    plain = _tested(_test_model(), data)
    assert torch.equal(plain, _tested(_test_model(), data)), 'the plain pass is not reproducible: nothing below can be judged'
    model = _test_model(dict(ref_perturb=dict(scale=1, rotate=0)))
    assert model.ref_perturb_cfg['kind'] == 'similarity'
    out = _tested(model, data)
    assert torch.equal(model.img_ref_stack.cpu().view(torch.int32), _stack(data).view(torch.int32))
    assert torch.equal(out.view(torch.int32), plain.view(torch.int32))
    # and a real perturbation changes the output
    assert not torch.equal(_tested(_test_model(dict(ref_perturb=dict(scale=1.25, rotate=10))), data), plain)


@pytest.mark.parametrize('single', [False, True])
def test_ref_perturb_by_180_degrees_feeds_the_double_flip(single):
    data = _data(single=single)
    model = _test_model(dict(ref_perturb=dict(scale=1, rotate=180)), single=single)
    model.feed_data(data)
    fed = data['img_ref'] if single else _stack(data)
    assert torch.equal(model.img_ref_stack.cpu().view(torch.int32), fed.flip(-1, -2).contiguous().view(torch.int32))
    model.test()
    model.check_numeric_range()
    assert bool(torch.isfinite(model.output).all())


def test_ref_perturb_by_corners_depends_on_seed_and_image_index_only():
    from mrefsr_amd import hip
    val = dict(ref_perturb=dict(perturb=[3, 12], seed=4))
    model = _test_model(val)
    batches = [dict(_data(f'refviews/c{i}'), lq_path=[f'c{i}.png']) for i in range(2)]
    fed = []
    feed = model.feed_data
    model.feed_data = lambda d: (feed(d), fed.append(model.img_ref_stack.clone()))[0]
    try:
        model.validation(batches, 0, None)
    finally:
        del model.feed_data
    assert len(fed) == 2
    for i, d in enumerate(batches):
        s = views.indexed_corner_homographies(4, i, K, H, W, (3, 12))   # reference k of image i: the k-th matrix of (seed, i)
        assert torch.equal(fed[i], hip.warp_perspective(_stack(d).cuda(), s, clamp=True)), i
    # B = 2: image b of the batch takes the matrices of (seed, base + b); entry k * B + b of the k-major stack is its k-th
    two = {n: torch.cat([batches[0][n], batches[1][n]]) for n in ('img_in_lq', 'img_in_up', 'img_ref_list', 'img_in')}
    model.feed_data(two)
    per_image = [views.indexed_corner_homographies(4, b, K, H, W, (3, 12)) for b in range(2)]
    fed2 = _stack(two).cuda()
    assert fed2.shape[0] == 2 * K and not torch.equal(per_image[0][1], per_image[1][0])
    for k in range(K):
        for b in range(2):
            want = hip.warp_perspective(fed2[k * 2 + b:k * 2 + b + 1], per_image[b][k], clamp=True)
            assert torch.equal(model.img_ref_stack[k * 2 + b:k * 2 + b + 1], want), (k, b)
    # outside validation a fed batch counts from image 0
    model.feed_data(batches[1])
    assert torch.equal(model.img_ref_stack, hip.warp_perspective(_stack(batches[1]).cuda(), views.indexed_corner_homographies(4, 0, K, H, W, (3, 12)),
                                                                 clamp=True))


# ------------------------------------------------------------------ val.match_probe
def _twin_extractor(model):
    """the LR stack's weights in the reference stack -> the state to put back"""
    ext = model.get_bare_model(model.net_extractor)
    saved = {k: v.clone() for k, v in ext.feature_extraction_image2.state_dict().items()}
    ext.feature_extraction_image2.load_state_dict(ext.feature_extraction_image1.state_dict())
    return saved


def test_the_probe_finds_an_integer_translation_of_the_input_itself():
    from mrefsr_amd import hip
    model = _test_model(dict(match_probe=dict(source='lq_up', margin=3, thresholds=[1, 2])))
    data = _data()
    saved = _twin_extractor(model)
    try:
        model.feed_data(data)
        assert torch.equal(views.to_feature_coords(torch.tensor(SHIFT, dtype=torch.float64)),
                           torch.tensor([[1.0, 0, 1.0], [0, 1.0, -2.0], [0, 0, 1.0]], dtype=torch.float64))
        got = model.match_probe(SHIFT)
        print('probe, margin 3:', got)
        assert got == dict(count=66, match_epe=0.0, match_pck1=1.0, match_pck2=1.0)
        model.match_probe_cfg = dict(model.match_probe_cfg, margin=2)
        got2 = model.match_probe(torch.tensor(SHIFT, dtype=torch.float64))
        print('probe, margin 2 (the oracle finds wrong matches here; only the count is asserted):', got2)
        assert got2['count'] == 104
        # the probe leaves the fed batch and the pass alone
        model.test()
        model.check_numeric_range()
        assert torch.equal(model.match_img_in.cpu(), data['img_in_up'])
        # the view it made: the shifted input, zeros where the source is outside
        view = hip.warp_perspective(model.match_img_in, SHIFT, clamp=True).cpu()
        assert torch.equal(view[:, :, :H - 8, 4:], data['img_in_up'][:, :, 8:, :W - 4]) and not bool(view[:, :, H - 8:].any()) and not bool(view[..., :4].any())
    finally:
        model.get_bare_model(model.net_extractor).feature_extraction_image2.load_state_dict(saved)
    # source: gt needs the fed batch's own img_in: an earlier batch's GT is not taken for it
    model = _test_model(dict(match_probe=dict(source='gt', perturb=[3, 12])))
    model.feed_data(data)
    assert model.match_probe()['count'] > 0
    model.feed_data({k: v for k, v in data.items() if k != 'img_in'})
    with pytest.raises(ValueError, match=r'val\.match_probe\.source'):
        model.match_probe()
    # with the stacks' own (different) synthetic weights nothing of the kind is found: the probe measures the extractor
    model = _test_model(dict(match_probe=dict(source='lq_up', margin=3)))
    model.feed_data(data)
    other = model.match_probe(SHIFT)
    assert other['count'] == 66 and other['match_epe'] > 0.5


def test_validation_with_the_probe_returns_the_same_numbers_twice():
    val = dict(match_probe=dict(perturb=[3, 12], thresholds=[1, 2], margin=3, source='gt', seed=2))
    model = _test_model(val)
    batches = [dict(_data(f'refviews/p{i}'), lq_path=[f'p{i}.png']) for i in range(2)]
    plain = _test_model().validation(batches, 0, None)
    model = _test_model(val)
    scalars = {}

    class Tb:
        def add_scalar(self, k, v, it):
            scalars[k] = v
    first = model.validation(batches, 0, Tb())
    second = model.validation(batches, 0, None)
    keys = ['match_epe', 'match_pck1', 'match_pck2']
    assert all(k in first for k in keys) and [first[k] for k in keys] == [second[k] for k in keys]
    assert all(np.isfinite(first[k]) for k in keys) and 0 <= first['match_pck1'] <= first['match_pck2'] <= 1
    assert {k: scalars[k] for k in keys} == {k: first[k] for k in keys}
    assert {k: first[k] for k in plain} == plain   # the usual metrics are the usual ones
    # the pooled numbers are those of the two images' own probes under the views of (seed, index)
    total = np.zeros(4)
    for i, d in enumerate(batches):
        model.feed_data(d)
        s = views.indexed_corner_homographies(2, i, 1, H, W, (3, 12))
        r = model.match_probe(s)
        total += np.array([r['count'], r['match_epe'] * r['count'], r['match_pck1'] * r['count'], r['match_pck2'] * r['count']])
    assert total[0] > 0
    assert np.allclose(total[1:] / total[0], [first[k] for k in keys], rtol=1e-12, atol=0)
