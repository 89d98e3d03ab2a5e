"""GPU: the multi-reference training step with opt['degradation'] (B = 2, K = 2, GT 64 x 64, LR 16 x 16, n_blocks 2, synthetic
weights).

  1. feed_data synthesises: img_in_lq lies on the 1/255 grid and is not the dataset's, match_img_in is its bicubic x4 clamped to
     [0, 1], gt_usm is the sharpened GT; two models from one seed make identical steps with finite losses
  2. l1_gt_usm / percep_gt_usm / gan_gt_usm change exactly the losses they name
  3. test() after a training step uses the fed LQ unchanged; validation feeds the dataset's LQ and puts the flag back
  4. without the option: two models make the same step bit for bit and no degrade_* entry point of the library is called
  5. queue_size = 2 B: two batches fill the pool, the third comes out of it
  6. the options that are refused"""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

B, K, LR = 2, 2, 16
LAYERS = {'conv1_2': 0.1, 'conv2_2': 0.1, 'conv3_4': 1.0}
DEG = dict(resize_range=[0.2, 1.5])   # a GT side of 64 stays at 12 pixels or more in front of the second 21 x 21 blur


def _load_synth(module):
    spec = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    module.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()}, strict=True)


def _opt(degradation=None, gan=False, **top):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), total_iter=255000, warmup_iter=-1,
                 net_g_pretrain_steps=0, pixel_criterion='L1Loss', pixel_weight=1.0, deterministic=True)
    opt = dict(
        name='degrade', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, manual_seed=10, is_train=True,
        dist=False, rank=0, network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=2, groups=8),
        network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                         vgg_type='vgg19'),
        network_extractor=dict(type='ContrasMultiExtractorSep'),
        path=dict(pretrain_network_g=None, pretrain_network_feature_extractor=None, strict_load=True), train=train, val=dict(save_img=False))
    if gan:
        train.update(perceptual_opt=dict(layer_weights=dict(LAYERS)), gan_type='wgan_softplus', gan_weight=1e-3, grad_penalty_weight=0,
                     lr_d=1e-4, beta_d=[0.9, 0.999])
        opt['network_d'] = dict(type='StyleGAN2Discriminator', out_size=64, narrow=0.125)
    if degradation is not None:
        opt['degradation'] = degradation
    opt.update(top)
    return opt


def _data(tag='a'):
    samples = [synth.sr_sample(f'degrade/{tag}{i}', K, LR, LR) for i in range(B)]
    return {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}


def _model(opt):
    from mrefsr_amd.models import build_model
    torch.manual_seed(10)
    model = build_model(opt)
    for name in ('net_g', 'net_extractor', 'net_map'):
        _load_synth(model.get_bare_model(getattr(model, name)))
    return model


def _params(model):
    return {n: p.detach().clone() for n, p in model.get_bare_model(model.net_g).named_parameters()}


def test_feed_data_synthesises_and_two_models_from_one_seed_agree():
    from mrefsr_amd import hip
    data = _data()
    a, b = _model(_opt(dict(DEG))), _model(_opt(dict(DEG)))
    a.feed_data(data)
    lq = a.img_in_lq
    assert tuple(lq.shape) == (B, 3, LR, LR) and lq.dtype == torch.float32
    assert float((lq * 255 - (lq * 255).round()).abs().max()) <= 1e-4 and float(lq.min()) >= 0 and float(lq.max()) <= 1
    assert float((lq.cpu() - data['img_in_lq']).abs().max()) > 1e-2                      # not the dataset's bicubic LQ
    want = torch.clamp(hip.degrade_resize(lq, scale_factor=4, mode='bicubic'), 0, 1)
    assert torch.equal(a.match_img_in, want) and tuple(want.shape) == (B, 3, 4 * LR, 4 * LR)
    assert torch.equal(a.gt.cpu(), data['img_in']) and torch.equal(a.gt_usm, hip.degrade_usm(a.gt))
    assert len(a.img_ref_list) == K and torch.equal(a.img_ref_list[1].cpu(), data['img_ref_list'][:, 1])   # the references are untouched
    b.feed_data(data)
    assert torch.equal(a.img_in_lq, b.img_in_lq)
    for step in (1, 2):
        if step == 2:
            a.feed_data(data)
            b.feed_data(data)
            assert torch.equal(a.img_in_lq, b.img_in_lq) and not torch.equal(a.img_in_lq, lq)   # a new draw every batch
        a.optimize_parameters(step)
        b.optimize_parameters(step)
        la, lb = a.get_current_log(), b.get_current_log()
        assert np.isfinite(la['l_g_pix']) and la == lb
    pa, pb = _params(a), _params(b)
    assert all(torch.equal(pa[n], pb[n]) for n in pa)
    # train.hip_graph stays allowed with the option: the sharpened GT is one more static input of the capture
    graphed = _opt(dict(DEG))
    del graphed['train']['deterministic']
    graphed['train']['hip_graph'] = True
    m = _model(graphed)
    m.feed_data(data)
    assert m._train_graph_wanted() and m._train_inputs() == m._TRAIN_INPUTS + ('gt_usm',)


def test_gt_usm_switches_change_exactly_the_losses_they_name():
    data = _data()
    logs = {}
    for name in (None, 'l1_gt_usm', 'percep_gt_usm', 'gan_gt_usm'):
        model = _model(_opt(dict(DEG), gan=True, **({name: True} if name else {})))
        model.feed_data(data)
        assert float((model.gt_usm - model.gt).abs().max()) > 1e-3
        model.optimize_parameters(1)
        logs[name] = model.get_current_log()
        assert all(np.isfinite(v) for v in logs[name].values()), logs[name]
    base = logs[None]
    owned = {'l1_gt_usm': 'l_g_pix', 'percep_gt_usm': 'l_g_percep', 'gan_gt_usm': 'l_d_real'}
    for name, key in owned.items():
        for other in owned.values():
            same = logs[name][other] == base[other]
            assert same == (other != key), (name, other, logs[name][other], base[other])
    # the generator's adversarial term sees D after its step: it moves with D's real images only
    assert logs['l1_gt_usm']['l_g_gan'] == base['l_g_gan'] == logs['percep_gt_usm']['l_g_gan'] != logs['gan_gt_usm']['l_g_gan']


def test_test_and_validation_do_not_synthesise():
    data = _data()
    model = _model(_opt(dict(DEG)))
    model.feed_data(data)
    model.optimize_parameters(1)
    lq, up = model.img_in_lq.clone(), model.match_img_in.clone()
    model.test()
    assert torch.equal(model.img_in_lq, lq) and torch.equal(model.match_img_in, up) and bool(torch.isfinite(model.output).all())
    assert model._synthesise
    model.nondist_validation([data], 1, None, False)
    assert torch.equal(model.img_in_lq.cpu(), data['img_in_lq']) and torch.equal(model.match_img_in.cpu(), data['img_in_up'])
    assert model.gt_usm is None and model._synthesise
    model.feed_data(data)                        # and training batches are synthesised again
    assert not torch.equal(model.img_in_lq.cpu(), data['img_in_lq']) and model.gt_usm is not None


def test_without_the_option_nothing_changes_and_no_degrade_entry_is_called(monkeypatch):
    from mrefsr_amd import _lib
    called = []
    real = _lib.call

    def counting(name, *args):
        called.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', counting)
    data = _data()
    a, b = _model(_opt()), _model(_opt())
    assert a.degradation is None and not a._synthesise and a._train_inputs() == a._TRAIN_INPUTS
    for m in (a, b):
        m.feed_data(data)
        assert torch.equal(m.img_in_lq.cpu(), data['img_in_lq']) and torch.equal(m.match_img_in.cpu(), data['img_in_up']) and m.gt_usm is None
        m.optimize_parameters(1)
    assert a.get_current_log() == b.get_current_log()
    pa, pb = _params(a), _params(b)
    assert all(torch.equal(pa[n], pb[n]) for n in pa) and torch.equal(a.output, b.output)
    assert called and not [n for n in called if 'degrade' in n]
    c = _model(_opt(dict(DEG)))
    c.feed_data(data)
    assert {n for n in called if 'degrade' in n} >= {'mrefsr_degrade_usm_f32', 'mrefsr_degrade_filter2d_f32', 'mrefsr_degrade_resize_f32',
                                                    'mrefsr_degrade_jpeg_f32', 'mrefsr_degrade_noise_f32'}


def test_pair_pool_of_two_batches_swaps_on_the_third_step():
    model = _model(_opt(dict(DEG, queue_size=2 * B)))
    batches = [_data(t) for t in 'abc']
    fed = []
    for i, data in enumerate(batches[:2]):
        model.feed_data(data)
        assert torch.equal(model.gt.cpu(), data['img_in']) and model.pair_pool.ptr == B * (i + 1)
        fed.append((model.gt.clone(), model.img_in_lq.clone(), torch.stack(model.img_ref_list, 1).clone()))
        model.optimize_parameters(i + 1)
    model.feed_data(batches[2])
    assert model.pair_pool.ptr == 2 * B
    gts, lqs, refs = (torch.cat([f[j] for f in fed]) for j in range(3))
    for s in range(B):      # every sample of the third batch is one of the pooled ones, with its own lq and references
        hit = [q for q in range(2 * B) if torch.equal(model.gt[s], gts[q])]
        assert len(hit) == 1, hit
        assert torch.equal(model.img_in_lq[s], lqs[hit[0]]) and torch.equal(torch.stack(model.img_ref_list, 1)[s], refs[hit[0]])
    from mrefsr_amd import hip
    assert torch.equal(model.gt_usm, hip.degrade_usm(model.gt))
    model.optimize_parameters(3)
    assert np.isfinite(model.get_current_log()['l_g_pix'])
    held = model.pair_pool.queue['img_in']
    assert sum(bool(torch.equal(held[q].cpu(), batches[2]['img_in'][s])) for q in range(2 * B) for s in range(B)) == B


def test_refused_options():
    from mrefsr_amd.models import build_model
    with pytest.raises(ValueError, match='l1_gt_usm'):
        build_model(_opt(l1_gt_usm=True))
    with pytest.raises(ValueError, match=r"\['resize_probs'\]"):
        build_model(_opt(dict(resize_probs=[1, 0, 0])))
    with pytest.raises(ValueError, match='scale'):
        build_model(_opt(dict(scale=2)))
    model = _model(_opt(dict(DEG)))
    bad = _data()
    bad['img_in'] = bad['img_in'][:, :, :56].contiguous()
    with pytest.raises(ValueError, match='multiple of 4'):
        model.feed_data(bad)
    with pytest.raises(ValueError, match='a dict'):
        build_model(_opt(True))
    # {} is the option with every default: at a GT side of 64 its resize_range [0.15, 1.5] is refused by name
    with pytest.raises(ValueError, match='resize_range '):
        _model(_opt({})).feed_data(_data())
    with pytest.raises(ValueError, match='divisible'):
        _model(_opt(dict(DEG, queue_size=3))).feed_data(_data())
