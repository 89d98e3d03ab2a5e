"""GPU: train.ema_decay and train.hip_adam in whole optimisation steps of MultiRefRestorationModel (B = 2, K = 2, LR 24 x 24,
two residual blocks; the e2e_c2 golden at its own shape for the comparison with the reference's step)."""
import logging
import os

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

DECAY = 0.999


def _opt(train_extra=None, is_train=True, path=None, network_d=None):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), total_iter=255000, warmup_iter=-1,
                 net_g_pretrain_steps=0, pixel_criterion='L1Loss', pixel_weight=1.0)
    train.update(train_extra or {})
    p = dict(pretrain_network_g=None, pretrain_network_feature_extractor=None, strict_load=True)
    p.update(path or {})
    return dict(
        name='optim', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, manual_seed=10, is_train=is_train,
        dist=False, rank=0, network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=2, groups=8),
        network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                         vgg_type='vgg19'),
        network_extractor=dict(type='ContrasMultiExtractorSep'), network_d=network_d, path=p, train=train, val=dict(save_img=False))


def _load_synth(model, names):
    for name in names:   # synthetic weights (a fresh MRAPARestorationNet has zero offset convolutions)
        net = model.get_bare_model(getattr(model, name))
        spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()})


def _batches(n=3):
    out = []
    for it in range(n):
        samples = [synth.sr_sample(f'optim/b{it}/s{i}', 2, 24, 24) for i in range(2)]
        out.append({k: torch.from_numpy(np.stack([s[k] for s in samples])) for k in samples[0]})
    return out


def _model(train_extra=None, **kw):
    from mrefsr_amd.models import build_model
    torch.manual_seed(10)
    model = build_model(_opt(train_extra, **kw))
    _load_synth(model, ('net_g', 'net_extractor', 'net_map'))
    if model.net_g_ema is not None:
        model.model_ema(0)   # (the weights were replaced behind the constructor's copy)
    return model


def _params(net):
    return {n: p.detach().clone() for n, p in net.named_parameters()}


def _run(train_extra, batches, **kw):
    """three steps: the model, net_g's parameters after each step and (with an EMA) net_g_ema's before the first and after each"""
    model = _model(train_extra, **kw)
    net = model.get_bare_model(model.net_g)
    posts, emas = [], [_params(model.net_g_ema)] if model.net_g_ema is not None else []
    for it, data in enumerate(batches, 1):
        model.feed_data(data)
        model.optimize_parameters(it)
        posts.append(_params(net))
        if model.net_g_ema is not None:
            emas.append(_params(model.net_g_ema))
    return model, posts, emas


def _assert_ema_recursion(posts, emas):
    """every update against float64 d * e + a * p of the recorded fp32 states (d, a the fp32-rounded scalars), within
    2^-23 * max(|e|, |p|) per element: the bound of one update (its roundings), so each update is fed the EMA recorded before it"""
    d, a = float(np.float32(DECAY)), float(np.float32(1.0 - DECAY))
    assert len(emas) == len(posts) + 1
    moved = 0
    for it, post in enumerate(posts):
        for n, p in post.items():
            e0, e1 = emas[it][n].double(), emas[it + 1][n].double()
            want = d * e0 + a * p.double()
            bound = 2.0 ** -23 * torch.maximum(e0.abs(), p.double().abs())
            assert bool(((e1 - want).abs() <= bound).all()), (it, n)
            moved += int((emas[it + 1][n] != emas[it][n]).sum())
    assert moved > 0


def _synth_named(model):
    """net_g's synthetic initial parameters by name"""
    net = model.get_bare_model(model.net_g)
    spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd = synth.state_dict(spec)
    return [(n, torch.from_numpy(sd[n]).cuda()) for n, _ in net.named_parameters()]


@pytest.fixture(scope='module')
def batches():
    return _batches()


@pytest.fixture(scope='module')
def ema_run(batches, tmp_path_factory):
    """train.ema_decay + train.deterministic, three steps, saved: shared by the tests below (nothing in it is modified)"""
    path = dict(models=str(tmp_path_factory.mktemp('ema') / 'models'))
    model, posts, emas = _run(dict(ema_decay=DECAY, deterministic=True), batches, path=path)
    model.save(0, 3)
    return model, posts, emas, os.path.join(path['models'], 'net_g_3.pth')


def test_ema_follows_the_recursion_and_leaves_net_g_alone(batches, ema_run):
    model, posts, emas, _ = ema_run
    assert model.net_g_ema is not None and not model.net_g_ema.training and model.net_g.training
    assert not any(p.requires_grad for p in model.net_g_ema.parameters())
    assert type(model.optimizer_g) is torch.optim.Adam
    start = dict(_synth_named(model))
    for n, p in emas[0].items():
        assert torch.equal(p, start[n])                           # initialised by an update with decay 0: net_g's bits
    _assert_ema_recursion(posts, emas)
    _, plain, none = _run(dict(deterministic=True), batches)      # the same run without an EMA: net_g bit-identical
    assert none == []
    for n in posts[-1]:
        for it in range(3):
            assert torch.equal(posts[it][n], plain[it][n]), (it, n)


def test_test_runs_the_ema_weights_and_the_checkpoint_holds_both(batches, ema_run, caplog):
    model, posts, emas, ckpt = ema_run
    saved = torch.load(ckpt, map_location='cpu')
    assert sorted(saved) == ['params', 'params_ema']
    for n, p in posts[-1].items():
        assert torch.equal(saved['params'][n], p.cpu()) and torch.equal(saved['params_ema'][n], emas[-1][n].cpu())
    with caplog.at_level(logging.WARNING, logger='basicsr'):
        model.feed_data(batches[0])
        model.test()
        out = model.output.clone()
        model.test()                                              # (and again, nothing having changed in between)
        assert torch.equal(model.output, out)
    assert 'without a version bump' not in caplog.text            # the EMA's raw-pointer writes moved its version counters
    assert model.net_g.training and not model.net_g_ema.training
    outs = {}
    for key in ('params_ema', 'params'):
        fresh = _fresh_for_test(ckpt, key)
        fresh.feed_data(batches[0])
        fresh.test()
        outs[key] = fresh.output.clone()
    assert torch.equal(out, outs['params_ema'])                  # test() ran net_g_ema: the bits of a model loaded from params_ema
    assert not torch.equal(out, outs['params'])


def _fresh_for_test(ckpt, key):
    from mrefsr_amd.models import build_model
    fresh = build_model(_opt(is_train=False, path=dict(pretrain_network_g=ckpt, param_key_g=key)))
    _load_synth(fresh, ('net_extractor', 'net_map'))
    return fresh


def test_hip_adam_takes_the_reference_step_of_config2(golden, monkeypatch):
    """train.hip_adam on the e2e_c2 golden (B = 4, K = 5, LR 40): the comparison of test_config2_train_step_b4_k5_lr40_vs_reference
    -- loss, gradient fingerprints, post-Adam parameter sums of the reference's optimize_parameters -- with that test's own checks
    and tolerances"""
    import test_configs_gpu as TC
    from mrefsr_amd.optim import HipAdam
    plain = TC._opt

    def opt(is_train):
        o = plain(is_train)
        o['train']['hip_adam'] = True
        return o
    monkeypatch.setattr(TC, '_opt', opt)
    g = golden('e2e_c2')
    model, data, _ = TC._golden_model(g, True)
    assert type(model.optimizer_g) is HipAdam
    model.feed_data(data)
    TC._check_train_step_against_reference(g, model)
    st = model.optimizer_g.state_dict()['state']
    assert len(st) == len(list(model.get_bare_model(model.net_g).parameters())) and all(float(s['step']) == 1.0 for s in st.values())


def _moments(model):
    st = model.optimizer_g.state
    return {n: (st[p]['exp_avg'].clone(), st[p]['exp_avg_sq'].clone(), float(st[p]['step']))
            for n, p in model.get_bare_model(model.net_g).named_parameters()}


def test_hip_adam_with_ema_is_bit_reproducible_and_resumes_into_torchs_adam(batches, tmp_path, caplog):
    from mrefsr_amd.optim import HipAdam
    extra = dict(hip_adam=True, ema_decay=DECAY, deterministic=True)
    path = dict(training_states=str(tmp_path / 'states'), models=str(tmp_path / 'models'))
    a, posts_a, emas_a = _run(extra, batches, path=path)
    b, posts_b, emas_b = _run(extra, batches)
    assert type(a.optimizer_g) is HipAdam and a.optimizer_g.ema_params and len(a.optimizer_g.ema_params) == len(posts_a[0])
    _assert_ema_recursion(posts_a, emas_a)                        # the EMA written by the Adam pass obeys the same recursion
    ma, mb = _moments(a), _moments(b)
    for n in posts_a[-1]:
        for it in range(3):
            assert torch.equal(posts_a[it][n], posts_b[it][n]), (it, n)
            assert torch.equal(emas_a[it + 1][n], emas_b[it + 1][n]), (it, n)
        assert torch.equal(ma[n][0], mb[n][0]) and torch.equal(ma[n][1], mb[n][1]) and ma[n][2] == mb[n][2] == 3.0, n
    with caplog.at_level(logging.WARNING, logger='basicsr'):
        a.feed_data(batches[0])
        a.test()
    assert 'without a version bump' not in caplog.text
    # resume into torch's own Adam (hip_adam: false)
    a.save_training_state(0, 3)
    a.save(0, 3)
    state = torch.load(os.path.join(path['training_states'], '3.state'), map_location='cpu', weights_only=False)
    c = _model(dict(ema_decay=DECAY, deterministic=True), path=dict(path, pretrain_network_g=os.path.join(path['models'], 'net_g_3.pth')))
    assert type(c.optimizer_g) is torch.optim.Adam
    c.load_network(c.net_g, os.path.join(path['models'], 'net_g_3.pth'))
    c.load_network(c.net_g_ema, os.path.join(path['models'], 'net_g_3.pth'), True, 'params_ema')
    c.resume_training(state)
    before = _params(c.get_bare_model(c.net_g))
    for n in before:
        assert torch.equal(before[n], posts_a[-1][n]) and torch.equal(dict(c.net_g_ema.named_parameters())[n], emas_a[-1][n])
    c.feed_data(batches[0])
    c.optimize_parameters(4)
    after = _params(c.get_bare_model(c.net_g))
    assert all(float(s['step']) == 4.0 for s in c.optimizer_g.state_dict()['state'].values())
    assert any(not torch.equal(after[n], before[n]) for n in after) and all(bool(torch.isfinite(v).all()) for v in after.values())
    # ... and back: that state into HipAdam
    c.save_training_state(0, 4)
    state4 = torch.load(os.path.join(path['training_states'], '4.state'), map_location='cpu', weights_only=False)
    a.resume_training(state4)
    a.feed_data(batches[1])
    a.optimize_parameters(5)
    assert all(float(s['step']) == 5.0 for s in a.optimizer_g.state_dict()['state'].values())


def test_adversarial_steps_with_hip_adam(batches):
    from mrefsr_amd.optim import HipAdam
    model = _model(dict(hip_adam=True, ema_decay=DECAY, gan_type='wgan', gan_weight=1e-3, grad_penalty_weight=10.0, lr_d=1e-4,
                        beta_d=[0.9, 0.999], net_d_steps=1), network_d=dict(type='ImageDiscriminator', in_nc=3, ndf=32))
    assert type(model.optimizer_d) is HipAdam and type(model.optimizer_g) is HipAdam and not model.optimizer_d.ema_params
    d0 = _params(model.get_bare_model(model.net_d))
    g0 = _params(model.get_bare_model(model.net_g))
    for it in (1, 2):
        model.feed_data(batches[it - 1])
        model.optimize_parameters(it)
    d1, g1 = _params(model.get_bare_model(model.net_d)), _params(model.get_bare_model(model.net_g))
    assert all(bool(torch.isfinite(v).all()) for v in list(d1.values()) + list(g1.values()) + list(_params(model.net_g_ema).values()))
    still = [n for n in d0 if torch.equal(d0[n], d1[n])]          # (a bias in front of a BatchNorm has no gradient to speak of)
    assert 2 * len(still) <= len(d0), still
    assert any(not torch.equal(g0[n], g1[n]) for n in g0)
    log = model.get_current_log()
    assert {'l_d_real', 'l_d_fake', 'l_grad_penalty', 'l_g_gan', 'l_g_pix'} <= set(log) and all(np.isfinite(v) for v in log.values())
    assert all(float(s['step']) == 2.0 for s in model.optimizer_d.state_dict()['state'].values())
