"""GPU: ImageDiscriminator (archs/discriminator_arch.py) and the adversarial training step of MultiRefRestorationModel.

  a. the whole discriminator against an fp64 CPU restatement with the same weights: D(x), d D / d x, the WGAN-GP penalty and
     d penalty / d theta for every parameter (two batch sizes and an odd image size)
  b. optimize_parameters against the reference's own steps (tests/golden/e2e_c2_gan.npz: WGAN-GP; e2e_c2_gan_vanilla.npz: vanilla,
     net_d_steps 2, steps 1 and 2; both from tests/golden/gen_golden_gan.py)
  c. three steps finite, two fresh models the same bits; d. a tripped fp16-range flag re-runs net_g's forward without repeating the
     D step; e. save_training_state / resume_training with two optimizers; g. RefRestorationModel with a discriminator"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
import synth_disc
from conftest import spec_from
from test_archs_gpu import load_synth
from test_configs_gpu import _check_train_step_against_reference, _opt

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _disc(seed_spec=None, ndf=32):
    from mrefsr_amd.archs import build_network
    net = build_network(dict(type='ImageDiscriminator', in_nc=3, ndf=ndf))
    spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd = synth_disc.state_dict(spec)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.to(DEV).train(), sd


def _ref_forward(sd, x, masks=None):
    """ImageDiscriminator.forward in fp64 torch (training-mode BatchNorm).  masks: the LeakyReLU masks (z > 0) of the ten
    BatchNorm layers taken from the kernels' own forward (see _record_masks)"""
    h, i = x, 0
    for blk in range(1, 6):
        for conv, bn, stride in ((0, 1, 1), (3, 4, 2)):
            p = f'conv_block{blk}.'
            h = F.conv2d(h, sd[f'{p}{conv}.weight'], sd[f'{p}{conv}.bias'], stride=stride, padding=1)
            z = F.batch_norm(h, None, None, sd[f'{p}{bn}.weight'], sd[f'{p}{bn}.bias'], True, 0.1, 1e-5)
            h = F.leaky_relu(z, 0.2) if masks is None else torch.where(masks[i].permute(0, 3, 1, 2).cpu(), z, 0.2 * z)
            i += 1
    h = h.mean((2, 3), keepdim=True)
    h = F.leaky_relu(F.conv2d(h, sd['out_block.1.weight'], sd['out_block.1.bias']), 0.2)
    return torch.sigmoid(F.conv2d(h, sd['out_block.3.weight'], sd['out_block.3.bias']))


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).norm() / want.norm().clamp_min(1e-300)).item()


def _record_masks(monkeypatch):
    """the LeakyReLU masks of every BatchNorm launch from now on, in launch order.  Pre-activations within ~1e-7 of 0 occur (one is
    1.2e-10 at B = 4, 160 x 160): their sign is rounding noise in any fp32 arithmetic -- torch's own fp32 autograd is 5.8e-3 off
    fp64 in d D / d x at B = 2, 96 x 96 for that reason -- so the fp64 restatement takes the masks from the kernels' forward."""
    from mrefsr_amd import hip
    rec, real = [], hip.disc_bn_lrelu

    def wrap(*a, **kw):
        r = real(*a, **kw)
        rec.append(r[0] > 0)
        return r
    monkeypatch.setattr(hip, 'disc_bn_lrelu', wrap)
    return rec


@pytest.mark.parametrize('b,h,w', [(4, 160, 160), (2, 96, 96), (3, 75, 53)])
def test_discriminator_and_penalty_vs_fp64(b, h, w, monkeypatch):
    from mrefsr_amd.losses import gradient_penalty_loss
    masks = _record_masks(monkeypatch)
    net, sd = _disc()
    params = dict(net.named_parameters())
    sd64 = {k: torch.from_numpy(np.asarray(v)).double().requires_grad_(k in params) for k, v in sd.items()}
    g = torch.Generator().manual_seed(b * 1000 + h)
    real = torch.rand(b, 3, h, w, generator=g) * 2 - 1
    fake = torch.rand(b, 3, h, w, generator=g) * 2 - 1
    # D(x) and d D / d x
    x = real.to(DEV).requires_grad_(True)
    out = net(x)
    gx, = torch.autograd.grad(out.sum(), x)
    xr = real.double().requires_grad_(True)
    want = _ref_forward(sd64, xr, masks[:10])
    wgx, = torch.autograd.grad(want.sum(), xr)
    assert out.shape == want.shape == (b, 1, 1, 1)
    assert _rel(out, want) <= 1e-4 and _rel(gx, wgx) <= 1e-4, (_rel(out, want), _rel(gx, wgx))
    # the penalty and its parameter gradients (reference's gradient_penalty_loss, alpha under one seed)
    for p in net.parameters():
        p.grad = None
    torch.manual_seed(7)
    del masks[:]
    pen = gradient_penalty_loss(net, real.to(DEV), fake.to(DEV))
    pen.backward()
    torch.manual_seed(7)
    alpha = torch.rand(b, 1, 1, 1).double()
    xi = (alpha * real.double() + (1 - alpha) * fake.double()).requires_grad_(True)
    di = _ref_forward(sd64, xi, masks[:10])
    gi, = torch.autograd.grad(di, xi, torch.ones_like(di), create_graph=True)
    wpen = ((gi.view(b, -1).norm(2, dim=1) - 1)**2).mean()
    wpen.backward()
    assert abs(pen.item() - wpen.item()) <= 1e-4 * abs(wpen.item()), (pen.item(), wpen.item())
    worst = {}
    for n, p in net.named_parameters():
        ref = sd64[n].grad
        if n.startswith('conv_block') and n.endswith('bias') and n.split('.')[1] in ('0', '3'):
            # a conv bias in front of a training-mode BatchNorm: its gradient is 0 analytically (rounding noise on both sides)
            wg = dict(net.named_parameters())[n[:-4] + 'weight'].grad
            assert p.grad.abs().max().item() <= 1e-4 * wg.abs().max().item(), n
            continue
        worst[n] = _rel(p.grad, ref)
    bad = {n: v for n, v in worst.items() if v > 1e-3}
    assert not bad, bad


def _gan_model(g, extra_train=None, network_d=True, model_type='MultiRefRestorationModel', path=None):
    from mrefsr_amd.models import build_model
    opt = _opt(True)
    opt['model_type'] = model_type
    opt['network_d'] = dict(type='ImageDiscriminator', in_nc=3, ndf=32) if network_d else None
    opt['train'].update(gan_type=str(g['gan_type']), gan_weight=float(g['gan_weight']), grad_penalty_weight=float(g['grad_penalty_weight']),
                        lr_d=float(g['lr_d']), beta_d=[0.9, 0.999], net_d_steps=int(g['net_d_steps']))
    opt['train'].update(extra_train or {})
    opt['path'].update(path or {})
    model = build_model(opt)
    for name in ('net_g', 'net_extractor', 'net_map', 'net_d'):
        net = model.get_bare_model(getattr(model, name))
        spec = spec_from(g, name + '_')
        assert sorted((k, tuple(v.shape)) for k, v in net.state_dict().items()) == sorted(spec), name
        sd = synth_disc.state_dict(spec) if name == 'net_d' else synth.state_dict(spec)
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    b, k, (lr_h, lr_w), key = int(g['b']), int(g['k']), [int(v) for v in g['lr_hw']], str(g['key'])
    samples = [synth.sr_sample(f'{key}/s{i}', k, lr_h, lr_w) for i in range(b)]
    data = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    assert str(g['chk']) == synth.checksum(*[data[n].numpy() for n in ('img_in_lq', 'img_in_up', 'img_ref_list', 'img_in')])
    model.feed_data(data)
    return model


def _bias_before_bn(n):
    return n.startswith('conv_block') and n.endswith('bias') and n.split('.')[1] in ('0', '3')


def _check_d(g, model, step_logs, grad_rel, param_sum_tol=5e-3, stat_tol=1e-4):
    """grad_rel: the gate on net_d's gradient fingerprints.  D's fake input is net_g's output, which carries the generator's own
    spread from the reference (the L1 step's gate on net_g's gradients is 2e-3, tests/test_configs_gpu.py)"""
    log = model.get_current_log()
    for step in step_logs:
        for k in [str(s) for s in g[f's{step}_log_keys']]:
            want = float(g[f's{step}_{k}'])
            got = step_logs[step][k]
            assert abs(got - want) <= 1e-4 * abs(want) + 1e-9, (step, k, got, want)
    del log
    net = model.get_bare_model(model.net_d)
    params = dict(net.named_parameters())
    names = [str(n) for n in g['d_param_names']]
    assert list(params) == names
    worst = 0.0
    for i, n in enumerate(names):
        gr = params[n].grad.detach().double()
        if _bias_before_bn(n):   # analytically 0: the fixture holds rounding noise (Adam then moves them by +-lr on its sign)
            assert float(gr.abs().sum()) <= 1e-4 * float(g['d_grad_abs'].max()), n
            continue
        ga = float(g['d_grad_abs'][i])
        assert abs(float(gr.abs().sum()) - ga) <= grad_rel * ga, (n, float(gr.abs().sum()), ga)
        assert abs(float(gr.sum()) - float(g['d_grad_sum'][i])) <= grad_rel * ga, (n, float(gr.sum()), float(g['d_grad_sum'][i]))
        worst = max(worst, abs(float(params[n].detach().double().sum()) - float(g['d_param_sum_after'][i])))
    assert worst <= param_sum_tol, worst
    bn = [(n, m) for n, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert [n for n, _ in bn] == [str(s) for s in g['bn_names']]
    rm = torch.cat([m.running_mean.detach().cpu() for _, m in bn]).double().numpy()
    rv = torch.cat([m.running_var.detach().cpu() for _, m in bn]).double().numpy()
    # (the batch statistics of the fake / interpolated images and of the G step's forward -- D after its Adam step -- carry the
    # spread of net_g's output and of D's sign-ambiguous Adam moves: 1e-4 of the scale; the kernel alone is held to 1e-5 of fp64 in
    # tests/test_disc_kernels_gpu.py)
    np.testing.assert_allclose(rm, g['bn_running_mean'], rtol=stat_tol, atol=stat_tol * np.abs(g['bn_running_mean']).max())
    np.testing.assert_allclose(rv, g['bn_running_var'], rtol=stat_tol, atol=stat_tol * np.abs(g['bn_running_var']).max())
    assert [int(m.num_batches_tracked) for _, m in bn] == [int(v) for v in g['bn_num_batches_tracked']]


def test_wgan_gp_step_vs_reference(golden):
    """gan_type wgan, gan_weight 1e-3, grad_penalty_weight 10: one optimize_parameters(1) against the reference's"""
    g = golden('e2e_c2_gan')
    torch.manual_seed(int(g['seed']))
    assert np.array_equal(torch.rand(4, 1, 1, 1).numpy().reshape(1, -1), g['alpha'])   # the CPU generator draws alpha first
    model = _gan_model(g)
    assert len(model.optimizers) == 2 and len(model.schedulers) == 2 and model.optimizers[1] is model.optimizer_d
    torch.manual_seed(int(g['seed']))
    _check_train_step_against_reference(g, model)   # net_g: l_g_pix, per-parameter gradients, post-Adam sums
    _check_d(g, model, {1: model.get_current_log()}, 2e-3)


def test_vanilla_two_steps_vs_reference(golden):
    """gan_type vanilla, no penalty, net_d_steps 2: step 1 trains D only, step 2 trains D and G"""
    g = golden('e2e_c2_gan_vanilla')
    model = _gan_model(g)
    torch.manual_seed(int(g['seed']))
    before = {n: p.detach().clone() for n, p in model.get_bare_model(model.net_g).named_parameters()}
    logs = {}
    model.optimize_parameters(1)
    logs[1] = model.get_current_log()
    assert 'l_g_gan' not in logs[1] and 'l_g_pix' not in logs[1]
    for n, p in model.get_bare_model(model.net_g).named_parameters():
        assert torch.equal(p.detach(), before[n]), n        # no G update at step 1
    model.log_dict.clear()
    model.optimize_parameters(2)
    logs[2] = model.get_current_log()
    # step 2's D starts from step 1's Adam update, which moved every element by +-lr on the sign of its gradient: elements whose
    # gradient is near 0 move the other way here, so step 2's D gradients carry that spread as well
    # (and after two Adam steps of +-lr per element, the parameter sums by up to ~1e-2 where such elements accumulate, and the
    # running statistics of step 2's forwards, taken through that D, by up to 1e-3 of their scale)
    _check_d(g, model, logs, 5e-2, 2e-2, 1e-3)
    names = [str(n) for n in g['param_names']]
    params = dict(model.get_bare_model(model.net_g).named_parameters())
    for i, n in enumerate(names):
        gr = params[n].grad.detach().double()
        tol = 2e-3 * float(g['grad_abs'][i]) + 1e-6
        assert abs(float(gr.abs().sum()) - float(g['grad_abs'][i])) <= tol, n
        assert abs(float(gr.sum()) - float(g['grad_sum'][i])) <= tol, n


def test_three_steps_finite(golden):
    g = golden('e2e_c2_gan')
    model = _gan_model(g)
    torch.manual_seed(3)
    for step in (1, 2, 3):
        model.optimize_parameters(step)
        assert all(np.isfinite(v) for v in model.get_current_log().values())
    for net in (model.net_d, model.net_g):
        for p in model.get_bare_model(net).parameters():
            assert torch.isfinite(p).all()


def test_d_step_is_deterministic():
    """two fresh discriminators under one seed: the same bits of the WGAN-GP D loss, every gradient and the running statistics (fixed
    summation orders, no float atomics; net_g's own backward is not bitwise reproducible, so the D step is run on fixed images)"""
    from mrefsr_amd.losses import GANLoss, GradientPenaltyLoss
    g = torch.Generator().manual_seed(5)
    real = (torch.rand(4, 3, 160, 160, generator=g) * 2 - 1).to(DEV)
    fake = (torch.rand(4, 3, 160, 160, generator=g) * 2 - 1).to(DEV)
    runs = []
    for _ in range(2):
        net, _ = _disc()
        gan, gp = GANLoss('wgan'), GradientPenaltyLoss(10.0)
        torch.manual_seed(3)
        loss = gan(net(real), True, is_disc=True) + gan(net(fake), False, is_disc=True) + gp(net, real, fake)
        loss.backward()
        runs.append([loss.detach()] + [p.grad.clone() for p in net.parameters()] + [b.clone() for b in net.buffers()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_gan_with_perceptual_and_style_is_finite(golden):
    g = golden('e2e_c2_gan')
    layers = {'conv1_2': 0.1, 'conv2_2': 0.1, 'conv3_4': 1.0, 'conv4_4': 1.0, 'conv5_4': 1.0}
    model = _gan_model(g, dict(perceptual_opt=dict(layer_weights=layers), style_opt=dict(layer_weights=layers, perceptual_weight=0,
                                                                                          style_weight=100.0)))
    torch.manual_seed(1)
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert {'l_g_pix', 'l_g_percep', 'l_g_style', 'l_g_gan', 'l_grad_penalty'} <= set(log)
    assert all(np.isfinite(v) for v in log.values())


def test_range_flag_trip_runs_the_d_step_once(golden, monkeypatch):
    from mrefsr_amd import hip
    g = golden('e2e_c2_gan')
    model = _gan_model(g)
    real = hip.conv_range_tripped
    calls = []

    def tripped_once():
        calls.append(1)
        r = real()
        return True if len(calls) == 1 else r
    monkeypatch.setattr(hip, 'conv_range_tripped', tripped_once)
    torch.manual_seed(int(g['seed']))
    model.optimize_parameters(1)
    assert model.range_fallbacks == 1
    st = model.optimizer_d.state_dict()['state']
    assert st and all(int(s['step']) == 1 for s in st.values())
    net = model.get_bare_model(model.net_d)
    assert all(int(m.num_batches_tracked) == 4 for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert all(np.isfinite(v) for v in model.get_current_log().values())


def test_training_state_round_trip_with_two_optimizers(golden, tmp_path):
    g = golden('e2e_c2_gan')
    path = dict(training_states=str(tmp_path / 'states'), models=str(tmp_path / 'models'))
    model = _gan_model(g, path=path)
    for it in (1, 2):
        model.update_learning_rate(it)
        model.optimize_parameters(it)
    model.save_training_state(0, 2)
    model.save(0, 2)
    assert os.path.exists(tmp_path / 'models' / 'net_d_2.pth') and os.path.exists(tmp_path / 'models' / 'net_g_2.pth')
    state = torch.load(str(tmp_path / 'states' / '2.state'), map_location='cpu', weights_only=False)
    assert len(state['optimizers']) == 2 and len(state['schedulers']) == 2
    model2 = _gan_model(g, path=path)
    model2.load_network(model2.net_d, str(tmp_path / 'models' / 'net_d_2.pth'))
    model2.resume_training(state)
    s1, s2 = model.optimizer_d.state_dict()['state'], model2.optimizer_d.state_dict()['state']
    assert s1.keys() == s2.keys()
    for k in s1:
        assert torch.equal(s1[k]['exp_avg'].cpu(), s2[k]['exp_avg'].cpu()) and int(s1[k]['step']) == int(s2[k]['step'])
    for (n, a), b in zip(model.get_bare_model(model.net_d).state_dict().items(), model2.get_bare_model(model2.net_d).state_dict().values()):
        assert torch.equal(a.cpu(), b.cpu()), n


def test_single_reference_model_with_discriminator(golden):
    from mrefsr_amd.models import build_model
    g = golden('singleref')
    opt = _opt(True)
    opt.update(model_type='RefRestorationModel', network_g=dict(type='RestorationNet', ngf=64, n_blocks=16, groups=8),
               network_extractor=dict(type='ContrasExtractorSep'), network_d=dict(type='ImageDiscriminator'))
    opt['train'].update(gan_type='wgan', gan_weight=1e-3, grad_penalty_weight=10.0, lr_d=1e-4, beta_d=[0.9, 0.999])
    model = build_model(opt)
    load_synth(model.get_bare_model(model.net_g), spec_from(g, 'net_'))
    load_synth(model.get_bare_model(model.net_map), spec_from(g, 'map_'))
    load_synth(model.get_bare_model(model.net_extractor), spec_from(g, 'ext_'))
    data = {k: torch.from_numpy(g[k]) for k in ('img_in_lq', 'img_in_up', 'img_ref')}
    data['img_in'] = torch.from_numpy(g['out'])
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert {'l_d_real', 'l_d_fake', 'l_grad_penalty', 'l_g_gan', 'l_g_pix'} <= set(log)
    assert all(np.isfinite(v) for v in log.values())
