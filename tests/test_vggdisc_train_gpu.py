"""GPU: VGGStyleDiscriminator (archs/discriminator_arch.py) and the adversarial training step of MultiRefRestorationModel with it.

  a. the whole discriminator against an fp64 CPU restatement with the same weights: D(x), d D / d x, the WGAN-GP penalty and
     d penalty / d theta for every parameter, at (4, 160, 160) and (2, 160, 173)
  b. optimize_parameters against the reference's own steps (tests/golden/e2e_c2_gan_vgg.npz: WGAN-GP; e2e_c2_gan_vgg_vanilla.npz:
     vanilla, net_d_steps 2, steps 1 and 2; both from tests/golden/gen_golden_gan_vgg.py)
  c. two fresh D steps give the same bits; d. a tripped fp16-range flag updates the running statistics once; e. training states
     round-trip with two optimizers; f. RefRestorationModel with the new discriminator; g. the refusals that need a GPU tensor"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
import synth_vggdisc
from conftest import spec_from
from test_archs_gpu import load_synth
from test_configs_gpu import _opt
from test_disc_train_gpu import _rel

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NET_D = dict(type='VGGStyleDiscriminator', num_in_ch=3, num_feat=64)


def _disc():
    from mrefsr_amd.archs import build_network
    net = build_network(dict(NET_D))
    spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd = synth_vggdisc.state_dict(spec)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.to(DEV).train(), sd


def _record_masks(monkeypatch):
    """the LeakyReLU masks of every launch from now on, in launch order (conv0_0's epilogue, the nine BatchNorm layers, the head's
    hidden layer): pre-activations within rounding of 0 have no defined sign in fp32, so the fp64 restatement takes the
    masks from the kernels' forward"""
    from mrefsr_amd import hip
    rec = []
    real_conv, real_bn, real_head = hip.disc_vconv, hip.disc_bn_lrelu, hip.disc_linear_head

    def conv(*a, **kw):
        y = real_conv(*a, **kw)
        if (a[4] if len(a) > 4 else kw.get('act_slope')) is not None:
            rec.append(y > 0)
        return y

    def bn(*a, **kw):
        r = real_bn(*a, **kw)
        rec.append(r[0] > 0)
        return r

    def head(*a, **kw):
        r = real_head(*a, **kw)
        rec.append(r[1] > 0)
        return r
    monkeypatch.setattr(hip, 'disc_vconv', conv)
    monkeypatch.setattr(hip, 'disc_bn_lrelu', bn)
    monkeypatch.setattr(hip, 'disc_linear_head', head)
    return rec


def _ref_forward(sd, x, masks):
    """VGGStyleDiscriminator.forward in fp64 torch (training-mode BatchNorm) with the kernels' eleven LeakyReLU masks"""
    def act(z, m):
        return torch.where(m.permute(0, 3, 1, 2).cpu() if m.dim() == 4 else m.cpu(), z, 0.2 * z)
    h = act(F.conv2d(x, sd['conv0_0.weight'], sd['conv0_0.bias'], padding=1), masks[0])
    names = ['0_1'] + [f'{i}_{j}' for i in range(1, 5) for j in (0, 1)]
    for i, nm in enumerate(names):
        h = F.conv2d(h, sd[f'conv{nm}.weight'], None, stride=2 if nm.endswith('_1') else 1, padding=1)
        h = act(F.batch_norm(h, None, None, sd[f'bn{nm}.weight'], sd[f'bn{nm}.bias'], True, 0.1, 1e-5), masks[1 + i])
    hid = act(F.linear(h.reshape(h.shape[0], -1), sd['linear1.weight'], sd['linear1.bias']), masks[10])
    return F.linear(hid, sd['linear2.weight'], sd['linear2.bias'])


@pytest.mark.parametrize('b,h,w', [(4, 160, 160), (2, 160, 173)])
def test_discriminator_and_penalty_vs_fp64(b, h, w, monkeypatch):
    from mrefsr_amd.losses import gradient_penalty_loss
    masks = _record_masks(monkeypatch)
    net, sd = _disc()
    params = dict(net.named_parameters())
    sd64 = {k: torch.from_numpy(np.asarray(v)).double().requires_grad_(k in params) for k, v in sd.items()}
    g = torch.Generator().manual_seed(b * 1000 + w)
    real = torch.rand(b, 3, h, w, generator=g) * 2 - 1
    fake = torch.rand(b, 3, h, w, generator=g) * 2 - 1
    x = real.to(DEV).requires_grad_(True)
    out = net(x)
    gx, = torch.autograd.grad(out.sum(), x)
    assert len(masks) == 11
    xr = real.double().requires_grad_(True)
    want = _ref_forward(sd64, xr, masks)
    wgx, = torch.autograd.grad(want.sum(), xr)
    assert out.shape == want.shape == (b, 1)
    assert _rel(out, want) <= 1e-4 and _rel(gx, wgx) <= 1e-4, (_rel(out, want), _rel(gx, wgx))
    for p in net.parameters():
        p.grad = None
    torch.manual_seed(7)
    del masks[:]
    pen = gradient_penalty_loss(net, real.to(DEV), fake.to(DEV))
    pen.backward()
    assert len(masks) == 11   # one forward; the backward passes launch no masked forward
    torch.manual_seed(7)
    alpha = torch.rand(b, 1, 1, 1).double()
    xi = (alpha * real.double() + (1 - alpha) * fake.double()).requires_grad_(True)
    di = _ref_forward(sd64, xi, masks)
    gi, = torch.autograd.grad(di, xi, torch.ones_like(di), create_graph=True)
    wpen = ((gi.view(b, -1).norm(2, dim=1) - 1)**2).mean()
    wpen.backward()
    assert abs(pen.item() - wpen.item()) <= 1e-4 * abs(wpen.item()), (pen.item(), wpen.item())
    worst = {}
    for n, p in net.named_parameters():
        if sd64[n].grad is None:   # linear1.bias, linear2.bias: d D / d x does not depend on them (piecewise-linear head)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        worst[n] = _rel(p.grad, sd64[n].grad)
    assert not {n: v for n, v in worst.items() if v > 1e-3}, worst


def test_refusals_on_the_gpu():
    net, _ = _disc()
    with pytest.raises(RuntimeError, match='linear1 expects 12800 input features'):
        net(torch.rand(1, 3, 160, 192, device=DEV))
    net.eval()
    with pytest.raises(NotImplementedError, match='training mode'):
        net(torch.rand(1, 3, 160, 160, device=DEV))


def _gan_model(g, extra_train=None, path=None, model_type='MultiRefRestorationModel'):
    from mrefsr_amd.models import build_model
    opt = _opt(True)
    opt['model_type'] = model_type
    opt['network_d'] = dict(NET_D)
    opt['train'].update(gan_type=str(g['gan_type']), gan_weight=float(g['gan_weight']), grad_penalty_weight=float(g['grad_penalty_weight']),
                        lr_d=float(g['lr_d']), beta_d=[0.9, 0.999], net_d_steps=int(g['net_d_steps']))
    opt['train'].update(extra_train or {})
    opt['path'].update(path or {})
    model = build_model(opt)
    for name in ('net_g', 'net_extractor', 'net_map', 'net_d'):
        net = model.get_bare_model(getattr(model, name))
        spec = spec_from(g, name + '_')
        assert sorted((k, tuple(v.shape)) for k, v in net.state_dict().items()) == sorted(spec), name
        sd = synth_vggdisc.state_dict(spec) if name == 'net_d' else synth.state_dict(spec)
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    b, k, (lr_h, lr_w), key = int(g['b']), int(g['k']), [int(v) for v in g['lr_hw']], str(g['key'])
    samples = [synth.sr_sample(f'{key}/s{i}', k, lr_h, lr_w) for i in range(b)]
    data = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    assert str(g['chk']) == synth.checksum(*[data[n].numpy() for n in ('img_in_lq', 'img_in_up', 'img_ref_list', 'img_in')])
    model.feed_data(data)
    return model


def _fingerprints_close(net, names, gsum, gabs, psum, grad_rel, psum_tol):
    params = dict(net.named_parameters())
    assert list(params) == names
    for i, n in enumerate(names):
        gr = params[n].grad.detach().double()
        tol = grad_rel * float(gabs[i]) + 1e-6
        assert abs(float(gr.abs().sum()) - float(gabs[i])) <= tol, (n, float(gr.abs().sum()), float(gabs[i]))
        assert abs(float(gr.sum()) - float(gsum[i])) <= tol, (n, float(gr.sum()), float(gsum[i]))
        assert abs(float(params[n].detach().double().sum()) - float(psum[i])) <= psum_tol, n


def _check_step(g, model, logs, log_rel, g_grad_rel, d_grad_rel, psum_tol, stat_tol):
    """the step(s) against the reference's fixture.  log_rel: {log key: relative gate}; the gradient fingerprints of net_g and net_d
    relative to their abs-sums; psum_tol: parameter sums after the Adam step(s); stat_tol: running statistics, of their scale"""
    for step in logs:
        for k in [str(s) for s in g[f's{step}_log_keys']]:
            want, got = float(g[f's{step}_{k}']), logs[step][k]
            assert abs(got - want) <= log_rel.get((step, k), 1e-4) * abs(want) + 1e-9, (step, k, got, want)
    _fingerprints_close(model.get_bare_model(model.net_g), [str(n) for n in g['param_names']], g['grad_sum'], g['grad_abs'],
                        g['param_sum_after'], g_grad_rel, psum_tol)
    net = model.get_bare_model(model.net_d)
    _fingerprints_close(net, [str(n) for n in g['d_param_names']], g['d_grad_sum'], g['d_grad_abs'], g['d_param_sum_after'], d_grad_rel,
                        psum_tol)
    bn = [(n, m) for n, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert [n for n, _ in bn] == [str(s) for s in g['bn_names']]
    rm = torch.cat([m.running_mean.detach().cpu() for _, m in bn]).double().numpy()
    rv = torch.cat([m.running_var.detach().cpu() for _, m in bn]).double().numpy()
    np.testing.assert_allclose(rm, g['bn_running_mean'], rtol=stat_tol, atol=stat_tol * np.abs(g['bn_running_mean']).max())
    np.testing.assert_allclose(rv, g['bn_running_var'], rtol=stat_tol, atol=stat_tol * np.abs(g['bn_running_var']).max())
    assert [int(m.num_batches_tracked) for _, m in bn] == [int(v) for v in g['bn_num_batches_tracked']]


# What runs through D after its Adam step -- the G step's D forward and backward (l_g_gan and its gradient, which at gan_weight 1e-3
# outweighs the L1 term's in net_g's output gradient: |d D / d x| ~ 8 per image here), the fourth BatchNorm update, and step 2 of
# the vanilla fixture -- carries the spread of Adam's first step, which moves every element by +-lr on the sign of its gradient:
# elements whose gradient is rounding noise (linear1 alone has 1.28 M) move the other way than in the reference.  Everything before
# D's Adam step is held to 1e-4 (measured <= 6.1e-5); the wider gates below are on what comes after it (measured values in brackets).


def test_wgan_gp_step_vs_reference(golden):
    """gan_type wgan, gan_weight 1e-3, grad_penalty_weight 10: one optimize_parameters(1) against the reference's"""
    g = golden('e2e_c2_gan_vgg')
    torch.manual_seed(int(g['seed']))
    assert np.array_equal(torch.rand(4, 1, 1, 1).numpy().reshape(1, -1), g['alpha'])
    model = _gan_model(g)
    assert len(model.optimizers) == 2 and len(model.schedulers) == 2 and model.optimizers[1] is model.optimizer_d
    groups = [[pg['lr'], len(pg['params'])] for pg in model.optimizer_g.param_groups]
    np.testing.assert_allclose(np.array(groups, dtype=np.float64), g['opt_groups'])
    torch.manual_seed(int(g['seed']))
    model.optimize_parameters(1)
    # l_g_gan 1e-2 [4.6e-3]; net_g gradients 5e-2 of their abs-sum [3.7e-2, a PReLU slope]; D gradients 2e-3 [4.9e-4];
    # parameter sums 3e-2 [1.7e-2]; running statistics 1e-3 of scale [3.8e-4]
    _check_step(g, model, {1: model.get_current_log()}, {(1, 'l_g_gan'): 1e-2}, 5e-2, 2e-3, 3e-2, 1e-3)


def test_vanilla_two_steps_vs_reference(golden):
    """gan_type vanilla, no penalty, net_d_steps 2: step 1 trains D only, step 2 trains D and G"""
    g = golden('e2e_c2_gan_vgg_vanilla')
    model = _gan_model(g)
    torch.manual_seed(int(g['seed']))
    before = {n: p.detach().clone() for n, p in model.get_bare_model(model.net_g).named_parameters()}
    logs = {}
    model.optimize_parameters(1)
    logs[1] = model.get_current_log()
    assert 'l_g_gan' not in logs[1] and 'l_g_pix' not in logs[1]
    for n, p in model.get_bare_model(model.net_g).named_parameters():
        assert torch.equal(p.detach(), before[n]), n
    model.log_dict.clear()
    model.optimize_parameters(2)
    logs[2] = model.get_current_log()
    # step 2's D losses 1e-3 [3.8e-4: softplus at |out| = 7.4 amplifies out_d_fake's 5.8e-5]; net_g gradients 5e-2 [2.1e-2];
    # D gradients 5e-2 [1.1e-2], parameter sums 2e-2 [1.0e-2], running statistics 1e-3 of scale [2.1e-4] (those of e2e_c2_gan_vanilla)
    _check_step(g, model, logs, {(2, 'l_d_real'): 1e-3, (2, 'l_d_fake'): 1e-3}, 5e-2, 5e-2, 2e-2, 1e-3)


def test_d_step_is_deterministic():
    """two fresh discriminators under one seed: the same bits of the WGAN-GP D loss, every gradient, the running statistics and the
    parameters after an Adam step"""
    from mrefsr_amd.losses import GANLoss, GradientPenaltyLoss
    g = torch.Generator().manual_seed(5)
    real = (torch.rand(4, 3, 160, 160, generator=g) * 2 - 1).to(DEV)
    fake = (torch.rand(4, 3, 160, 160, generator=g) * 2 - 1).to(DEV)
    runs = []
    for _ in range(2):
        net, _ = _disc()
        opt = torch.optim.Adam(net.parameters(), lr=1e-4, betas=(0.9, 0.999))
        gan, gp = GANLoss('wgan'), GradientPenaltyLoss(10.0)
        torch.manual_seed(3)
        loss = gan(net(real), True, is_disc=True) + gan(net(fake), False, is_disc=True) + gp(net, real, fake)
        loss.backward()
        opt.step()
        runs.append([loss.detach()] + [p.grad.clone() for p in net.parameters()] + [p.detach().clone() for p in net.parameters()] +
                    [b.clone() for b in net.buffers()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_range_flag_trip_updates_the_statistics_once(golden, monkeypatch):
    from mrefsr_amd import hip
    g = golden('e2e_c2_gan_vgg')
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
    g = golden('e2e_c2_gan_vgg')
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


def test_single_reference_model_with_vggstyle_discriminator(golden):
    from mrefsr_amd.models import build_model
    g = golden('singleref')
    opt = _opt(True)
    opt.update(model_type='RefRestorationModel', network_g=dict(type='RestorationNet', ngf=64, n_blocks=16, groups=8),
               network_extractor=dict(type='ContrasExtractorSep'), network_d=dict(NET_D))
    opt['train'].update(gan_type='wgan', gan_weight=1e-3, grad_penalty_weight=10.0, lr_d=1e-4, beta_d=[0.9, 0.999])
    model = build_model(opt)
    load_synth(model.get_bare_model(model.net_g), spec_from(g, 'net_'))
    load_synth(model.get_bare_model(model.net_map), spec_from(g, 'map_'))
    load_synth(model.get_bare_model(model.net_extractor), spec_from(g, 'ext_'))
    s = synth.sr_sample('vggdisc/singleref', 1, 40, 40)   # GT 160 x 160: VGGStyleDiscriminator asserts input_size 160
    data = {k: torch.from_numpy(s[k][None]) for k in ('img_in_lq', 'img_in_up', 'img_in')}
    data['img_ref'] = torch.from_numpy(s['img_ref_list'][:1])
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert {'l_d_real', 'l_d_fake', 'l_grad_penalty', 'l_g_gan', 'l_g_pix'} <= set(log)
    assert all(np.isfinite(v) for v in log.values())
