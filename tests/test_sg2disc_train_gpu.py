"""GPU: StyleGAN2Discriminator (archs/discriminator_arch.py) and the adversarial training step of MultiRefRestorationModel with it.

  a. the whole discriminator against an fp64 CPU restatement with the same weights and the kernels' LeakyReLU masks: D(x), d D / d x,
     the WGAN-GP penalty and d penalty / d every parameter; B = 4 (one stddev group), 2 (a group of 2) and 8 (two groups)
  b. optimize_parameters against the reference's own steps (tests/golden/e2e_c2_gan_sg2.npz: WGAN-GP; e2e_c2_gan_sg2_vanilla.npz:
     vanilla, net_d_steps 2, steps 1 and 2; both from tests/golden/gen_golden_gan_sg2.py)
  c. two fresh D steps give the same bits; d. training states round-trip; e. RefRestorationModel with this discriminator;
  f. the refusals that need a GPU tensor; g. a step with perceptual + style + this discriminator"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
import synth_sg2disc
from conftest import spec_from
from test_archs_gpu import load_synth
from test_configs_gpu import _opt
from test_disc_train_gpu import _rel
from test_sg2disc_kernels_gpu import fir64

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NET_D = dict(type='StyleGAN2Discriminator', out_size=128)
SQRT2 = math.sqrt(2)


def _disc(stat_gain=1.0, **kw):
    """stat_gain multiplies final_conv's weights of the stddev channel (1 of C + 1 inputs under unit-normal weights: it carries 1 / C of
    final_conv's input energy, and its second-order effect on a conv_body gradient drowns in the rest)"""
    from mrefsr_amd.archs import build_network
    net = build_network(dict(type='StyleGAN2Discriminator', **kw))
    spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd = synth_sg2disc.state_dict(spec)
    sd['final_conv.0.weight'][:, -1] *= stat_gain
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.to(DEV).train(), sd


def _record_masks(monkeypatch):
    """the LeakyReLU masks of every activated layer of every forward from now on, in launch order (the input stage, conv1 and conv2 of
    each ResBlock, final_conv, final_linear.0): pre-activations within rounding of 0 have no defined sign in fp32, so
    the fp64 restatement takes the masks from the kernels' forward"""
    from mrefsr_amd import hip
    rec = []

    def wrap(name):
        real = getattr(hip, name)

        def conv(*a, **kw):
            y = real(*a, **kw)
            if (a[4] if len(a) > 4 else kw.get('act_slope')) is not None:
                rec.append(y > 0)
            return y
        monkeypatch.setattr(hip, name, conv)
    wrap('disc_vconv')
    wrap('disc_sg2_conv')
    real_head = hip.disc_linear_head

    def head(*a, **kw):
        out, hidden = real_head(*a, **kw)
        rec.append(hidden > 0)
        return out, hidden
    monkeypatch.setattr(hip, 'disc_linear_head', head)
    return rec


def _stat(out, group):
    """the reference's minibatch-stddev map (stylegan2_arch.py:786-792) of out [B,C,H,W] -> [B,1,H,W]"""
    b, c, h, w = out.shape
    sd = out.view(group, -1, 1, c, h, w)
    sd = torch.sqrt(sd.var(0, unbiased=False) + 1e-8)
    sd = sd.mean([2, 3, 4], keepdims=True).squeeze(2)
    return sd.repeat(group, 1, h, w)


class _StatConstBackward(torch.autograd.Function):
    """_stat whose backward treats the saved activations as constants: the gradient it returns is still linear in the incoming one, but
    its own derivative towards the activations -- the term the double backward must carry -- is dropped"""

    @staticmethod
    def forward(ctx, out, group):
        ctx.group = group
        ctx.save_for_backward(out)
        return _stat(out, group)

    @staticmethod
    def backward(ctx, g):
        out = ctx.saved_tensors[0].detach().requires_grad_(True)
        with torch.enable_grad():
            gh, = torch.autograd.grad(_stat(out, ctx.group), out, g, create_graph=True)
        return gh, None


def _ref_forward(net, sd, x, masks, drop_stat_term=False):
    """StyleGAN2Discriminator.forward in fp64 torch (the reference's arithmetic, stylegan2_arch.py:589-799) with the kernels' masks"""
    masks = list(masks)
    taps = torch.tensor(net.resample_taps, dtype=torch.float64)

    def act(z):
        m = masks.pop(0).cpu()
        return torch.where(m.permute(0, 3, 1, 2) if m.dim() == 4 else m, z, 0.2 * z) * SQRT2

    def conv(x, key, stride=1, padding=0):
        w = sd[key]
        return F.conv2d(x, w * (1 / math.sqrt(w.shape[1] * w.shape[2] ** 2)), None, stride, padding)

    def bias(key):
        return sd[key].view(1, -1, 1, 1)
    h = act(conv(x, 'conv_body.0.0.weight') + bias('conv_body.0.1.bias'))
    for n in range(1, len(net.conv_body)):
        p = f'conv_body.{n}.'
        t = act(conv(h, p + 'conv1.0.weight', 1, 1) + bias(p + 'conv1.1.bias'))
        t = act(conv(fir64(t, taps, (2, 2), 1), p + 'conv2.1.weight', 2) + bias(p + 'conv2.2.bias'))
        h = (t + conv(fir64(h, taps, (1, 1), 1), p + 'skip.1.weight', 2)) / SQRT2
    b = h.shape[0]
    group = min(b, net.stddev_group)
    h = torch.cat([h, _StatConstBackward.apply(h, group) if drop_stat_term else _stat(h, group)], 1)
    h = act(conv(h, 'final_conv.0.weight', 1, 1) + bias('final_conv.1.bias'))
    h = h.reshape(b, -1)
    w1, w2 = sd['final_linear.0.weight'], sd['final_linear.1.weight']
    h = act(F.linear(h, w1 / math.sqrt(w1.shape[1])) + sd['final_linear.0.bias'])
    assert not masks
    return F.linear(h, w2 / math.sqrt(w2.shape[1]), sd['final_linear.1.bias'])


def _penalty64(net, sd64, real, fake, masks, b, drop=False):
    torch.manual_seed(7)
    alpha = torch.rand(b, 1, 1, 1).double()
    xi = (alpha * real.double() + (1 - alpha) * fake.double()).requires_grad_(True)
    di = _ref_forward(net, sd64, xi, masks, drop)
    gi, = torch.autograd.grad(di, xi, torch.ones_like(di), create_graph=True)
    return ((gi.view(b, -1).norm(2, dim=1) - 1)**2).mean()


@pytest.mark.parametrize('b,kw', [(4, dict(out_size=64)), (2, dict(out_size=64)), (8, dict(out_size=64)), (4, dict(out_size=128, narrow=0.5))])
def test_discriminator_and_penalty_vs_fp64(b, kw, monkeypatch):
    """Gates: 1e-4 relative for D(x) [7.1e-7], d D / d x [1.5e-6] and the penalty [4.5e-8], 1e-3 for every penalty gradient [1.7e-4, a
    conv_body bias] (the sibling discriminators' gates; measured worst over the four cases in brackets); no parameter is excused
    except those whose fp64 gradient is None or zero (the biases behind the stddev channel: d D / d x does not depend on them)"""
    from mrefsr_amd.losses import gradient_penalty_loss
    masks = _record_masks(monkeypatch)
    # the narrow case checks the stddev double-backward term: its weights give the stddev channel the weight of 32^2 channels
    net, sd = _disc(stat_gain=32.0 if 'narrow' in kw else 1.0, **kw)
    size = kw['out_size']
    n_masks = 1 + 2 * (len(net.conv_body) - 1) + 2
    sd64 = {k: torch.from_numpy(np.asarray(v)).double().requires_grad_(True) for k, v in sd.items()}
    g = torch.Generator().manual_seed(b * 1000 + size)
    real = torch.rand(b, 3, size, size, generator=g) * 2 - 1
    fake = torch.rand(b, 3, size, size, generator=g) * 2 - 1
    x = real.to(DEV).requires_grad_(True)
    out = net(x)
    gx, = torch.autograd.grad(out.sum(), x)
    assert len(masks) == n_masks
    xr = real.double().requires_grad_(True)
    want = _ref_forward(net, sd64, xr, masks)
    wgx, = torch.autograd.grad(want.sum(), xr)
    assert out.shape == want.shape == (b, 1)
    print(f'\n[sg2 fp64 b={b} {kw}] D(x) {_rel(out, want):.2e}  dD/dx {_rel(gx, wgx):.2e}')
    assert _rel(out, want) <= 1e-4 and _rel(gx, wgx) <= 1e-4, (_rel(out, want), _rel(gx, wgx))
    for p in net.parameters():
        p.grad = None
    torch.manual_seed(7)
    del masks[:]
    pen = gradient_penalty_loss(net, real.to(DEV), fake.to(DEV))
    pen.backward()
    assert len(masks) == n_masks   # one forward; the backward passes launch no masked forward
    wpen = _penalty64(net, sd64, real, fake, masks, b)
    wpen.backward()
    print(f'[sg2 fp64 b={b} {kw}] penalty {abs(pen.item() - wpen.item()) / abs(wpen.item()):.2e} ({wpen.item():.4f})')
    assert abs(pen.item() - wpen.item()) <= 1e-4 * abs(wpen.item()), (pen.item(), wpen.item())
    worst, none = {}, set()
    for n, p in net.named_parameters():
        if sd64[n].grad is None or float(sd64[n].grad.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            none.add(n)
            continue
        worst[n] = _rel(p.grad, sd64[n].grad)
    print(f'[sg2 fp64 b={b} {kw}] worst penalty gradient {max(worst.values()):.2e} ({max(worst, key=worst.get)}); zero: {sorted(none)}')
    assert all(n.endswith('bias') for n in none), none
    assert set(worst) >= {n for n, _ in net.named_parameters() if n.endswith('weight')}
    assert not {n: v for n, v in worst.items() if v > 1e-3}, worst
    if 'narrow' in kw:
        # the stddev channel's double backward towards the activations: without it, the penalty gradient of a conv_body weight (all of
        # them were compared above) is off by at least ten times that comparison's gate.  Measured on the fp64 side.
        keys = [n for n in worst if n.startswith('conv_body.') and n.endswith('weight')]
        full = {n: sd64[n].grad.clone() for n in keys}
        for v in sd64.values():
            v.grad = None
        _penalty64(net, sd64, real, fake, masks, b, drop=True).backward()
        missing = {n: _rel(sd64[n].grad, full[n]) for n in keys}
        key = max(missing, key=missing.get)
        print(f'[sg2 fp64 b={b} {kw}] dropping the stddev double-backward term changes the penalty gradient of {key} by {missing[key]:.2e} '
              f'(conv_body.1.conv1.0.weight: {missing["conv_body.1.conv1.0.weight"]:.2e})')
        assert missing[key] >= 1e-2, missing   # ten times the gate of the comparison


def test_refusals_on_the_gpu():
    net, _ = _disc(out_size=32, narrow=0.125)
    for shape in ((4, 3, 64, 64), (4, 3, 32, 40)):
        with pytest.raises(RuntimeError, match='final_linear'):
            net(torch.rand(shape, device=DEV))
    with pytest.raises(RuntimeError, match='not divisible'):
        net(torch.rand(6, 3, 32, 32, device=DEV))
    with pytest.raises(NotImplementedError, match='fp32'):
        net(torch.rand(4, 3, 32, 32, device=DEV, dtype=torch.float16))
    # not an RGB batch: refused before final_linear is in question (the reference fails in its first convolution there), with the
    # siblings' NotImplementedError
    for shape in ((4, 1, 32, 32), (4, 4, 32, 32), (3, 32, 32)):
        with pytest.raises(NotImplementedError, match=r'fp32 \[B,3,H,W\] only'):
            net(torch.rand(shape, device=DEV))
    assert net(torch.rand(3, 3, 32, 32, device=DEV)).shape == (3, 1)   # a batch below stddev_group is its own group


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
        sd = synth_sg2disc.state_dict(spec) if name == 'net_d' else synth.state_dict(spec)
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    b, k, (lr_h, lr_w), key = int(g['b']), int(g['k']), [int(v) for v in g['lr_hw']], str(g['key'])
    samples = [synth.sr_sample(f'{key}/s{i}', k, lr_h, lr_w) for i in range(b)]
    data = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    assert str(g['chk']) == synth.checksum(*[data[n].numpy() for n in ('img_in_lq', 'img_in_up', 'img_ref_list', 'img_in')])
    model.feed_data(data)
    return model


def _fingerprints_close(tag, net, names, gsum, gabs, psum, grad_rel, psum_tol):
    params = dict(net.named_parameters())
    assert list(params) == names
    worst_g, worst_p, fails = 0.0, 0.0, []
    for i, n in enumerate(names):
        gr = params[n].grad.detach().double()
        eg = max(abs(float(gr.abs().sum()) - float(gabs[i])), abs(float(gr.sum()) - float(gsum[i])))
        ep = abs(float(params[n].detach().double().sum()) - float(psum[i]))
        worst_g, worst_p = max(worst_g, eg / (float(gabs[i]) + 1e-30)), max(worst_p, ep)
        if eg > grad_rel * float(gabs[i]) + 1e-6 or ep > psum_tol:
            fails.append((n, eg, float(gabs[i]), ep))
    print(f'[sg2 fixture {tag}] worst gradient fingerprint {worst_g:.2e} of its abs-sum, worst parameter sum {worst_p:.2e}')
    assert not fails, fails


def _check_step(g, model, logs, log_rel, g_grad_rel, d_grad_rel, psum_tol):
    """the step(s) against the reference's fixture.  log_rel: {(step, log key): relative gate}, 1e-4 otherwise; the gradient fingerprints
    of net_g and net_d relative to their abs-sums; psum_tol: parameter sums after the Adam step(s)"""
    fails = []
    for step in logs:
        for k in [str(s) for s in g[f's{step}_log_keys']]:
            want, got = float(g[f's{step}_{k}']), logs[step][k]
            print(f'[sg2 fixture log] step {step} {k}: {abs(got - want) / abs(want):.2e} ({want:.6g})')
            if abs(got - want) > log_rel.get((step, k), 1e-4) * abs(want) + 1e-9:
                fails.append((step, k, got, want))
    assert not fails, fails
    _fingerprints_close('net_g', model.get_bare_model(model.net_g), [str(n) for n in g['param_names']], g['grad_sum'], g['grad_abs'],
                        g['param_sum_after'], g_grad_rel, psum_tol)
    _fingerprints_close('net_d', model.get_bare_model(model.net_d), [str(n) for n in g['d_param_names']], g['d_grad_sum'], g['d_grad_abs'],
                        g['d_param_sum_after'], d_grad_rel, psum_tol)


def test_wgan_gp_step_vs_reference(golden):
    """gan_type wgan, gan_weight 1e-3, grad_penalty_weight 10: one optimize_parameters(1) against the reference's.  Every log of this
    step is taken before D's first Adam update: 1e-4 [1.9e-5, out_d_fake at |value| 0.0047]; the D gradient fingerprints likewise
    [3.5e-6].  net_g's gradients and the parameter sums after Adam keep the gates of test_vggdisc_train_gpu.py: 5e-2 of the abs-sum
    [2.6e-4], 3e-2 [7.8e-4]."""
    g = golden('e2e_c2_gan_sg2')
    torch.manual_seed(int(g['seed']))
    assert np.array_equal(torch.rand(4, 1, 1, 1).numpy().reshape(1, -1), g['alpha'])
    model = _gan_model(g)
    assert len(model.optimizers) == 2 and len(model.schedulers) == 2 and model.optimizers[1] is model.optimizer_d
    torch.manual_seed(int(g['seed']))
    model.optimize_parameters(1)
    _check_step(g, model, {1: model.get_current_log()}, {}, 5e-2, 1e-4, 3e-2)


def test_vanilla_two_steps_vs_reference(golden):
    """gan_type vanilla, no penalty, net_d_steps 2: step 1 trains D only (logs 1e-4 [1.9e-5]), step 2 trains D and G after D's Adam
    update: the gates of test_vggdisc_train_gpu.py (step 2's D losses 1e-3 [4.3e-7], its other logs 1e-4 [2.3e-6], gradients 5e-2 of
    their abs-sum [net_g 2.6e-4, net_d 1.0e-5], parameter sums 2e-2 [6.3e-4])"""
    g = golden('e2e_c2_gan_sg2_vanilla')
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
    _check_step(g, model, logs, {(2, 'l_d_real'): 1e-3, (2, 'l_d_fake'): 1e-3}, 5e-2, 5e-2, 2e-2)


def test_d_step_is_deterministic():
    """two fresh discriminators under one seed: the same bits of the WGAN-GP D loss, every gradient and the parameters after an Adam
    step (fixed summation orders, no float atomics)"""
    from mrefsr_amd.losses import GANLoss, GradientPenaltyLoss
    g = torch.Generator().manual_seed(5)
    real = (torch.rand(4, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    fake = (torch.rand(4, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    runs = []
    for _ in range(2):
        net, _ = _disc(out_size=64, narrow=0.5)
        opt = torch.optim.Adam(net.parameters(), lr=1e-4, betas=(0.9, 0.999))
        gan, gp = GANLoss('wgan'), GradientPenaltyLoss(10.0)
        torch.manual_seed(3)
        loss = gan(net(real), True, is_disc=True) + gan(net(fake), False, is_disc=True) + gp(net, real, fake)
        loss.backward()
        opt.step()
        runs.append([loss.detach()] + [p.grad.clone() for p in net.parameters()] + [p.detach().clone() for p in net.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_training_state_round_trip(golden, tmp_path):
    g = golden('e2e_c2_gan_sg2')
    path = dict(training_states=str(tmp_path / 'states'), models=str(tmp_path / 'models'))
    model = _gan_model(g, path=path)
    for it in (1, 2):
        model.update_learning_rate(it)
        model.optimize_parameters(it)
    model.save_training_state(0, 2)
    model.save(0, 2)
    assert os.path.exists(tmp_path / 'models' / 'net_d_2.pth')
    saved = torch.load(str(tmp_path / 'models' / 'net_d_2.pth'), map_location='cpu')['params']
    assert [(k, tuple(v.shape)) for k, v in saved.items()] == spec_from(g, 'net_d_')   # the reference's keys, shapes and order
    state = torch.load(str(tmp_path / 'states' / '2.state'), map_location='cpu', weights_only=False)
    assert len(state['optimizers']) == 2 and len(state['schedulers']) == 2
    model2 = _gan_model(g, path=path)
    model2.load_network(model2.net_d, str(tmp_path / 'models' / 'net_d_2.pth'))
    model2.resume_training(state)
    s1, s2 = model.optimizer_d.state_dict()['state'], model2.optimizer_d.state_dict()['state']
    assert s1.keys() == s2.keys()
    for k in s1:
        assert torch.equal(s1[k]['exp_avg'].cpu(), s2[k]['exp_avg'].cpu()) and int(s1[k]['step']) == int(s2[k]['step'])
    sd1, sd2 = model.get_bare_model(model.net_d).state_dict(), model2.get_bare_model(model2.net_d).state_dict()
    assert list(sd1) == list(sd2)
    for k in sd1:
        assert torch.equal(sd1[k].cpu(), sd2[k].cpu()), k


def test_single_reference_model_with_stylegan2_discriminator(golden):
    from mrefsr_amd.models import build_model
    g = golden('singleref')
    opt = _opt(True)
    opt.update(model_type='RefRestorationModel', network_g=dict(type='RestorationNet', ngf=64, n_blocks=16, groups=8),
               network_extractor=dict(type='ContrasExtractorSep'), network_d=dict(NET_D, narrow=0.5))
    opt['train'].update(gan_type='wgan', gan_weight=1e-3, grad_penalty_weight=10.0, lr_d=1e-4, beta_d=[0.9, 0.999])
    model = build_model(opt)
    load_synth(model.get_bare_model(model.net_g), spec_from(g, 'net_'))
    load_synth(model.get_bare_model(model.net_map), spec_from(g, 'map_'))
    load_synth(model.get_bare_model(model.net_extractor), spec_from(g, 'ext_'))
    s = synth.sr_sample('sg2disc/singleref', 1, 32, 32)
    data = {k: torch.from_numpy(s[k][None]) for k in ('img_in_lq', 'img_in_up', 'img_in')}
    data['img_ref'] = torch.from_numpy(s['img_ref_list'][:1])
    model.feed_data(data)
    w0 = model.get_bare_model(model.net_d).conv_body[1].skip[1].weight.detach().clone()
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert {'l_d_real', 'l_d_fake', 'l_grad_penalty', 'l_g_gan', 'l_g_pix'} <= set(log)
    assert all(np.isfinite(v) for v in log.values())
    assert not torch.equal(w0, model.get_bare_model(model.net_d).conv_body[1].skip[1].weight.detach())


def test_gan_with_perceptual_and_style_is_finite(golden):
    g = golden('e2e_c2_gan_sg2')
    layers = {'conv1_2': 0.1, 'conv2_2': 0.1, 'conv3_4': 1.0, 'conv4_4': 1.0, 'conv5_4': 1.0}
    model = _gan_model(g, dict(perceptual_opt=dict(layer_weights=layers), style_opt=dict(layer_weights=layers, perceptual_weight=0,
                                                                                          style_weight=100.0)))
    torch.manual_seed(1)
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert {'l_g_pix', 'l_g_percep', 'l_g_style', 'l_g_gan', 'l_grad_penalty', 'l_d_real', 'l_d_fake'} <= set(log)
    assert all(np.isfinite(v) for v in log.values())
