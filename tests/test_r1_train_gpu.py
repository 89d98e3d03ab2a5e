"""GPU: r1_penalty through the four discriminators and the lazily regularised D step of MultiRefRestorationModel.

  a. r1_penalty and d penalty / d every parameter against the fp64 restatements of the discriminators' own *_train_gpu.py files (the
     kernels' LeakyReLU masks, grad_outputs all ones on the real batch), at the smallest input and batch each of those files uses for
     its WGAN-GP test and under that test's gates: 1e-4 relative for the penalty, 1e-3 for every parameter gradient
  b. optimize_parameters(1) and (2) against the reference's own steps (tests/golden/e2e_c2_gan_sg2_r1.npz from
     tests/golden/gen_golden_gan_r1.py: wgan_softplus, r1_reg_weight 10, net_d_reg_every 2), gates of test_sg2disc_train_gpu.py
  c. the lazy schedule; d. bit reproducibility; e. clipping and hip_adam on the summed gradients; f. options absent: the launches of
     before.  (The DDP-wrapped D step is in test_zz_r1_dist_gpu.py: a process group is made in-process, at the end of the run.)"""
import math

import numpy as np
import pytest
import torch

import synth
import synth_sg2disc
import test_disc_train_gpu as T_IMG
import test_sg2disc_train_gpu as T_SG2
import test_unetdisc_train_gpu as T_UNET
import test_vggdisc_train_gpu as T_VGG
from conftest import spec_from
from test_configs_gpu import _opt
from test_disc_train_gpu import _rel
from test_gradclip_train_gpu import _coef32, _lane_squares
from test_optim_train_gpu import _model, _params
from test_sg2disc_kernels_gpu import fir64

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SG2_64 = dict(type='StyleGAN2Discriminator', out_size=64)


def _r1_vs_fp64(tag, net, sd64, real, masks, ref_forward, excused=(), torch32=None):
    """r1_penalty(net(x), x) on the kernels against the fp64 restatement with the masks of that forward.  Gates: the penalty 1e-4, every
    parameter gradient 1e-3.  ``torch32(masks)`` -> {name: gradient}: torch's own fp32 autograd of the same restatement on the same data;
    it is run only if a gradient misses 1e-3, and such a gradient may then be off by twice what torch's is (both are printed)."""
    from mrefsr_amd.losses import r1_penalty
    b = real.shape[0]
    for p in net.parameters():
        p.grad = None
    del masks[:]
    x = real.to(DEV).requires_grad_(True)
    pen = r1_penalty(net(x), x)
    pen.backward()
    n_masks = len(masks)
    xr = real.double().requires_grad_(True)
    gi, = torch.autograd.grad(ref_forward(xr, masks).sum(), xr, create_graph=True)
    assert len(masks) == n_masks   # one forward; the backward passes launch no masked forward
    wpen = gi.pow(2).reshape(b, -1).sum(1).mean()
    wpen.backward()
    err = abs(pen.item() - wpen.item()) / abs(wpen.item())
    worst, zero = {}, set()
    for n, p in net.named_parameters():
        if n in excused:
            continue
        ref = sd64[n].grad
        if ref is None or float(ref.abs().max()) == 0.0:   # d D / d x does not depend on it
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            zero.add(n)
            continue
        worst[n] = _rel(p.grad, ref)
    key = max(worst, key=worst.get)
    print(f'\n[r1 fp64 {tag}] penalty {err:.2e} ({wpen.item():.4g})  worst parameter gradient {worst[key]:.2e} ({key}); zero: {sorted(zero)}')
    assert err <= 1e-4, (pen.item(), wpen.item())
    assert all(n.endswith('bias') for n in zero), zero
    over = {n: v for n, v in worst.items() if v > 1e-3}
    if over and torch32 is not None:
        theirs = torch32(masks)
        torch_err = {n: _rel(theirs[n], sd64[n].grad) for n in over}
        for n in sorted(over):
            print(f'[r1 fp64 {tag}] {n}: kernels {over[n]:.2e}, torch fp32 autograd of the restatement {torch_err[n]:.2e}')
        over = {n: (v, torch_err[n]) for n, v in over.items() if v > 2 * torch_err[n]}
    assert not over, over


def _sd64(net, sd):
    params = dict(net.named_parameters())
    return {k: torch.from_numpy(np.asarray(v)).double().requires_grad_(k in params) for k, v in sd.items()}


def _real(b, h, w):
    return torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(b * 1000 + h + w)) * 2 - 1


def test_r1_image_discriminator_vs_fp64(monkeypatch):
    masks = T_IMG._record_masks(monkeypatch)
    net, sd = T_IMG._disc()
    sd64 = _sd64(net, sd)
    # a conv bias in front of a training-mode BatchNorm has gradient 0 analytically (rounding noise on both sides)
    excused = [n for n, _ in net.named_parameters() if n.startswith('conv_block') and n.endswith('bias') and n.split('.')[1] in ('0', '3')]
    _r1_vs_fp64('ImageDiscriminator 3x75x53', net, sd64, _real(3, 75, 53), masks, lambda x, m: T_IMG._ref_forward(sd64, x, m[:10]), excused)
    for n in excused:
        wg = dict(net.named_parameters())[n[:-4] + 'weight'].grad
        assert dict(net.named_parameters())[n].grad.abs().max().item() <= 1e-4 * wg.abs().max().item(), n


def test_r1_vggstyle_discriminator_vs_fp64(monkeypatch):
    masks = T_VGG._record_masks(monkeypatch)
    net, sd = T_VGG._disc()
    sd64 = _sd64(net, sd)
    _r1_vs_fp64('VGGStyleDiscriminator 2x160x173', net, sd64, _real(2, 160, 173), masks, lambda x, m: T_VGG._ref_forward(sd64, x, m))


def test_r1_unet_discriminator_vs_fp64(monkeypatch):
    masks = T_UNET._record_masks(monkeypatch)
    net, sd = T_UNET._disc(True)
    sd64 = _sd64(net, sd)
    uv1 = T_UNET._power64(sd64, 1)   # the one training forward of a fresh discriminator
    _r1_vs_fp64('UNetDiscriminatorSN 2x160x192', net, sd64, _real(2, 160, 192), masks, lambda x, m: T_UNET._ref_forward(sd64, x, m, uv1, True))


@pytest.mark.parametrize('b', [4, 2])
def test_r1_stylegan2_discriminator_vs_fp64(b, monkeypatch):
    """out_size 64; B = 4 is one stddev group, B = 2 a group of 2"""
    masks = T_SG2._record_masks(monkeypatch)
    net, sd = T_SG2._disc(out_size=64)
    sd64 = {k: torch.from_numpy(np.asarray(v)).double().requires_grad_(True) for k, v in sd.items()}
    real = _real(b, 64, 64)

    def torch32(m):
        """the restatement in fp32 (torch's CPU kernels), the same masks"""
        monkeypatch.setattr(T_SG2, 'fir64', lambda x, k, pad, down: fir64(x, k.to(x.dtype), pad, down))
        sd32 = {k: torch.from_numpy(np.asarray(v)).float().requires_grad_(True) for k, v in sd.items()}
        x32 = real.clone().requires_grad_(True)
        g32, = torch.autograd.grad(T_SG2._ref_forward(net, sd32, x32, m).sum(), x32, create_graph=True)
        g32.pow(2).reshape(b, -1).sum(1).mean().backward()
        return {k: v.grad for k, v in sd32.items() if v.grad is not None}
    _r1_vs_fp64(f'StyleGAN2Discriminator {b}x64x64', net, sd64, real, masks, lambda x, m: T_SG2._ref_forward(net, sd64, x, m), torch32=torch32)


# ------------------------------------------------------------------ b. against the reference
def _golden_model(g):
    from mrefsr_amd.models import build_model
    opt = _opt(True)
    opt['network_d'] = dict(SG2_64)
    opt['train'].update(gan_type=str(g['gan_type']), gan_weight=float(g['gan_weight']), grad_penalty_weight=float(g['grad_penalty_weight']),
                        lr_d=float(g['lr_d']), beta_d=[0.9, 0.999], net_d_steps=int(g['net_d_steps']),
                        r1_reg_weight=float(g['r1_reg_weight']), net_d_reg_every=int(g['net_d_reg_every']))
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


def test_softplus_r1_two_steps_vs_reference(golden):
    """gan_type wgan_softplus, gan_weight 1e-3, r1_reg_weight 10, net_d_reg_every 2, B = 4, K = 5, LR 16 x 16 with
    StyleGAN2Discriminator(64): step 1 has no R1, step 2 has it, after D's and G's first Adam updates.  Gates of
    test_sg2disc_train_gpu.py's two-step golden test: step 2's D losses 1e-3, the other logs 1e-4 -- l_d_r1 among them --, gradient
    fingerprints 5e-2 of their abs-sum, parameter sums 2e-2."""
    g = golden('e2e_c2_gan_sg2_r1')
    assert str(g['gan_type']) == 'wgan_softplus' and int(g['net_d_reg_every']) == 2 and [int(s) for s in g['steps']] == [1, 2]
    model = _golden_model(g)
    assert model.cri_grad_penalty is None and model.r1_reg_weight == 10.0 and model.net_d_reg_every == 2
    torch.manual_seed(int(g['seed']))
    logs = {}
    model.optimize_parameters(1)
    logs[1] = model.get_current_log()
    assert 'l_d_r1' not in logs[1]
    model.optimize_parameters(2)
    logs[2] = model.get_current_log()
    assert 'l_d_r1' in logs[2] and 'l_d_r1' in [str(s) for s in g['s2_log_keys']]
    for step in (1, 2):   # (r1_penalty: the generator's record of the unweighted value; the model logs the weighted l_d_r1)
        logs[step] = dict(logs[step], r1_penalty=logs[step].get('l_d_r1', 0.0) / (float(g['r1_reg_weight']) / 2 * int(g['net_d_reg_every'])))
    T_SG2._check_step(g, model, logs, {(2, 'l_d_real'): 1e-3, (2, 'l_d_fake'): 1e-3}, 5e-2, 5e-2, 2e-2)


# ------------------------------------------------------------------ c-f. the D step on a small model
GAN = dict(gan_type='wgan_softplus', gan_weight=1e-3, grad_penalty_weight=0.0, lr_d=1e-4, beta_d=[0.9, 0.999], net_d_steps=1)


def _batch(it=0):
    samples = [synth.sr_sample(f'r1/b{it}/s{i}', 2, 16, 16) for i in range(2)]   # GT 64 x 64
    return {k: torch.from_numpy(np.stack([s[k] for s in samples])) for k in samples[0]}


def _small(extra, network_d=SG2_64):
    """test_optim_train_gpu's two-block model (B = 2, K = 2) with a discriminator holding synthetic weights"""
    model = _model(dict(GAN, **extra), network_d=dict(network_d))
    net = model.get_bare_model(model.net_d)
    spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth_sg2disc.state_dict(spec).items()}, strict=True)
    return model


def _d_state(model):
    net = model.get_bare_model(model.net_d)
    return {n: p.grad.detach().clone() for n, p in net.named_parameters()}, _params(net)


@pytest.fixture(scope='module')
def data():
    return _batch()


@pytest.fixture(scope='module')
def r1_run(data):
    """step 1 with R1 on (every step), hip_adam and the norm logged but not clipped: shared, not modified"""
    model = _small(dict(r1_reg_weight=10.0, hip_adam=True, deterministic=True, skip_nonfinite_steps=True))
    start = _params(model.get_bare_model(model.net_d))
    model.feed_data(data)
    model.optimize_parameters(1)
    torch.cuda.synchronize()
    grads, params = _d_state(model)
    return dict(log=model.get_current_log(), grads=grads, params=params, start=start)


def test_lazy_schedule(data, monkeypatch):
    from mrefsr_amd import hip
    calls, real = [], hip.r1_sqnorm

    def counted(g):
        calls.append(tuple(g.shape))
        return real(g)
    monkeypatch.setattr(hip, 'r1_sqnorm', counted)
    model = _small(dict(r1_reg_weight=10.0, net_d_reg_every=2))
    model.feed_data(data)
    seen = []
    for step in (1, 2, 3, 4):   # (log_dict is left to the model, as in a training loop: a plain step drops the last l_d_r1)
        model.optimize_parameters(step)
        seen.append((len(calls), 'l_d_r1' in model.get_current_log()))
    assert seen == [(0, False), (1, True), (1, False), (2, True)]
    assert calls == [(2, 3, 64, 64)] * 2   # the gradient towards the real batch, once per regularised step


def test_two_fresh_runs_give_the_same_bits(data, r1_run):
    model = _small(dict(r1_reg_weight=10.0, hip_adam=True, deterministic=True, skip_nonfinite_steps=True))
    model.feed_data(data)
    model.optimize_parameters(1)
    grads, params = _d_state(model)
    log = model.get_current_log()
    assert log['l_d_r1'] == r1_run['log']['l_d_r1'] and log['grad_norm_d'] == r1_run['log']['grad_norm_d'] and log['l_d_r1'] > 0
    for n in grads:
        assert torch.equal(grads[n], r1_run['grads'][n]) and torch.equal(params[n], r1_run['params'][n]), n
    assert any(not torch.equal(params[n], r1_run['start'][n]) for n in params)


def test_clip_and_hip_adam_see_the_summed_gradients(data, r1_run):
    """grad_norm_d is the norm of the GAN and the R1 gradients together (DESIGN.md 3.4's bound), and the update is clip-then-Adam on
    that sum: the first moment within an ulp of (1 - beta1) fl32(g coef), the parameters no further from float64 Adam than twice
    torch's fused Adam on the same clipped gradients (the bars of test_gradclip_train_gpu.py)"""
    max_norm = 0.5 * r1_run['log']['grad_norm_d']
    model = _small(dict(r1_reg_weight=10.0, hip_adam=True, deterministic=True, grad_clip_norm_d=max_norm))
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    raw, params = _d_state(model)
    for n in raw:
        assert torch.equal(raw[n], r1_run['grads'][n]), n   # the gradient tensors are not written
    # ... and they hold more than the GAN term: a twin without R1 has other gradients
    plain = _small(dict(hip_adam=True, deterministic=True, skip_nonfinite_steps=True))
    plain.feed_data(data)
    plain.optimize_parameters(1)
    gan_only, _ = _d_state(plain)
    assert any(not torch.equal(raw[n], gan_only[n]) for n in raw) and 'l_d_r1' not in plain.get_current_log()
    want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in raw.values()))
    bound = ((_lane_squares([g.numel() for g in raw.values()]) + 1) / 2 + 2) * 2.0 ** -24
    err = abs(log['grad_norm_d'] - want) / want
    print(f'\ngrad_norm_d {log["grad_norm_d"]!r} float64 {want!r}: |rel err| / bound = {err / bound:.3f}')
    assert err <= bound and log['grad_norm_d'] == r1_run['log']['grad_norm_d'] and log['skipped_steps_d'] == 0
    coef = _coef32(log['grad_norm_d'], max_norm)
    assert np.float32(model.optimizer_d.clip_state.coef.item()) == coef and 0.49 < float(coef) < 0.51
    net = model.get_bare_model(model.net_d)
    grp = model.optimizer_d.param_groups[0]
    lr, (b1, b2), eps = grp['lr'], grp['betas'], grp['eps']
    clipped = {n: torch.from_numpy(raw[n].cpu().numpy() * coef).to(DEV) for n in raw}   # fl32(g * coef)
    twins = {n: torch.nn.Parameter(r1_run['start'][n].clone()) for n in raw}
    for n, q in twins.items():
        q.grad = clipped[n]
    torch.optim.Adam(list(twins.values()), lr=lr, betas=(b1, b2), eps=eps, fused=True).step()
    dh = dt = 0.0
    for n, p in net.named_parameters():
        g = clipped[n].cpu().double().numpy()
        m = model.optimizer_d.state[p]['exp_avg'].cpu().double().numpy()
        ulp = np.spacing(np.abs((1 - b1) * g).astype(np.float32)).astype(np.float64)
        assert (np.abs(m - (1 - b1) * g) <= ulp).all(), n
        want_p = r1_run['start'][n].cpu().double().numpy() - lr / (1 - b1) * ((1 - b1) * g) / (np.sqrt((1 - b2) * g * g) / math.sqrt(1 - b2) + eps)
        dh = max(dh, float(np.abs(params[n].cpu().double().numpy() - want_p).max()))
        dt = max(dt, float(np.abs(twins[n].detach().cpu().double().numpy() - want_p).max()))
    print(f'max |dev from float64 Adam| of the D parameters: hip_adam {dh:.3e}  clip + torch fused Adam {dt:.3e}')
    assert dt > 0.0 and dh <= 2.0 * dt


def _kernel_names(model, data, it):
    from torch.profiler import ProfilerActivity, profile
    model.feed_data(data)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        model.optimize_parameters(it)
        torch.cuda.synchronize()
    return [e.name.replace(' ', '') for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_options_absent_the_step_launches_what_it_launched(data, monkeypatch):
    """a wgan + WGAN-GP step without the new options: none of the new kernels, and the same kernel list as a step during which the
    new code path is not there to be taken (r1_penalty and both hip wrappers replaced by functions that raise).

    Both traces start from the same process-wide state of nhwc_train: its cache of fp16 weight scales is emptied and its count of
    range checks set to 0.  check_scales() takes one foreach norm over every cached weight that is still alive, those of earlier
    models included, so the number of its launches follows what the process ran before, and every 50th check is a full refresh."""
    from mrefsr_amd import hip, losses
    from mrefsr_amd.archs import nhwc_train
    wgan_gp = dict(gan_type='wgan', grad_penalty_weight=10.0, deterministic=True)

    def traced():
        nhwc_train.reset_scales()
        monkeypatch.setattr(nhwc_train._scales, 'checks', 0)
        torch.manual_seed(11)
        model = _small(wgan_gp)
        model.feed_data(data)
        model.optimize_parameters(1)
        torch.manual_seed(12)   # (the penalty's alpha)
        return model, _kernel_names(model, data, 2)
    model, names = traced()
    assert len(names) > 100 and not [n for n in names if 'r1_sqnorm' in n]
    assert 'l_d_r1' not in model.get_current_log() and 'l_grad_penalty' in model.get_current_log()

    def gone(*a, **kw):
        raise AssertionError('the R1 path was taken with its options absent')
    for mod, name in ((hip, 'r1_sqnorm'), (hip, 'r1_sqnorm_bwd'), (losses, 'r1_penalty'), (losses.losses, 'r1_penalty')):
        monkeypatch.setattr(mod, name, gone)
    _, without = traced()
    assert names == without
    monkeypatch.undo()
    # (the names do show with the option on: two forward launches and one backward launch per regularised step)
    model = _small(dict(wgan_gp, r1_reg_weight=10.0))
    model.feed_data(data)
    model.optimize_parameters(1)
    on = _kernel_names(model, data, 2)
    assert [sum(k in n for n in on) for k in ('r1_sqnorm_partial_kernel', 'r1_sqnorm_finalize_kernel', 'r1_sqnorm_bwd_kernel')] == [1, 1, 1]
    assert {'l_d_r1', 'l_grad_penalty'} <= set(model.get_current_log())   # WGAN-GP is still allowed beside R1
