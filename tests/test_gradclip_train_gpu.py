"""GPU: train.grad_clip_norm_g / train.grad_clip_norm_d / train.skip_nonfinite_steps in whole optimisation steps of
MultiRefRestorationModel (the set-up of test_optim_train_gpu: B = 2, K = 2, LR 24 x 24, two residual blocks, synthetic weights,
train.deterministic; the VGGStyleDiscriminator step at LR 40 x 40, the only image size that discriminator takes)."""
import math

import numpy as np
import pytest
import torch

import synth
from test_optim_train_gpu import DECAY, _batches, _model, _params, _synth_named

pytestmark = pytest.mark.gpu

GRID, CHUNK = 2048, 1024


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.get_bare_model(model.net_g).named_parameters() if p.grad is not None}


def _step(model, data, it=1):
    model.feed_data(data)
    model.optimize_parameters(it)
    torch.cuda.synchronize()


def _lane_squares(sizes):
    """L of the norm kernel's error bound: the most squares one lane adds (4 per chunk of its block's share of the table)"""
    t = sum((n + 3 + CHUNK - 1) // CHUNK for n in sizes if n)
    return 4 * max(t * (b + 1) // GRID - t * b // GRID for b in range(GRID))


def _coef32(total_norm, max_norm):
    c = np.float32(max_norm) / (np.float32(total_norm) + np.float32(1e-6))
    return np.float32(1.0) if c > 1 else c


@pytest.fixture(scope='module')
def batches():
    return _batches(2)


@pytest.fixture(scope='module')
def twin(batches):
    """step 1 without clipping (train.skip_nonfinite_steps alone: the norm is taken and logged, coef = 1), shared and not modified"""
    model = _model(dict(hip_adam=True, deterministic=True, skip_nonfinite_steps=True))
    _step(model, batches[0])
    log = model.get_current_log()
    st = model.optimizer_g.state
    net = model.get_bare_model(model.net_g)
    return dict(log=log, grads=_grads(model), params=_params(net), exp_avg={n: st[p]['exp_avg'].clone() for n, p in net.named_parameters()})


@pytest.fixture(scope='module')
def clipped(batches, twin):
    """step 1 with train.hip_adam and the norm clipped to half of what the twin logged"""
    max_norm = 0.5 * twin['log']['grad_norm_g']
    model = _model(dict(hip_adam=True, deterministic=True, grad_clip_norm_g=max_norm))
    _step(model, batches[0])
    return model, max_norm


def test_step_one_with_hip_adam_and_a_clip_against_the_unclipped_twin(twin, clipped):
    model, max_norm = clipped
    log = model.get_current_log()
    assert twin['log']['skipped_steps_g'] == 0 and log['skipped_steps_g'] == 0
    raw = _grads(model)
    for n, g in twin['grads'].items():
        assert torch.equal(raw[n], g), n                          # the gradient tensors are not written (and the step is deterministic)
    want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in raw.values()))
    L = _lane_squares([g.numel() for g in raw.values()])
    bound = ((L + 1) / 2 + 2) * 2.0 ** -24
    err = abs(log['grad_norm_g'] - want) / want
    print(f'grad_norm_g {log["grad_norm_g"]!r} float64 {want!r}: L = {L}, |rel err| / bound = {err / bound:.3f}')
    assert err <= bound and log['grad_norm_g'] == twin['log']['grad_norm_g']   # the unclipped norm, the same bits in both runs
    coef = _coef32(log['grad_norm_g'], max_norm)
    assert np.float32(model.optimizer_g.clip_state.coef.item()) == coef and 0.49 < float(coef) < 0.51
    st = model.optimizer_g.state
    beta1 = model.optimizer_g.param_groups[0]['betas'][0]
    worst = 0.0
    for n, p in model.get_bare_model(model.net_g).named_parameters():
        g_eff = (raw[n].cpu().numpy() * coef).astype(np.float64)   # fl32(g * coef)
        m = st[p]['exp_avg'].cpu().double().numpy()
        ulp = np.spacing(np.abs((1 - beta1) * g_eff).astype(np.float32)).astype(np.float64)
        assert (np.abs(m - (1 - beta1) * g_eff) <= ulp).all(), n
        # ... so it is the twin's first moment times coef
        mt = twin['exp_avg'][n].cpu().double().numpy()
        big = np.abs(mt) > 1e-30
        if big.any():
            worst = max(worst, float(np.abs(m[big] / mt[big] - float(coef)).max()))
    print(f'exp_avg / twin exp_avg - coef: worst {worst:.3e}')
    assert worst <= 4 * 2.0 ** -23                               # (one ulp on either side of the quotient, relative to coef ~ 0.5)
    assert all(float(s['step']) == 1.0 for s in model.optimizer_g.state_dict()['state'].values())


def test_step_one_without_hip_adam(batches, twin, clipped):
    hip_model, max_norm = clipped
    model = _model(dict(deterministic=True, grad_clip_norm_g=max_norm))
    assert type(model.optimizer_g) is torch.optim.Adam
    start = dict(_synth_named(model))
    _step(model, batches[0])
    log = model.get_current_log()
    assert log['grad_norm_g'] == twin['log']['grad_norm_g'] and log['skipped_steps_g'] == 0
    coef = _coef32(log['grad_norm_g'], max_norm)
    scaled = _grads(model)
    for n, g in twin['grads'].items():                            # scaled in place, as torch's clip does: fl32(raw * coef)
        assert np.array_equal(scaled[n].cpu().numpy().view(np.int32), (g.cpu().numpy() * coef).view(np.int32)), n
    # the parameters of the two runs, with the kernel test's bar: each against float64 Adam on fl32(raw * coef)
    lr_of = {p: (grp['lr'], grp['betas'], grp['eps']) for grp in model.optimizer_g.param_groups for p in grp['params']}
    mine, theirs = _params(hip_model.get_bare_model(hip_model.net_g)), _params(model.get_bare_model(model.net_g))
    dh = dt = 0.0
    for n, p in model.get_bare_model(model.net_g).named_parameters():
        lr, (b1, b2), eps = lr_of[p]
        g = (twin['grads'][n].cpu().numpy() * coef).astype(np.float64)
        m, v = (1 - b1) * g, (1 - b2) * g * g
        want = start[n].cpu().double().numpy() - lr / (1 - b1) * m / (np.sqrt(v) / math.sqrt(1 - b2) + eps)
        dh = max(dh, float(np.abs(mine[n].cpu().double().numpy() - want).max()))
        dt = max(dt, float(np.abs(theirs[n].cpu().double().numpy() - want).max()))
    print(f'step 1, max |dev from float64| of the parameters: hip_adam {dh:.3e}  clip + torch fused Adam {dt:.3e}')
    assert dt > 0.0 and dh <= 2.0 * dt


@pytest.mark.parametrize('hip_adam', [True, False], ids=['hip_adam', 'torch_adam'])
def test_a_poisoned_batch_is_skipped(batches, hip_adam):
    extra = dict(hip_adam=hip_adam, deterministic=True, ema_decay=DECAY, skip_nonfinite_steps=True)
    model = _model(extra)
    net = model.get_bare_model(model.net_g)
    with torch.no_grad():
        for e in model.net_g_ema.parameters():
            e.mul_(0.5)                                           # (away from net_g, so that an update of it shows)
    p0, e0 = _params(net), _params(model.net_g_ema)
    clean = model._loss_and_backward

    def poisoned(step):   # one gradient element becomes inf between backward and update
        out = clean(step)
        next(p for p in net.parameters() if p.grad is not None).grad.view(-1)[0] = float('inf')
        return out
    model._loss_and_backward = poisoned
    _step(model, batches[0], 1)
    model._loss_and_backward = clean
    log = model.get_current_log()
    assert log['skipped_steps_g'] == 1 and not np.isfinite(log['grad_norm_g'])
    p1, e1 = _params(net), _params(model.net_g_ema)
    for n in p0:
        assert torch.equal(p1[n], p0[n]), n                       # parameters bit for bit
    for p in net.parameters():
        st = model.optimizer_g.state[p]
        assert not bool(st['exp_avg'].any()) and not bool(st['exp_avg_sq'].any())   # the moments as they were: zero
    assert all(float(s['step']) == 0.0 for s in model.optimizer_g.state_dict()['state'].values())   # the un-advanced step
    assert model.get_current_log()['skipped_steps_g'] == 1        # (folded into the host counters or not)
    d, a = float(np.float32(DECAY)), float(np.float32(1.0 - DECAY))
    for n in e0:                                                  # the EMA update was made: d * e + a * p of the unchanged p
        want = d * e0[n].double() + a * p0[n].double()
        assert bool(((e1[n].double() - want).abs() <= 2.0 ** -23 * torch.maximum(e0[n].double().abs(), p0[n].double().abs())).all()), n
    assert any(not torch.equal(e1[n], e0[n]) for n in e0)
    # the next step against a twin that never ran that batch
    _step(model, batches[1], 2)
    other = _model(extra)
    _step(other, batches[1], 1)
    p2, q = _params(net), _params(other.get_bare_model(other.net_g))
    assert all(bool(torch.isfinite(v).all()) for v in p2.values())
    assert any(not torch.equal(p2[n], p0[n]) for n in p2)
    for n in p2:
        assert torch.equal(p2[n], q[n]), n
    assert all(float(s['step']) == 1.0 for s in model.optimizer_g.state_dict()['state'].values())
    log = model.get_current_log()
    assert log['skipped_steps_g'] == 1 and np.isfinite(log['grad_norm_g'])


def test_wgan_gp_step_with_vggstyle_discriminator_and_grad_clip_norm_d():
    samples = [synth.sr_sample(f'gradclip/s{i}', 2, 40, 40) for i in range(2)]   # GT 160 x 160, the size VGGStyleDiscriminator asserts
    data = {k: torch.from_numpy(np.stack([s[k] for s in samples])) for k in samples[0]}
    model = _model(dict(hip_adam=True, grad_clip_norm_d=1.0, grad_clip_norm_g=1.0, skip_nonfinite_steps=True, gan_type='wgan', gan_weight=1e-3,
                        grad_penalty_weight=10.0, lr_d=1e-4, beta_d=[0.9, 0.999], net_d_steps=1),
                   network_d=dict(type='VGGStyleDiscriminator', num_in_ch=3, num_feat=64))
    d0 = _params(model.get_bare_model(model.net_d))
    _step(model, data)
    log = model.get_current_log()
    print({k: log[k] for k in ('grad_norm_d', 'grad_norm_g', 'skipped_steps_d', 'skipped_steps_g', 'l_grad_penalty')})
    assert {'grad_norm_d', 'grad_norm_g', 'skipped_steps_d', 'skipped_steps_g', 'l_d_real', 'l_d_fake', 'l_grad_penalty', 'l_g_gan'} <= set(log)
    assert all(np.isfinite(v) for v in log.values())
    assert log['grad_norm_d'] > 0 and log['skipped_steps_d'] == 0 and log['skipped_steps_g'] == 0
    d1 = _params(model.get_bare_model(model.net_d))
    assert all(bool(torch.isfinite(v).all()) for v in d1.values()) and any(not torch.equal(d0[n], d1[n]) for n in d0)
    grads = [p.grad for p in model.net_d.parameters() if p.grad is not None]   # (hip_adam: left as backward wrote them)
    want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    assert abs(log['grad_norm_d'] - want) <= ((_lane_squares([g.numel() for g in grads]) + 1) / 2 + 2) * 2.0 ** -24 * want


def _kernel_names(model, data, it):
    from torch.profiler import ProfilerActivity, profile
    model.feed_data(data)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        model.optimize_parameters(it)
        torch.cuda.synchronize()
    return [e.name.replace(' ', '') for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


# the kernels behind the new entry points, as the trace names them (demangled, blanks removed) or mangled
NEW_KERNELS = dict(norm=('grad_walk_kernel<false>', 'grad_walk_kernelILb0E'), scale=('grad_walk_kernel<true>', 'grad_walk_kernelILb1E'),
                   finalize=('grad_norm_finalize_kernel',), adam_clip=('optim_multi_kernel<true,true>', 'optim_multi_kernelILb1ELb1E'))
PLAIN_ADAM = ('optim_multi_kernel<true,false>', 'optim_multi_kernelILb1ELb0E')


def _launched(names, forms):
    return any(f in n for n in names for f in forms)


def test_options_absent_no_new_kernel_is_launched(batches):
    for extra in (dict(deterministic=True), dict(deterministic=True, hip_adam=True, ema_decay=DECAY)):
        model = _model(extra)
        assert getattr(model.optimizer_g, '_mrefsr_clip', None) is None
        _step(model, batches[0], 1)
        names = _kernel_names(model, batches[1], 2)
        assert len(names) > 100
        assert not [k for k, forms in NEW_KERNELS.items() if _launched(names, forms)]
        assert _launched(names, PLAIN_ADAM) == bool(extra.get('hip_adam'))
        assert not {'grad_norm_g', 'skipped_steps_g'} & set(model.get_current_log())
    # (the names do show when the options are on: with train.hip_adam, then with torch's Adam)
    for hip_adam, want in ((True, {'norm', 'finalize', 'adam_clip'}), (False, {'norm', 'finalize', 'scale'})):
        model = _model(dict(deterministic=True, hip_adam=hip_adam, grad_clip_norm_g=1.0))
        _step(model, batches[0], 1)
        names = _kernel_names(model, batches[1], 2)
        assert {k for k, forms in NEW_KERNELS.items() if _launched(names, forms)} == want
        assert not _launched(names, PLAIN_ADAM)
