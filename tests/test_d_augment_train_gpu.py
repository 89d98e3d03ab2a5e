"""GPU: train.d_augment in whole steps of MultiRefRestorationModel -- the small model of the GAN train tests (two residual blocks,
B = 2, K = 2, GT 64 x 64).

  a. option absent: the launches of before, none of the new kernels
  b. p: 0 with the full policy: the plain step's bits (ImageDiscriminator with wgan + gradient penalty, StyleGAN2Discriminator(64)
     with wgan_softplus + R1 on every step)
  c. p: 1: D's parameter gradients and d l_g_gan / d output against float64 autograd of test_disc_train_gpu.py's float64
     discriminator composed with d_augment_torch on the tables the model drew, under that file's gates (1e-3 / 1e-4)
  d. two fresh runs from one seed give the same bits;  e. adaptive p."""
import numpy as np
import pytest
import torch

import synth_disc
import test_disc_train_gpu as T_IMG
from test_disc_train_gpu import _rel
from test_optim_train_gpu import _model
from test_r1_train_gpu import SG2_64, _batch, _kernel_names, _small

pytestmark = pytest.mark.gpu

DEV = 'cuda'
IMG = dict(type='ImageDiscriminator', in_nc=3, ndf=32)
WGAN_GP = dict(gan_type='wgan', grad_penalty_weight=10.0, deterministic=True)
SOFTPLUS_R1 = dict(gan_type='wgan_softplus', r1_reg_weight=10.0, net_d_reg_every=1, deterministic=True)
FULL = ['color', 'translation', 'cutout', 'flip']
SOFTPLUS = dict(gan_type='wgan_softplus', deterministic=True)


@pytest.fixture(scope='module')
def data():
    return _batch()


def _img_model(extra):
    """_small with an ImageDiscriminator holding test_disc_train_gpu's synthetic weights -> (model, those weights)"""
    model = _model(dict(gan_weight=1e-3, lr_d=1e-4, beta_d=[0.9, 0.999], net_d_steps=1, **extra), network_d=dict(IMG))
    net = model.get_bare_model(model.net_d)
    sd = synth_disc.state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()])
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model, sd


def _step(model, data, seed=7):
    model.feed_data(data)
    torch.manual_seed(seed)   # (the penalty's alpha)
    model.optimize_parameters(1)
    torch.cuda.synchronize()
    grads = {f'{which}.{n}': p.grad.detach().clone() for which in ('net_d', 'net_g')
             for n, p in model.get_bare_model(getattr(model, which)).named_parameters() if p.grad is not None}
    return model.get_current_log(), grads


# ------------------------------------------------------------------ a. option absent
def test_option_absent_the_step_launches_what_it_launched(data, monkeypatch):
    """the construction of test_r1_train_gpu.py's test of the same name, its nhwc_train scale-cache reset included: the kernel list of
    a wgan + WGAN-GP step equals that of a step during which the new wrappers, the sampler and the autograd entry raise"""
    from mrefsr_amd import hip
    from mrefsr_amd.archs import d_augment as da
    from mrefsr_amd.archs import nhwc_train

    def traced():
        nhwc_train.reset_scales()
        monkeypatch.setattr(nhwc_train._scales, 'checks', 0)
        torch.manual_seed(11)
        model = _small(WGAN_GP)
        model.feed_data(data)
        model.optimize_parameters(1)
        torch.manual_seed(12)
        return model, _kernel_names(model, data, 2)
    model, names = traced()
    assert model.d_augment is None and model._d is model.net_d          # the same object is called and passed
    assert len(names) > 100 and not [n for n in names if 'disc_augment' in n]

    def gone(*a, **kw):
        raise AssertionError('the augmentation path was taken with its option absent')
    for mod, name in ((hip, 'disc_augment'), (hip, 'disc_augment_adj'), (da, 'sample_d_augment'), (da, 'd_augment')):
        monkeypatch.setattr(mod, name, gone)
    _, without = traced()
    assert names == without
    monkeypatch.undo()
    # (the names do show with the option on: a D step with WGAN-GP and the G step make four calls, each with its backward)
    model = _small(dict(WGAN_GP, d_augment=dict(policy=FULL, p=1.0)))
    model.feed_data(data)
    model.optimize_parameters(1)
    on = _kernel_names(model, data, 2)
    assert sum('disc_augment_fwd_kernel' in n for n in on) >= 4 and sum('disc_augment_adj_kernel' in n for n in on) >= 2


# ------------------------------------------------------------------ b. p: 0
@pytest.mark.parametrize('which', ['image_wgan_gp', 'sg2_softplus_r1'])
def test_p0_reproduces_the_plain_step_bit_for_bit(which, data):
    def build(extra):
        if which == 'image_wgan_gp':
            return _img_model(dict(WGAN_GP, **extra))[0]
        return _small(dict(SOFTPLUS_R1, **extra), network_d=SG2_64)
    plain_log, plain = _step(build({}), data)
    model = build(dict(d_augment=dict(policy=FULL, p=0)))
    log, grads = _step(model, data)
    assert model.d_augment is not None and model._d == model._d_augmented
    assert ('l_grad_penalty' if which == 'image_wgan_gp' else 'l_d_r1') in log and 'l_g_gan' in log
    assert log == plain_log, (log, plain_log)
    assert sorted(grads) == sorted(plain) and len([k for k in grads if k.startswith('net_d.')]) > 10
    for k in grads:
        assert torch.equal(grads[k], plain[k]), k


# ------------------------------------------------------------------ c. p: 1 against float64
@pytest.fixture(scope='module')
def p1_run(data):
    """one step with p: 1 (ImageDiscriminator, wgan + gradient penalty, manual_seed 10), the tables it drew and the LeakyReLU masks
    of its discriminator forwards: shared, not modified"""
    from mrefsr_amd.archs import d_augment as da
    mp = pytest.MonkeyPatch()
    try:
        masks = T_IMG._record_masks(mp)
        tables, real = [], da.sample_d_augment

        def sampler(*a, **kw):
            tables.append(real(*a, **kw))
            return tables[-1]
        mp.setattr(da, 'sample_d_augment', sampler)
        model, sd = _img_model(dict(WGAN_GP, d_augment=dict(policy=FULL, p=1.0)))
        log, grads = _step(model, data)
        # the G step's call once more, on the tables it drew: d l_g_gan / d output (D after its update, its parameters frozen)
        out = model.output.detach().clone().requires_grad_(True)
        l_g_gan = model.cri_gan(model.net_d(da.d_augment(out, tables[3].to(DEV))), True, is_disc=False)
        g_out, = torch.autograd.grad(l_g_gan, out)
        sd_after = {k: v.detach().cpu().clone() for k, v in model.get_bare_model(model.net_d).state_dict().items()}
        return dict(log=log, grads=grads, tables=list(tables), masks=[m.clone() for m in masks], sd=sd, sd_after=sd_after,
                    real=model._gt_for('gan').detach().cpu(), fake=model.output.detach().cpu(), g_out=g_out.cpu(),
                    l_g_gan=float(l_g_gan.detach()))
    finally:
        mp.undo()


def test_p1_step_vs_float64(p1_run):
    from mrefsr_amd.archs import d_augment as da
    r = p1_run
    tables, masks = r['tables'], r['masks']
    assert len(tables) == 4 and len(masks) == 50    # real, fake, interpolate, G step; ten BatchNorm layers per forward (+ the re-run)
    assert all(t.contrast for t in tables) and all(not torch.equal(tables[0].packed, t.packed) for t in tables[1:])   # independent draws
    b = r['real'].shape[0]
    real, fake = r['real'].double(), r['fake'].double()
    names = [n for n in r['grads'] if n.startswith('net_d.')]
    sd64 = {k: torch.from_numpy(np.asarray(v)).double().requires_grad_(f'net_d.{k}' in names) for k, v in r['sd'].items()}

    def D(x, table, m):
        return T_IMG._ref_forward(sd64, da.d_augment_torch(x, table), m)
    # the D step: -mean D(T0 real) + mean D(T1 fake) + 10 gradient_penalty(D o T2), the gradient taken towards the interpolate
    l_d = -D(real, tables[0], masks[0:10]).mean() + D(fake, tables[1], masks[10:20]).mean()
    torch.manual_seed(7)
    alpha = torch.rand(b, 1, 1, 1).double()
    xi = (alpha * real + (1 - alpha) * fake).requires_grad_(True)
    di = D(xi, tables[2], masks[20:30])
    gi, = torch.autograd.grad(di, xi, torch.ones_like(di), create_graph=True)
    pen = 10.0 * ((gi.view(b, -1).norm(2, dim=1) - 1) ** 2).mean()
    (l_d + pen).backward()
    log = r['log']
    print(f'\n[d_augment p=1] l_grad_penalty {log["l_grad_penalty"]:.6g} (float64 {pen.item():.6g})  l_d_real + l_d_fake '
          f'{log["l_d_real"] + log["l_d_fake"]:.6g} (float64 {l_d.item():.6g})')
    assert abs(log['l_grad_penalty'] - pen.item()) <= 1e-4 * abs(pen.item())
    worst = {}
    for n in names:
        k = n[len('net_d.'):]
        if T_IMG._bias_before_bn(k):    # analytically 0 (rounding noise on both sides), the rule of test_disc_train_gpu.py
            wg = r['grads'][n[:-4] + 'weight']
            assert r['grads'][n].abs().max().item() <= 1e-4 * wg.abs().max().item(), n
            continue
        worst[k] = _rel(r['grads'][n], sd64[k].grad)
    key = max(worst, key=worst.get)
    print(f'[d_augment p=1] worst D parameter gradient {worst[key]:.2e} ({key}) of {len(worst)}; gate 1e-3')
    # the G step's term, D after its Adam update
    sd64 = {k: v.double() for k, v in r['sd_after'].items()}
    out = fake.clone().requires_grad_(True)
    l_g = -1e-3 * D(out, tables[3], masks[40:50]).mean()
    want, = torch.autograd.grad(l_g, out)
    err = _rel(r['g_out'], want)
    print(f'[d_augment p=1] l_g_gan {r["l_g_gan"]:.6g} (float64 {l_g.item():.6g})  d l_g_gan / d output {err:.2e}; gate 1e-4')
    assert abs(r['l_g_gan'] - log['l_g_gan']) <= 1e-6 * abs(log['l_g_gan'])     # the re-run is the G step's call
    assert float(want.abs().max()) > 0
    assert not {k: v for k, v in worst.items() if v > 1e-3}, {k: v for k, v in worst.items() if v > 1e-3}
    assert err <= 1e-4, err


# ------------------------------------------------------------------ d. reproducibility
def test_two_fresh_runs_from_one_seed_give_the_same_bits(data, p1_run):
    model, _ = _img_model(dict(WGAN_GP, d_augment=dict(policy=FULL, p=1.0)))
    log, grads = _step(model, data)
    assert log == p1_run['log']
    for k in grads:
        assert torch.equal(grads[k], p1_run['grads'][k]), k


# ------------------------------------------------------------------ e. adaptive p
@pytest.mark.parametrize('target,want', [(2.0, [0.5, 0.25, 0.25, 0.0, 0.0, 0.0]), (-2.0, [0.5, 0.75, 0.75, 1.0, 1.0, 1.0])])
def test_adaptive_p_moves_by_count_over_speed_and_clamps(target, want, data):
    """interval 2, B = 2: 4 images per interval, speed_kimg 0.016 -> steps of exactly 4 / 16; sign(D) lies in [-1, 1], so a target
    of 2 is never met (p falls) and one of -2 always exceeded (p rises)"""
    model = _small(dict(SOFTPLUS, d_augment=dict(policy=FULL, p=0.5, adaptive=dict(target=target, interval=2, speed_kimg=0.016))),
                   network_d=SG2_64)
    reads, real = [], model.d_adaptive.read

    def counted():
        reads.append(1)
        return real()
    model.d_adaptive.read = counted
    model.feed_data(data)
    seen = []
    for step in range(1, 7):
        model.optimize_parameters(step)
        log = model.get_current_log()
        seen.append(log['d_aug_p'])
        assert len(reads) == step // 2                       # exactly one readback per interval
        assert ('d_aug_rt' in log) == (step >= 2)
        if step >= 2:
            assert -1.0 <= log['d_aug_rt'] <= 1.0
    assert seen == want
    state = model.d_adaptive.state_dict()
    assert state['p'] == want[-1] and state['steps'] == 6 and state['acc'] is None


def test_adaptive_state_is_saved_and_restored(data, tmp_path):
    opt = dict(SOFTPLUS, d_augment=dict(policy=FULL, p=0.5, adaptive=dict(target=-2.0, interval=2, speed_kimg=0.016)))
    model = _small(opt, network_d=SG2_64)
    model.opt['path']['training_states'] = str(tmp_path)
    model.feed_data(data)
    for step in (1, 2, 3):
        model.optimize_parameters(step)
    model.save_training_state(0, 3)
    state = torch.load(tmp_path / '3.state', weights_only=False)
    assert state['d_augment']['p'] == 0.75 and state['d_augment']['steps'] == 3 and state['d_augment']['acc'][1] == 2.0
    twin = _small(opt, network_d=SG2_64)
    assert twin.d_adaptive.p == 0.5
    twin.resume_training(state)
    assert twin.d_adaptive.p == 0.75 and twin.d_adaptive.steps == 3 and twin.d_adaptive.acc.tolist() == state['d_augment']['acc']
    del state['d_augment']                                   # a state file from before the option: the option's p
    older = _small(opt, network_d=SG2_64)
    older.resume_training(state)
    assert older.d_adaptive.p == 0.5 and older.d_adaptive.acc is None


def test_refusals_at_construction():
    with pytest.raises(ValueError, match='wgan'):
        _small(dict(WGAN_GP, d_augment=dict(policy=FULL, adaptive={})))
    with pytest.raises(ValueError, match='rotate'):
        _small(dict(WGAN_GP, d_augment=dict(policy=['rotate'])))
    with pytest.raises(ValueError, match='network_d'):
        _model(dict(d_augment=dict(policy=FULL)))
