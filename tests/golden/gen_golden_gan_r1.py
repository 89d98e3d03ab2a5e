#!/usr/bin/env python3
"""Generate tests/golden/e2e_c2_gan_sg2_r1.npz and gan_wgan_softplus.npz.

    e2e_c2_gan_sg2_r1:  gen_golden_gan_sg2.py's adversarial steps of the reference's own MultiRefRestorationModel (B = 4, K = 5,
                        LR 16 x 16 -> GT 64 x 64) with StyleGAN2Discriminator(out_size 64) as net_d, cri_gan the reference's
                        basicsr.losses.losses.GANLoss('wgan_softplus', loss_weight 1e-3) (losses.py:258-360), no gradient penalty,
                        and the lazily applied R1 penalty of basicsr/models/stylegan2_model.py:208-219 with r1_reg_weight 10 and
                        net_d_reg_every 2: optimize_parameters(1) (no R1) and (2) (R1).
    gan_wgan_softplus:  the reference GANLoss's constructor signature and its values and input gradients for gan_type wgan_softplus
                        (real / fake target, is_disc true / false, loss_weight 1 and 0.25) on a [4,1] and a [2,1,8,8] input.

The reference's multi-reference model has no R1 lines, so they are added around it: its optimizer_d.step is wrapped, and before the
real step of an iteration with step % net_d_reg_every == 0 the wrapper runs the reference's own r1_penalty (losses.py:391-405) on a
detached leaf copy of model.gt, forward and backward, in the order and with the weighting of stylegan2_model.py:208-219.  The gradients
that Adam then sees are the sum of both backward passes.  Recorded: what gen_golden_gan_sg2.py records, plus l_d_r1 (the weighted
penalty, .detach().mean(), as stylegan2_model.py:218 logs it) and r1_penalty (the unweighted value).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_gan_r1.py
"""
import inspect
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import gen_golden_gan as GG  # noqa: E402
import gen_golden_gan_sg2 as GS  # noqa: E402
import synth  # noqa: E402
import synth_sg2disc  # noqa: E402

R = G.R
LR = 16
NETWORK_D = dict(type='StyleGAN2Discriminator', out_size=4 * LR)
TRAIN = dict(gan_type='wgan', gan_weight=1e-3, grad_penalty_weight=0.0, lr_d=1e-4, beta_d=[0.9, 0.999])   # (cri_gan is replaced below)
R1_REG_WEIGHT, NET_D_REG_EVERY = 10.0, 2
STEPS = [1, 2]
LOG_KEYS = GG.LOG_KEYS + ('l_d_r1', 'r1_penalty')


def softplus_inputs():
    """the two inputs of the GANLoss cases: values on both sides of 0, some where softplus saturates"""
    a = synth.randn('gan_softplus/a', (4, 1)) * 3
    b = synth.randn('gan_softplus/b', (2, 1, 8, 8)) * 6
    return a.astype(np.float32), b.astype(np.float32)


def gen_softplus():
    L = R.ref_module('basicsr.losses.losses')
    sig = inspect.signature(L.GANLoss.__init__)
    arrays = dict(ctor_names=np.array(list(sig.parameters)),
                  ctor_defaults=np.array([repr(p.default) if p.default is not inspect.Parameter.empty else '' for p in sig.parameters.values()]))
    cases = []
    torch.set_grad_enabled(True)
    for xi, x in enumerate(softplus_inputs()):
        arrays[f'x{xi}'] = x
        for real in (True, False):
            for is_disc in (True, False):
                for w in (1.0, 0.25):
                    crit = L.GANLoss('wgan_softplus', loss_weight=w)
                    assert crit.get_target_label(torch.zeros(1), real) is real   # a bool label, as for wgan
                    t = torch.from_numpy(x).requires_grad_(True)
                    loss = crit(t, real, is_disc=is_disc)
                    grad, = torch.autograd.grad(loss, t)
                    key = f'x{xi}_real{int(real)}_disc{int(is_disc)}_w{w}'
                    cases.append(key)
                    arrays[key + '_loss'], arrays[key + '_grad'] = loss.detach().numpy(), grad.numpy()
    torch.set_grad_enabled(False)
    arrays['cases'] = np.array(cases)
    G.save('gan_wgan_softplus', **arrays)


def gen_r1(name='e2e_c2_gan_sg2_r1'):
    mm = R.ref_module('basicsr.models.multi_ref_restoration_model')
    L = R.ref_module('basicsr.losses.losses')
    _, up = GS.ref_stylegan2()   # registers StyleGAN2Discriminator
    init = mm.MultiRefRestorationModel.__init__

    def with_gan(self, opt):
        opt['network_d'] = dict(NETWORK_D)
        opt['path']['pretrain_network_d'] = None
        opt['train'].update(TRAIN)
        init(self, opt)
    mm.MultiRefRestorationModel.__init__ = with_gan
    torch.set_grad_enabled(True)
    try:
        model, specs, data = G._build_model(True, 4, 5, LR, LR, 'e2e_c2')
    finally:
        mm.MultiRefRestorationModel.__init__ = init
    model.cri_gan = L.GANLoss('wgan_softplus', real_label_val=1.0, fake_label_val=0.0, loss_weight=TRAIN['gan_weight'])
    assert model.cri_grad_penalty is None
    d_spec = G.spec_of(model.net_d)
    sd = synth_sg2disc.state_dict(d_spec)
    model.net_d.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model.feed_data(data)

    current = {}
    real_step = model.optimizer_d.step

    def step_with_r1(*a, **kw):
        if current['step'] % NET_D_REG_EVERY == 0:
            real_img = model.gt.detach().clone().requires_grad_(True)
            real_pred = model.net_d(real_img)
            penalty = L.r1_penalty(real_pred, real_img)
            l_d_r1 = R1_REG_WEIGHT / 2 * penalty * NET_D_REG_EVERY + 0 * real_pred[0]
            model.log_dict['l_d_r1'] = l_d_r1.detach().mean()
            model.log_dict['r1_penalty'] = penalty.detach()
            l_d_r1.backward()
        return real_step(*a, **kw)
    model.optimizer_d.step = step_with_r1

    arrays = {}
    calls = up._native_calls
    torch.manual_seed(GG.SEED)
    for step in STEPS:
        current['step'] = step
        model.log_dict.clear()
        model.optimize_parameters(step)
        logs = {k: float(model.log_dict[k]) for k in LOG_KEYS if k in model.log_dict}
        print(name, 'step', step, logs)
        for k, v in logs.items():
            arrays[f's{step}_{k}'] = np.array(v)
        arrays[f's{step}_log_keys'] = np.array(sorted(logs))
    assert up._native_calls > calls, 'the reference did not take its CPU upfirdn2d path'
    assert 'l_d_r1' not in arrays['s1_log_keys'] and 'l_d_r1' in arrays['s2_log_keys']
    d_names, d_gsum, d_gabs, d_psum = GG._fingerprints(model.net_d)
    g_names, g_gsum, g_gabs, g_psum = GG._fingerprints(model.net_g)
    torch.set_grad_enabled(False)
    groups = [[float(g['lr']), len(g['params'])] for g in model.optimizer_g.param_groups]
    arrays.update(
        loss=np.array(arrays[f's{STEPS[-1]}_l_g_pix']), opt_groups=np.array(groups), b=np.array(4), k=np.array(5), lr_hw=np.array([LR, LR]),
        key=np.array('e2e_c2'), seed=np.array(GG.SEED), steps=np.array(STEPS),
        chk=np.array(synth.checksum(*[data[n].numpy() for n in ('img_in_lq', 'img_in_up', 'img_ref_list', 'img_in')])),
        gan_type=np.array('wgan_softplus'), gan_weight=np.array(TRAIN['gan_weight']), grad_penalty_weight=np.array(0.0),
        net_d_steps=np.array(1), lr_d=np.array(TRAIN['lr_d']), r1_reg_weight=np.array(R1_REG_WEIGHT), net_d_reg_every=np.array(NET_D_REG_EVERY),
        d_param_names=np.array(d_names), d_grad_sum=d_gsum, d_grad_abs=d_gabs, d_param_sum_after=d_psum,
        param_names=np.array(g_names), grad_sum=g_gsum, grad_abs=g_gabs, param_sum_after=g_psum)
    for nm, spec in list(specs.items()) + [('net_d', d_spec)]:
        sa = G.spec_arrays(spec)
        arrays[f'{nm}_spec_keys'], arrays[f'{nm}_spec_shapes'] = sa['spec_keys'], sa['spec_shapes']
    G.save(name, **arrays)


def main():
    assert R.available(), 'reference tree not present: run in the build container'
    which = sys.argv[1:] or ['softplus', 'r1']
    if 'softplus' in which:
        gen_softplus()
    if 'r1' in which:
        gen_r1()


if __name__ == '__main__':
    main()
