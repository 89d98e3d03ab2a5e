#!/usr/bin/env python3
"""Generate tests/golden/e2e_c2_gan.npz and e2e_c2_gan_vanilla.npz: the reference's own MultiRefRestorationModel.optimize_parameters
at BASELINE configs[2]'s per-GPU shape (B = 4, K = 5, LR 40 x 40 -> GT 160 x 160) with an ImageDiscriminator(3, 32) next to the
L1 pixel loss (basicsr/models/multi_ref_restoration_model.py:98-113, 149-185, 219-278; basicsr/archs/discriminator_arch.py:10-45;
basicsr/models/losses.py:275-427).

    e2e_c2_gan:          gan_type wgan, gan_weight 1e-3, grad_penalty_weight 10: one optimize_parameters(1)
    e2e_c2_gan_vanilla:  gan_type vanilla, no penalty, net_d_steps 2: optimize_parameters(1) (D only) and (2) (D and G)

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_gan.py
The three generator-side nets are built and loaded exactly as gen_golden._build_model does (synthetic weights, the inputs of
e2e_c2); net_d takes synth_disc.state_dict(spec) weights, and its spec is stored so the GPU test rebuilds it without the reference.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import synth  # noqa: E402
import synth_disc  # noqa: E402

R = G.R
SEED = 1234
NETWORK_D = dict(type='ImageDiscriminator', in_nc=3, ndf=32)
CONFIGS = {
    'e2e_c2_gan': (dict(gan_type='wgan', gan_weight=1e-3, grad_penalty_weight=10.0, lr_d=1e-4, beta_d=[0.9, 0.999]), [1]),
    'e2e_c2_gan_vanilla': (dict(gan_type='vanilla', gan_weight=1e-3, grad_penalty_weight=0.0, lr_d=1e-4, beta_d=[0.9, 0.999],
                                net_d_steps=2), [1, 2]),
}
LOG_KEYS = ('l_d_real', 'out_d_real', 'l_d_fake', 'out_d_fake', 'l_grad_penalty', 'l_g_pix', 'l_g_gan')


def _fingerprints(net):
    names, gsum, gabs, psum = [], [], [], []
    for n, p in net.named_parameters():
        names.append(n)
        g = p.grad.detach().double() if p.grad is not None else torch.zeros(1, dtype=torch.float64)
        gsum.append(float(g.sum()))
        gabs.append(float(g.abs().sum()))
        psum.append(float(p.detach().double().sum()))
    return names, np.array(gsum), np.array(gabs), np.array(psum)


def gen(name):
    train_extra, steps = CONFIGS[name]
    mm = R.ref_module('basicsr.models.multi_ref_restoration_model')
    R.ref_module('basicsr.archs.discriminator_arch')   # registers ImageDiscriminator
    init = mm.MultiRefRestorationModel.__init__

    def with_gan(self, opt):
        opt['network_d'] = dict(NETWORK_D)
        opt['path']['pretrain_network_d'] = None
        opt['train'].update(train_extra)
        init(self, opt)
    mm.MultiRefRestorationModel.__init__ = with_gan
    torch.set_grad_enabled(True)
    try:
        model, specs, data = G._build_model(True, 4, 5, 40, 40, 'e2e_c2')
    finally:
        mm.MultiRefRestorationModel.__init__ = init
    d_spec = G.spec_of(model.net_d)
    sd = synth_disc.state_dict(d_spec)
    model.net_d.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model.feed_data(data)
    alphas = []
    rand = torch.rand

    def rec_rand(*a, **kw):
        t = rand(*a, **kw)
        alphas.append(t.clone())
        return t
    torch.rand = rec_rand
    arrays = {}
    try:
        torch.manual_seed(SEED)
        for step in steps:
            model.log_dict.clear()
            model.optimize_parameters(step)
            logs = {k: float(model.log_dict[k]) for k in LOG_KEYS if k in model.log_dict}
            print(name, 'step', step, logs)
            for k, v in logs.items():
                arrays[f's{step}_{k}'] = np.array(v)
            arrays[f's{step}_log_keys'] = np.array(sorted(logs))
    finally:
        torch.rand = rand
    d_names, d_gsum, d_gabs, d_psum = _fingerprints(model.net_d)
    g_names, g_gsum, g_gabs, g_psum = _fingerprints(model.net_g)
    bn = [(n, m) for n, m in model.net_d.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]
    torch.set_grad_enabled(False)
    groups = [[float(g['lr']), len(g['params'])] for g in model.optimizer_g.param_groups]
    arrays.update(
        loss=np.array(arrays[f's{steps[-1]}_l_g_pix']), opt_groups=np.array(groups), b=np.array(4), k=np.array(5), lr_hw=np.array([40, 40]), key=np.array('e2e_c2'), seed=np.array(SEED), steps=np.array(steps),
        chk=np.array(synth.checksum(*[data[n].numpy() for n in ('img_in_lq', 'img_in_up', 'img_ref_list', 'img_in')])),
        gan_type=np.array(train_extra['gan_type']), gan_weight=np.array(train_extra['gan_weight']),
        grad_penalty_weight=np.array(train_extra['grad_penalty_weight']), net_d_steps=np.array(train_extra.get('net_d_steps', 1)),
        lr_d=np.array(train_extra['lr_d']),
        alpha=np.stack([a.numpy().reshape(-1) for a in alphas]) if alphas else np.zeros((0, 4), np.float32),
        d_param_names=np.array(d_names), d_grad_sum=d_gsum, d_grad_abs=d_gabs, d_param_sum_after=d_psum,
        param_names=np.array(g_names), grad_sum=g_gsum, grad_abs=g_gabs, param_sum_after=g_psum,
        bn_names=np.array([n for n, _ in bn]), bn_running_mean=np.concatenate([m.running_mean.numpy() for _, m in bn]),
        bn_running_var=np.concatenate([m.running_var.numpy() for _, m in bn]),
        bn_num_batches_tracked=np.array([int(m.num_batches_tracked) for _, m in bn]))
    for nm, spec in list(specs.items()) + [('net_d', d_spec)]:
        sa = G.spec_arrays(spec)
        arrays[f'{nm}_spec_keys'], arrays[f'{nm}_spec_shapes'] = sa['spec_keys'], sa['spec_shapes']
    G.save(name, **arrays)


def main():
    for name in (sys.argv[1:] or CONFIGS):
        gen(name)


if __name__ == '__main__':
    main()
