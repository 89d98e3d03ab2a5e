#!/usr/bin/env python3
"""Generate tests/golden/e2e_c2_gan_unet.npz and e2e_c2_gan_unet_vanilla.npz: gen_golden_gan.py's two adversarial steps of the
reference's own MultiRefRestorationModel (B = 4, K = 5, LR 40 x 40 -> GT 160 x 160) with UNetDiscriminatorSN(3, 64) as net_d
(basicsr/archs/discriminator_arch.py:127-200, skip_connection True).

    e2e_c2_gan_unet:          gan_type wgan, gan_weight 1e-3, grad_penalty_weight 10: one optimize_parameters(1)
    e2e_c2_gan_unet_vanilla:  gan_type vanilla, no penalty, net_d_steps 2: optimize_parameters(1) (D only) and (2) (D and G)

Both record what gen_golden_gan.py records (logs, alphas, D / G gradient fingerprints, parameter sums, the net_d spec) except the
BatchNorm statistics (this discriminator has none); instead sn_names / sn_u / sn_v hold every spectral-norm buffer after the step(s).
net_d takes synth_unetdisc.state_dict(spec) weights.  e2e_c2_gan_unet.npz also holds init_names / init_sha256: the sha256 of every
state_dict tensor of the reference's UNetDiscriminatorSN(3, 64) built right after torch.manual_seed(0).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_gan_unet.py
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import gen_golden_gan as GG  # noqa: E402
import synth  # noqa: E402
import synth_unetdisc  # noqa: E402

R = G.R
NETWORK_D = dict(type='UNetDiscriminatorSN', num_in_ch=3, num_feat=64, skip_connection=True)
CONFIGS = {
    'e2e_c2_gan_unet': GG.CONFIGS['e2e_c2_gan'],
    'e2e_c2_gan_unet_vanilla': GG.CONFIGS['e2e_c2_gan_vanilla'],
}


def init_hashes():
    """per-tensor sha256 of the reference's UNetDiscriminatorSN(3, 64) state_dict under torch.manual_seed(0)"""
    da = R.ref_module('basicsr.archs.discriminator_arch')
    torch.manual_seed(0)
    net = da.UNetDiscriminatorSN(3, 64)
    names, hashes = [], []
    for k, v in net.state_dict().items():
        names.append(k)
        hashes.append(hashlib.sha256(np.ascontiguousarray(v.detach().cpu().numpy()).tobytes()).hexdigest())
    return dict(init_names=np.array(names), init_sha256=np.array(hashes))


def gen(name):
    """gen_golden_gan.gen with this file's discriminator, recording the spectral-norm buffers instead of BatchNorm statistics"""
    train_extra, steps = CONFIGS[name]
    mm = R.ref_module('basicsr.models.multi_ref_restoration_model')
    R.ref_module('basicsr.archs.discriminator_arch')   # registers UNetDiscriminatorSN_basicsr
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
    sd = synth_unetdisc.state_dict(d_spec)
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
        torch.manual_seed(GG.SEED)
        for step in steps:
            model.log_dict.clear()
            model.optimize_parameters(step)
            logs = {k: float(model.log_dict[k]) for k in GG.LOG_KEYS if k in model.log_dict}
            print(name, 'step', step, logs)
            for k, v in logs.items():
                arrays[f's{step}_{k}'] = np.array(v)
            arrays[f's{step}_log_keys'] = np.array(sorted(logs))
    finally:
        torch.rand = rand
    d_names, d_gsum, d_gabs, d_psum = GG._fingerprints(model.net_d)
    g_names, g_gsum, g_gabs, g_psum = GG._fingerprints(model.net_g)
    sn = [(n, m) for n, m in model.net_d.named_modules() if hasattr(m, 'weight_u')]
    torch.set_grad_enabled(False)
    groups = [[float(g['lr']), len(g['params'])] for g in model.optimizer_g.param_groups]
    arrays.update(
        loss=np.array(arrays[f's{steps[-1]}_l_g_pix']), opt_groups=np.array(groups), b=np.array(4), k=np.array(5), lr_hw=np.array([40, 40]),
        key=np.array('e2e_c2'), seed=np.array(GG.SEED), steps=np.array(steps),
        chk=np.array(synth.checksum(*[data[n].numpy() for n in ('img_in_lq', 'img_in_up', 'img_ref_list', 'img_in')])),
        gan_type=np.array(train_extra['gan_type']), gan_weight=np.array(train_extra['gan_weight']),
        grad_penalty_weight=np.array(train_extra['grad_penalty_weight']), net_d_steps=np.array(train_extra.get('net_d_steps', 1)),
        lr_d=np.array(train_extra['lr_d']),
        alpha=np.stack([a.numpy().reshape(-1) for a in alphas]) if alphas else np.zeros((0, 4), np.float32),
        d_param_names=np.array(d_names), d_grad_sum=d_gsum, d_grad_abs=d_gabs, d_param_sum_after=d_psum,
        param_names=np.array(g_names), grad_sum=g_gsum, grad_abs=g_gabs, param_sum_after=g_psum,
        sn_names=np.array([n for n, _ in sn]), sn_u=np.concatenate([m.weight_u.numpy() for _, m in sn]),
        sn_v=np.concatenate([m.weight_v.numpy() for _, m in sn]))
    for nm, spec in list(specs.items()) + [('net_d', d_spec)]:
        sa = G.spec_arrays(spec)
        arrays[f'{nm}_spec_keys'], arrays[f'{nm}_spec_shapes'] = sa['spec_keys'], sa['spec_shapes']
    if name == 'e2e_c2_gan_unet':
        arrays.update(init_hashes())
    G.save(name, **arrays)


def main():
    for name in (sys.argv[1:] or CONFIGS):
        gen(name)


if __name__ == '__main__':
    main()
