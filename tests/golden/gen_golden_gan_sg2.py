#!/usr/bin/env python3
"""Generate tests/golden/e2e_c2_gan_sg2.npz and e2e_c2_gan_sg2_vanilla.npz: gen_golden_gan.py's two adversarial steps of the
reference's own MultiRefRestorationModel (B = 4, K = 5, LR 32 x 32 -> GT 128 x 128) with StyleGAN2Discriminator(out_size 128) as
net_d (basicsr/archs/stylegan2_arch.py:733-799; channel_multiplier, resample_kernel, stddev_group and narrow at their defaults).

    e2e_c2_gan_sg2:          gan_type wgan, gan_weight 1e-3, grad_penalty_weight 10: one optimize_parameters(1)
    e2e_c2_gan_sg2_vanilla:  gan_type vanilla, no penalty, net_d_steps 2: optimize_parameters(1) (D only) and (2) (D and G)

Both record what gen_golden_gan_unet.py records (logs, alphas, D / G gradient fingerprints, parameter sums, the net_d spec) except the
spectral-norm buffers (this discriminator has no buffer at all).  net_d takes synth_sg2disc.state_dict(spec) weights.
e2e_c2_gan_sg2.npz also holds init_names / init_sha256: the sha256 of every state_dict tensor of the reference's
StyleGAN2Discriminator(128) built right after torch.manual_seed(0).

The reference's FusedLeakyReLU calls a compiled extension (fused_act_ext.fused_bias_act) that exists for CUDA only and has no CPU
fallback; this file binds that one name to fused_bias_act below, written from the operator's definition.  The reference's upfirdn2d
has its own CPU path (upfirdn2d_native), and gen() asserts that it was taken.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_gan_sg2.py
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import gen_golden_gan as GG  # noqa: E402
import synth  # noqa: E402
import synth_sg2disc  # noqa: E402

R = G.R
LR = 32
NETWORK_D = dict(type='StyleGAN2Discriminator', out_size=4 * LR)
CONFIGS = {
    'e2e_c2_gan_sg2': GG.CONFIGS['e2e_c2_gan'],
    'e2e_c2_gan_sg2_vanilla': GG.CONFIGS['e2e_c2_gan_vanilla'],
}


def fused_bias_act(input, bias, refer, act, grad, alpha, scale):
    """act 3 (leaky ReLU) of the fused operator.  grad 0: scale * lrelu(input + bias, alpha).  grad 1: the same gate applied to a
    gradient, taken from the sign of the forward's output `refer`: scale * (input + bias) where refer > 0, scale * alpha * (input +
    bias) elsewhere.  bias (may be empty) runs along dim 1."""
    assert act == 3 and grad in (0, 1)
    x = input
    if bias.numel():
        x = x + bias.view(1, -1, *([1] * (input.ndim - 2)))
    gate = x if grad == 0 else refer
    return torch.where(gate > 0, x, x * alpha) * scale


def ref_stylegan2():
    """the reference's stylegan2_arch with the stand-in bound; counts the calls of its CPU FIR path"""
    fa = R.ref_module('basicsr.ops.fused_act.fused_act')
    fa.fused_act_ext = types.SimpleNamespace(fused_bias_act=fused_bias_act)
    up = R.ref_module('basicsr.ops.upfirdn2d.upfirdn2d')
    if not hasattr(up, '_native_calls'):
        native = up.upfirdn2d_native
        up._native_calls = 0

        def counted(*a, **kw):
            up._native_calls += 1
            return native(*a, **kw)
        up.upfirdn2d_native = counted
    return R.ref_module('basicsr.archs.stylegan2_arch'), up


def init_hashes():
    """per-tensor sha256 of the reference's StyleGAN2Discriminator(128) state_dict under torch.manual_seed(0)"""
    sg, _ = ref_stylegan2()
    torch.manual_seed(0)
    net = sg.StyleGAN2Discriminator(4 * LR)
    names, hashes = [], []
    for k, v in net.state_dict().items():
        names.append(k)
        hashes.append(hashlib.sha256(np.ascontiguousarray(v.detach().cpu().numpy()).tobytes()).hexdigest())
    return dict(init_names=np.array(names), init_sha256=np.array(hashes))


def gen(name):
    """gen_golden_gan.gen with this file's discriminator; no buffers to record"""
    train_extra, steps = CONFIGS[name]
    mm = R.ref_module('basicsr.models.multi_ref_restoration_model')
    _, up = ref_stylegan2()   # registers StyleGAN2Discriminator
    init = mm.MultiRefRestorationModel.__init__

    def with_gan(self, opt):
        opt['network_d'] = dict(NETWORK_D)
        opt['path']['pretrain_network_d'] = None
        opt['train'].update(train_extra)
        init(self, opt)
    mm.MultiRefRestorationModel.__init__ = with_gan
    torch.set_grad_enabled(True)
    try:
        model, specs, data = G._build_model(True, 4, 5, LR, LR, 'e2e_c2')
    finally:
        mm.MultiRefRestorationModel.__init__ = init
    d_spec = G.spec_of(model.net_d)
    sd = synth_sg2disc.state_dict(d_spec)
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
    calls = up._native_calls
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
    assert up._native_calls > calls, 'the reference did not take its CPU upfirdn2d path'
    d_names, d_gsum, d_gabs, d_psum = GG._fingerprints(model.net_d)
    g_names, g_gsum, g_gabs, g_psum = GG._fingerprints(model.net_g)
    torch.set_grad_enabled(False)
    groups = [[float(g['lr']), len(g['params'])] for g in model.optimizer_g.param_groups]
    arrays.update(
        loss=np.array(arrays[f's{steps[-1]}_l_g_pix']), opt_groups=np.array(groups), b=np.array(4), k=np.array(5), lr_hw=np.array([LR, LR]),
        key=np.array('e2e_c2'), seed=np.array(GG.SEED), steps=np.array(steps),
        chk=np.array(synth.checksum(*[data[n].numpy() for n in ('img_in_lq', 'img_in_up', 'img_ref_list', 'img_in')])),
        gan_type=np.array(train_extra['gan_type']), gan_weight=np.array(train_extra['gan_weight']),
        grad_penalty_weight=np.array(train_extra['grad_penalty_weight']), net_d_steps=np.array(train_extra.get('net_d_steps', 1)),
        lr_d=np.array(train_extra['lr_d']),
        alpha=np.stack([a.numpy().reshape(-1) for a in alphas]) if alphas else np.zeros((0, 4), np.float32),
        d_param_names=np.array(d_names), d_grad_sum=d_gsum, d_grad_abs=d_gabs, d_param_sum_after=d_psum,
        param_names=np.array(g_names), grad_sum=g_gsum, grad_abs=g_gabs, param_sum_after=g_psum)
    for nm, spec in list(specs.items()) + [('net_d', d_spec)]:
        sa = G.spec_arrays(spec)
        arrays[f'{nm}_spec_keys'], arrays[f'{nm}_spec_shapes'] = sa['spec_keys'], sa['spec_shapes']
    if name == 'e2e_c2_gan_sg2':
        arrays.update(init_hashes())
    G.save(name, **arrays)


def main():
    for name in (sys.argv[1:] or CONFIGS):
        gen(name)


if __name__ == '__main__':
    main()
