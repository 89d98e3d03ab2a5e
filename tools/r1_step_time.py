#!/usr/bin/env python3
"""What the lazily applied R1 penalty adds to the adversarial step.

  python tools/r1_step_time.py [--gan-type wgan_softplus] [--r1-reg-weight 10] [--torch-d] [--steps 10] [--warmup 3] [--out FILE.json]

One configuration per process -- run the settings in fresh processes, interleaved, in one session (the protocol of
tools/update_step_time.py).  MultiRefRestorationModel at B = 4, K = 5, LR 32 x 32 with StyleGAN2Discriminator(128), no WGAN-GP:
  step_ms             optimize_parameters, every step regularised when --r1-reg-weight > 0 (net_d_reg_every 1)
  d_step_ms           _discriminator_step alone on net_g's detached output (the same: regularised when R1 is on)
  d_step_launches     kernels of one such D step (torch profiler), and with R1 on the time of each launch of csrc/gan_reg.hip's kernels
--r1-reg-weight 0 --gan-type wgan is what the tree could do before wgan_softplus and R1 existed.  --torch-d: the discriminator's
forward replaced by the module tree on torch / MIOpen autograd (tools/gan_step_time.py's counterpart), the same R1 lines on it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gan-type', default='wgan_softplus')
    ap.add_argument('--r1-reg-weight', type=float, default=10.0)
    ap.add_argument('--torch-d', action='store_true')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out')
    a = ap.parse_args()
    import torch
    import gan_step_time as G
    torch.cuda.set_device(0)
    G.GAN['r1'] = dict(gan_type=a.gan_type, gan_weight=1e-3, grad_penalty_weight=0.0)
    if a.r1_reg_weight > 0:
        G.GAN['r1'].update(r1_reg_weight=a.r1_reg_weight, net_d_reg_every=1)
    model = G._model('r1', 'StyleGAN2Discriminator', 32)
    if a.torch_d:
        model.net_d.forward = G._torch_d(model.net_d)
    it = [0]

    def step():
        it[0] += 1
        model.optimize_parameters(it[0])
    res = dict(gan_type=a.gan_type, r1_reg_weight=a.r1_reg_weight, torch_d=a.torch_d, step_ms=G._median_ms(step, a.steps, a.warmup))
    with torch.no_grad():
        model.output = model._forward()

    def d_step():
        model._discriminator_step(1)
    res['d_step_ms'] = G._median_ms(d_step, a.steps, a.warmup)
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        d_step()
        torch.cuda.synchronize()
    events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    res['d_step_launches'] = len(events)
    res['d_step_kernel_ms'] = sum(e.device_time for e in events) / 1e3
    res['r1_kernels_us'] = {k: [e.device_time for e in events if k in e.name]
                            for k in ('r1_sqnorm_partial_kernel', 'r1_sqnorm_finalize_kernel', 'r1_sqnorm_bwd_kernel')}
    res['log'] = {k: v for k, v in model.get_current_log().items() if k.startswith('l_d')}
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
