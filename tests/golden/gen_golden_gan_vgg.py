#!/usr/bin/env python3
"""Generate tests/golden/e2e_c2_gan_vgg.npz and e2e_c2_gan_vgg_vanilla.npz: gen_golden_gan.py's two adversarial steps of the
reference's own MultiRefRestorationModel (B = 4, K = 5, LR 40 x 40 -> GT 160 x 160) with VGGStyleDiscriminator(3, 64) as net_d
(basicsr/archs/discriminator_arch.py:47-125, input_size 160).

    e2e_c2_gan_vgg:          gan_type wgan, gan_weight 1e-3, grad_penalty_weight 10: one optimize_parameters(1)
    e2e_c2_gan_vgg_vanilla:  gan_type vanilla, no penalty, net_d_steps 2: optimize_parameters(1) (D only) and (2) (D and G)

Both record what gen_golden_gan.py records (logs, alphas, D / G gradient fingerprints, parameter sums, BatchNorm running statistics,
the net_d spec); net_d takes synth_vggdisc.state_dict(spec) weights.  e2e_c2_gan_vgg.npz also holds init_names / init_sha256: the
sha256 of every state_dict tensor of the reference's VGGStyleDiscriminator(3, 64) built right after torch.manual_seed(0).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_gan_vgg.py
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
import synth_vggdisc  # noqa: E402

NETWORK_D = dict(type='VGGStyleDiscriminator', num_in_ch=3, num_feat=64)
CONFIGS = {
    'e2e_c2_gan_vgg': GG.CONFIGS['e2e_c2_gan'],
    'e2e_c2_gan_vgg_vanilla': GG.CONFIGS['e2e_c2_gan_vanilla'],
}


def init_hashes():
    """per-tensor sha256 of the reference's VGGStyleDiscriminator(3, 64) state_dict under torch.manual_seed(0)"""
    da = G.R.ref_module('basicsr.archs.discriminator_arch')
    torch.manual_seed(0)
    net = da.VGGStyleDiscriminator(3, 64)
    names, hashes = [], []
    for k, v in net.state_dict().items():
        names.append(k)
        hashes.append(hashlib.sha256(np.ascontiguousarray(v.detach().cpu().numpy()).tobytes()).hexdigest())
    return dict(init_names=np.array(names), init_sha256=np.array(hashes))


def main():
    extra = init_hashes()
    save = G.save
    # gen_golden_gan.gen with this file's discriminator, weights and fixture names (its module globals are swapped for the call)
    GG.NETWORK_D, GG.CONFIGS, GG.synth_disc = NETWORK_D, CONFIGS, synth_vggdisc

    def save_with_init(name, **arrays):
        if name == 'e2e_c2_gan_vgg':
            arrays.update(extra)
        save(name, **arrays)
    G.save = save_with_init
    try:
        for name in (sys.argv[1:] or CONFIGS):
            GG.gen(name)
    finally:
        G.save = save


if __name__ == '__main__':
    main()
