"""Synthetic UNetDiscriminatorSN weights shared by tests/golden/gen_golden_gan_unet.py and the GPU tests: synth.state_dict(spec)
(He-scaled convolution weights, biases sigma 0.02), with every spectral-norm vector (weight_u, weight_v) scaled to unit length, as
torch.nn.utils.spectral_norm keeps them."""
import numpy as np

import synth


def state_dict(spec, seed=0):
    sd = synth.state_dict(spec, seed)
    for key, _ in spec:
        if key.endswith('.weight_u') or key.endswith('.weight_v'):
            v = sd[key].astype(np.float64)
            sd[key] = (v / np.linalg.norm(v)).astype(np.float32)
    return sd
