"""Synthetic VGGStyleDiscriminator weights shared by tests/golden/gen_golden_gan_vgg.py and the GPU tests: synth_disc.state_dict(spec)
(BatchNorm layers in the ranges of their default initialisation), with the linear layers' weights rescaled to sigma 1 / sqrt(fan_in).
synth.state_dict gives every 2-D tensor sigma 0.05, which at linear1's fan-in of num_feat * 8 * 25 (12 800 at num_feat 64) would make
the hidden layer O(5)."""
import numpy as np

import synth_disc


def state_dict(spec, seed=0):
    sd = synth_disc.state_dict(spec, seed)
    for key, shape in spec:
        if key.startswith('linear') and key.endswith('.weight'):
            fan_in = int(shape[1])
            sd[key] = (sd[key] * ((1.0 / fan_in)**0.5 / 0.05)).astype(np.float32)
    return sd
