"""Synthetic ImageDiscriminator weights shared by tests/golden/gen_golden_gan.py and the GPU tests: synth.state_dict(spec), with
the BatchNorm layers moved to the ranges the reference's initialisation gives them (weight N(1, 0.02), positive running
variance, num_batches_tracked 0)."""
import numpy as np

import synth


def state_dict(spec, seed=0):
    sd = synth.state_dict(spec, seed)
    bn = {k.rsplit('.', 1)[0] for k, _ in spec if k.endswith('running_mean')}
    for p in bn:
        sd[p + '.weight'] = (1.0 + sd[p + '.weight']).astype(np.float32)
        sd[p + '.running_var'] = (1.0 + np.abs(sd[p + '.running_var'])).astype(np.float32)
        sd[p + '.num_batches_tracked'] = np.array(0, np.int64)
    return sd
