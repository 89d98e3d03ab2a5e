"""Synthetic StyleGAN2Discriminator weights shared by tests/golden/gen_golden_gan_sg2.py and the GPU tests.  The network's
equalised learning rate multiplies every weight by 1 / sqrt(fan_in) when it is used, so the weights at rest are unit normal (the
distribution the reference's constructor draws them from) and D's output stays O(1); biases have sigma 0.02 (all zero after the
constructor, which would hide a wrong bias path)."""
import synth


def state_dict(spec, seed=0):
    out = {}
    for key, shape in spec:
        shape = tuple(int(s) for s in shape)
        out[key] = synth.randn(key, shape, seed, 0.02 if len(shape) == 1 else 1.0)
    return out
