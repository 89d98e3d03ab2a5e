"""Inputs of the LDL artifact-loss tests (tests/test_ldl_loss_*.py) and of tests/golden/gen_golden_ldl.py: (out, gt, ema) fp32
[B,3,H,W], deterministic from a seed, in two classes

  generic   out = gt + 0.1 randn, ema = gt + 0.1 randn (``scales``: a noise scale per sample instead of 0.1)
  plateau   out = gt + 0.3 + 0.01 randn, ema alike: a large residual mean under a small local variance (a one-pass variance
            sum r^2 - (sum r)^2 / n in fp32 is wrong by about 1e-3 there)

both made so that the mask r >= r_e is not a rounding lottery: wherever |r - r_e| < 1e-3 (r = sum_c |gt - out|, r_e = sum_c
|gt - ema|, in fp32) ema is set to out at that pixel in all three channels -- an exact tie, which every precision keeps."""
import torch

CLASSES = ('generic', 'plateau')
GOLDEN_SHAPES = ((1, 4, 4), (1, 5, 6), (1, 7, 9), (3, 33, 17))


def make_inputs(cls, shape, seed, scales=None):
    g = torch.Generator().manual_seed(seed)
    b, h, w = shape
    gt = torch.rand(b, 3, h, w, generator=g)
    n_out, n_ema = torch.randn(b, 3, h, w, generator=g), torch.randn(b, 3, h, w, generator=g)
    if cls == 'generic':
        s = torch.tensor(scales if scales is not None else [0.1] * b, dtype=torch.float32).view(b, 1, 1, 1)
        out, ema = gt + s * n_out, gt + s * n_ema
    elif cls == 'plateau':
        out, ema = gt + 0.3 + 0.01 * n_out, gt + 0.3 + 0.01 * n_ema
    else:
        raise ValueError(cls)
    r, r_e = (gt - out).abs().sum(1, keepdim=True), (gt - ema).abs().sum(1, keepdim=True)
    ema = torch.where((r - r_e).abs() < 1e-3, out, ema)
    return out.contiguous(), gt.contiguous(), ema.contiguous()


def golden_key(cls, shape):
    return f'{cls}_{shape[0]}x{shape[1]}x{shape[2]}'
