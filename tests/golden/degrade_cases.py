"""Inputs of the degradation tests (tests/test_degrade_*.py) and of tests/golden/gen_golden_degrade.py, deterministic from a seed.

image(): a smooth sinusoid image plus N(0, noise), clamped to [0, 1] -- smooth enough that JPEG coefficients and USM residuals stay
away from their rounding cliffs for all but a few positions (the generator asserts how few).
chain_plan(): the fixed plan of the golden chain (Gaussian noise in both stages, mixed gray flags)."""
import numpy as np
import torch

FILTER_SHAPE = (2, 3, 23, 37)
USM_CASES = {'usm_32x40': (2, 32, 40, 0.02, 11), 'usm_40x56': (2, 40, 56, 0.02, 12)}                 # b, h, w, noise, seed
JPEG_CASES = {'jpeg_40x56': (2, 40, 56, 0.02, 21, (40.0, 85.0)), 'jpeg_33x47': (2, 33, 47, 0.02, 22, (55.0, 75.0))}
CHAIN_GT = (2, 48, 64)
KERNEL_CASES = {
    'k_iso': ('iso', 21, 2.3, 2.3, 0.0, 1.0), 'k_aniso': ('aniso', 15, 2.9, 0.7, 0.6, 1.0),
    'k_giso': ('generalized_iso', 13, 1.7, 1.7, 0.0, 0.8), 'k_ganiso': ('generalized_aniso', 21, 2.5, 1.1, -1.2, 2.5),
    'k_piso': ('plateau_iso', 17, 1.9, 1.9, 0.0, 1.6), 'k_paniso': ('plateau_aniso', 9, 2.2, 0.9, 2.1, 1.3),
}
SINC_CASES = {'k_sinc13': (1.3, 13, 0), 'k_sinc7pad': (2.6, 7, 21), 'k_sinc21': (0.9, 21, 21)}     # cutoff, size, pad_to


def image(b, h, w, noise, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
    x = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w)
    phase = torch.rand(b, 3, 1, 1, generator=g) * 6.28
    fy, fx = 0.05 + 0.1 * torch.rand(b, 3, 1, 1, generator=g), 0.05 + 0.1 * torch.rand(b, 3, 1, 1, generator=g)
    img = 0.5 + 0.35 * torch.sin(fy * y + phase) * torch.cos(fx * x - phase)
    return (img + noise * torch.randn(b, 3, h, w, generator=g)).clamp(0, 1).contiguous()


def filter_kernels(seed=5):
    """[2,21,21] and [2,7,7] positive kernels of sum 1"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in (21, 7):
        t = torch.rand(2, k, k, generator=g) ** 3
        out.append((t / t.sum(dim=(1, 2), keepdim=True)).contiguous())
    return out


def chain_plan():
    """the golden chain's decisions as plain numbers (the kernels come from the golden file)"""
    return dict(resize1=(1.37, 'bilinear'), sigma1=np.array([12.0, 25.0], np.float32), gray1=np.array([1.0, 0.0], np.float32),
                jpeg1=np.array([60.0, 85.0], np.float32), second_blur=True, resize2=(0.8, 'bicubic'),
                sigma2=np.array([8.0, 17.0], np.float32), gray2=np.array([0.0, 1.0], np.float32), final_mode='area',
                resize_before_jpeg=True, jpeg2=np.array([70.0, 50.0], np.float32), scale=4, noise_seeds=(101, 202))


def golden_plan(golden):
    """the DegradationPlan of the golden chain, its stored noise draws included; golden: the arrays of degrade.npz"""
    from mrefsr_amd import degradation as D
    p = chain_plan()
    b, h, w = CHAIN_GT
    n1, n2 = torch.from_numpy(golden['chain_n1']), torch.from_numpy(golden['chain_n2'])
    ng1 = torch.from_numpy(golden['chain_ng1']).expand(b, 1, *n1.shape[2:])
    ng2 = torch.from_numpy(golden['chain_ng2']).expand(b, 1, *n2.shape[2:])
    return D.DegradationPlan(
        gt_hw=(h, w), scale=p['scale'], kernel1=golden['chain_kernel1'], kernel2=golden['chain_kernel2'], sinc_kernel=golden['chain_sinc'],
        resize1=p['resize1'], noise1=D.NoisePlan(False, p['sigma1'], p['gray1'], (n1, ng1)), jpeg1=p['jpeg1'], second_blur=p['second_blur'],
        resize2=p['resize2'], noise2=D.NoisePlan(False, p['sigma2'], p['gray2'], (n2, ng2)), final_mode=p['final_mode'],
        resize_before_jpeg=p['resize_before_jpeg'], jpeg2=p['jpeg2'])
