"""GPU: the kernels of csrc/degrade.hip (through the hip.degrade_* wrappers) against the definitions of mrefsr_amd/degradation.py,
which tests/test_degrade_cpu.py ties to the reference's own functions.

Error bars are not fixed in advance.  Per case the yardstick is the definition evaluated in fp32 against the same in float64 (for
resize: F.interpolate on the GPU in both); the kernel may be FACTOR = 4 times as far from float64 as that, with a floor of one fp32
ulp of the value range [0, 1] (2^-23).  Both figures are printed.  USM and JPEG have rounding cliffs; what is left out of the
comparison, and the extra allowance, is derived in their tests."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import degrade_cases as cases

pytestmark = pytest.mark.gpu

FACTOR = 4.0
ULP = 2.0 ** -23
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'degrade.npz')


def bar(ref32, ref64):
    return max(FACTOR * float((ref32.double().cpu() - ref64.cpu()).abs().max()), ULP)


def check(name, out, ref32, ref64, extra=0.0, keep=None):
    err = (out.double().cpu() - ref64.cpu()).abs()
    if keep is not None:
        err = err * keep
    allowed = bar(ref32, ref64) + extra
    print(f'{name}: kernel {float(err.max()):.3e}  allowed {allowed:.3e} (yardstick {float((ref32.double().cpu() - ref64.cpu()).abs().max()):.3e})')
    assert float(err.max()) <= allowed, (name, float(err.max()), allowed)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


# ---------------------------------------------------------------------------------------------------------------- filter2d
@pytest.mark.parametrize('case', ['k21', 'k7', 'shared', 'h11', 'wide'])
def test_filter2d(case):
    from mrefsr_amd import degradation as D, hip
    k21, k7 = cases.filter_kernels()
    if case == 'h11':      # the smallest legal height for k = 21
        img, kern = cases.image(1, 11, 29, 0.05, 41), k21[:1]
    elif case == 'wide':   # more than one tile in both directions (16 x 64 pixels each)
        img, kern = cases.image(2, 35, 131, 0.05, 42), k21
    else:                  # 23 x 37: the halo is wider than half the tile, odd sizes
        img = cases.image(2, 23, 37, 0.05, 3)
        kern = {'k21': k21, 'k7': k7, 'shared': k21[:1]}[case]
    out = hip.degrade_filter2d(img.cuda(), kern.cuda())
    check(f'filter2d {case}', out, D.filter2d_torch(img, kern), D.filter2d_torch(img.double(), kern.double()))
    if case == 'k21':      # and the reference's own output
        assert float((out.cpu() - torch.from_numpy(golden()['filter_out21'])).abs().max()) <= 2 * bar(D.filter2d_torch(img, kern), D.filter2d_torch(img.double(), kern.double()))


def test_filter2d_delta_kernel_returns_the_input_bit_for_bit():
    from mrefsr_amd import hip
    img = cases.image(2, 23, 37, 0.05, 43).cuda()
    for k in (3, 21):
        delta = torch.zeros(2, k, k, device='cuda')
        delta[:, k // 2, k // 2] = 1
        assert torch.equal(hip.degrade_filter2d(img, delta), img)
    with pytest.raises(Exception, match='reflect'):
        hip.degrade_filter2d(img[:, :, :10].contiguous(), torch.zeros(2, 21, 21, device='cuda'))


# ---------------------------------------------------------------------------------------------------------------- resize
RESIZE_CASES = {
    'up_1.37': ((2, 3, 23, 37), dict(scale_factor=1.37)), 'down_0.41': ((2, 3, 23, 37), dict(scale_factor=0.41)),
    'identity': ((2, 3, 23, 37), dict(scale_factor=1.0)), 'size_9x10': ((1, 3, 37, 41), dict(size=(9, 10))),
    'factor_0.25': ((1, 3, 37, 41), dict(scale_factor=0.25)),   # also 9 x 10, but mapped by 4.0 where size maps by 37/9, 41/10
    'one_wide': ((1, 3, 19, 1), dict(size=(7, 3))), 'x4_10x12': ((2, 3, 10, 12), dict(scale_factor=4)),
}


# (the x4 case is the bicubic up-sampling of the model input: that mode only)
@pytest.mark.parametrize('case,mode', [(c, m) for c in sorted(RESIZE_CASES) for m in ('area', 'bilinear', 'bicubic')
                                       if c != 'x4_10x12' or m == 'bicubic'])
def test_resize(case, mode):
    from mrefsr_amd import hip
    shape, kw = RESIZE_CASES[case]
    img = cases.image(shape[0], shape[2], shape[3], 0.1, 50).cuda()
    out = hip.degrade_resize(img, mode=mode, **kw)
    ref32, ref64 = F.interpolate(img, mode=mode, **kw), F.interpolate(img.double(), mode=mode, **kw)
    assert out.shape == ref32.shape
    check(f'resize {case} {mode}', out, ref32, ref64)
    if case == 'identity':
        assert torch.equal(out, img)


def test_resize_by_size_and_by_factor_differ_as_torch_does():
    from mrefsr_amd import hip
    img = cases.image(1, 37, 41, 0.1, 50).cuda()
    a, b = hip.degrade_resize(img, size=(9, 10), mode='bicubic'), hip.degrade_resize(img, scale_factor=0.25, mode='bicubic')
    ra, rb = F.interpolate(img, size=(9, 10), mode='bicubic'), F.interpolate(img, scale_factor=0.25, mode='bicubic')
    assert a.shape == b.shape and float((ra - rb).abs().max()) > 1e-3 and float((a - b).abs().max()) > 1e-3
    assert float((a - ra).abs().max()) < 1e-5 and float((b - rb).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- levels, noise
def level_image(n, b=2, h=20, w=30, seed=0):
    """images whose three channels together hold exactly min(n, 256) distinct clamped levels; n = 257: values below 0 and above 1
    as well, which clamp onto levels 0 and 255"""
    g = torch.Generator().manual_seed(seed)
    lv = torch.randperm(256, generator=g)[:min(n, 256)].float()
    idx = torch.randint(0, len(lv), (b, 3, h, w), generator=g)
    idx.view(b, -1)[:, :len(lv)] = torch.arange(len(lv))   # every level at least once in every sample
    img = lv[idx] / 255.
    if n > 256:
        img.view(b, -1)[:, -2] = -0.3
        img.view(b, -1)[:, -1] = 1.7
    return img.contiguous()


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257])
def test_levels(n):
    from mrefsr_amd import degradation as D, hip
    img = level_image(n)
    img[1, :, 10:] = img[1, :, :1, :1]   # the second sample holds fewer levels than the first
    vals = hip.degrade_levels(img.cuda())
    want = D.levels_torch(img)
    assert vals.shape == (2, 2) and torch.equal(vals.cpu(), want), (vals, want)
    count = len(torch.unique(torch.clamp((img[0] * 255).round(), 0, 255)))
    assert count == min(n, 256) and float(vals[0, 0]) == 2.0 ** int(np.ceil(np.log2(count)))
    assert torch.equal(hip.degrade_levels(img.cuda()), vals)   # the sets were left zero
    big = cases.image(3, 70, 90, 0.1, 60)                        # several blocks per sample
    assert torch.equal(hip.degrade_levels(big.cuda()).cpu(), D.levels_torch(big))


def test_noise_all_four_branches_to_one_ulp():
    from mrefsr_amd import degradation as D, hip
    img = cases.image(4, 23, 37, 0.05, 61).cuda()
    g = torch.Generator(device='cuda').manual_seed(5)
    gray = torch.tensor([0.0, 1.0, 1.0, 0.0], device='cuda')
    n = torch.randn(img.shape, generator=g, device='cuda')
    ng = torch.randn((4, 1, 23, 37), generator=g, device='cuda')
    sigma = torch.tensor([1.0, 30.0, 12.5, 25.0], device='cuda')
    out, ref = hip.degrade_noise(img, n, ng, sigma, gray), D.noise_torch(img, n, ng, sigma, gray)
    err = float((out - ref).abs().max())
    print(f'noise gaussian: {err:.3e}')
    assert err <= ULP and float(out.min()) >= 0 and float(out.max()) <= 1
    d = out[1] - img[1]                          # a gray sample: the same noise in the three channels wherever nothing was clamped
    free = ((out[1] > 0) & (out[1] < 1)).all(0)
    assert float(((d[0] - d[1]).abs() * free).max()) <= 4 * ULP and float((out[0] - img[0]).abs().max()) > 0
    vals = hip.degrade_levels(img)
    rate, rate_gray = D.poisson_rates_torch(img, vals)
    p, pg = torch.poisson(rate, generator=g), torch.poisson(rate_gray, generator=g)
    scale = torch.tensor([0.05, 3.0, 1.0, 2.5], device='cuda')
    out, ref = hip.degrade_noise(img, p, pg, scale, gray, vals, poisson=True), D.noise_torch(img, p, pg, scale, gray, vals, poisson=True)
    err = float((out - ref).abs().max())
    print(f'noise poisson: {err:.3e}')
    assert err <= ULP and float(out.min()) >= 0 and float(out.max()) <= 1
    ref64 = D.noise_torch(img.double(), p.double(), pg.double(), scale.double(), gray.double(), vals.double(), poisson=True)
    assert float((out.double() - ref64).abs().max()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- usm, jpeg
@pytest.mark.parametrize('key', sorted(cases.USM_CASES))
def test_usm(key):
    """Pixels with ||r| 255 - threshold| < eps (eps = 4 x the fp32 form's residual error, in threshold units) may get the other mask
    bit; each moves the soft mask of its neighbours by at most g0^2 (the largest tap) and so the output by g0^2 weight max|r|."""
    from mrefsr_amd import degradation as D, hip
    b, h, w, noise, seed = cases.USM_CASES[key]
    img = cases.image(b, h, w, noise, seed)
    ref64, ref32 = D.usm_sharp_torch(img.double()), D.usm_sharp_torch(img)
    g = torch.from_numpy(D.gaussian_kernel1d(51))
    kernel = torch.outer(g, g).unsqueeze(0)
    r64 = img.double() - D.filter2d_torch(img.double(), kernel)
    r32 = img - D.filter2d_torch(img, kernel.float())
    eps = FACTOR * float(((r32.double() - r64).abs() * 255).max())
    n = int(((r64.abs() * 255 - 10).abs() < eps).sum())
    assert n <= 1e-3 * img.numel(), (n, img.numel())
    extra = n * float(g.max()) ** 2 * 0.5 * float(r64.abs().max())
    out = hip.degrade_usm(img.cuda())
    print(f'usm {key}: eps {eps:.2e}, {n} pixels at the threshold, allowance {extra:.2e}')
    check(f'usm {key}', out, ref32, ref64, extra=extra)
    assert float((out.cpu() - torch.from_numpy(golden()[f'{key}_out'])).abs().max()) <= 2 * (bar(ref32, ref64) + extra)


def _macroblock_risk(coef, eps, hp, wp):
    b = coef.shape[0]
    near = (coef - torch.floor(coef) - 0.5).abs() < eps
    ny = (hp // 8) * (wp // 8) * 64
    y = near[:, :ny].view(b, hp // 8, wp // 8, 64).any(-1).view(b, hp // 16, 2, wp // 16, 2).any(4).any(2)
    c = near[:, ny:].view(b, 2, hp // 16, wp // 16, 64).any(-1).any(1)
    return y | c


@pytest.mark.parametrize('key', sorted(cases.JPEG_CASES))
def test_jpeg(key):
    """A macroblock with a Y, Cb or Cr coefficient within eps of a half-integer (eps = 4 x the reference's fp32-vs-float64
    coefficient error, from the golden file) is left out of the comparison -- at most one in four -- but must be finite and in [0, 1]."""
    from mrefsr_amd import degradation as D, hip
    b, h, w, noise, seed, quality = cases.JPEG_CASES[key]
    gd = golden()
    img, q = cases.image(b, h, w, noise, seed), torch.tensor(quality)
    assert torch.equal(img, torch.from_numpy(gd[f'{key}_img']))
    c64 = torch.from_numpy(gd[f'{key}_coef64'])
    eps = FACTOR * float((torch.from_numpy(gd[f'{key}_coef32']).double() - c64).abs().max())
    risk = _macroblock_risk(c64, eps, h + -h % 16, w + -w % 16)
    assert float(risk.double().mean()) <= 0.25
    keep = (~risk).repeat_interleave(16, 1).repeat_interleave(16, 2)[:, None, :h, :w].expand(b, 3, h, w)
    out = hip.degrade_jpeg(img.cuda(), q.cuda())
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0 and float(out.max()) <= 1
    ref64 = D.jpeg_torch(img.double(), q.double())
    ref32 = torch.from_numpy(gd[f'{key}_out'])          # the reference's own fp32 result
    print(f'jpeg {key}: eps {eps:.2e}, {int(risk.sum())} of {risk.numel()} macroblocks left out')
    check(f'jpeg {key}', out, torch.where(keep, ref32.double(), ref64).float(), ref64, keep=keep)
    assert float((out.cpu() - img).abs().max()) > 1e-3   # it did compress


# ---------------------------------------------------------------------------------------------------------------- the chain
def _grid_stats(a, b):
    d = ((a.double().cpu() - b.double().cpu()).abs() * 255).round()
    return float((d > 0).double().mean()), float(d.max())


def test_chain_against_the_golden_chain():
    """The chain rounds three times (two JPEG quantisations and the final 1/255 grid), so no two arithmetics agree on every pixel.
    Yardstick: the reference's fp32 chain (the golden file) against the float64 chain of the *_torch operators on the same plan and
    draws -- the fraction of pixels that differ and the largest difference in levels.  The kernels may differ from float64 in
    FACTOR times as many pixels (floor: 1 % of them) by FACTOR times as many levels (floor: one level)."""
    from mrefsr_amd import degradation as D
    gd = golden()
    deg, plan = D.HighOrderDegradation({}), cases.golden_plan(gd)
    gt = torch.from_numpy(gd['chain_gt'])
    lq64, usm64 = deg.apply_torch(gt.double(), plan)
    lq, gt_usm = deg.apply(gt.cuda(), plan)
    assert lq.shape == (2, 3, 12, 16) and lq.dtype == torch.float32
    assert float((lq * 255 - (lq * 255).round()).abs().max()) <= 1e-4
    frac_ref, lev_ref = _grid_stats(torch.from_numpy(gd['chain_lq']), lq64)
    frac, lev = _grid_stats(lq, lq64)
    print(f'chain: reference differs from float64 in {frac_ref:.4f} of the pixels by <= {lev_ref:.0f} levels; kernels {frac:.4f}, {lev:.0f}')
    assert frac <= max(FACTOR * frac_ref, 0.01) and lev <= max(FACTOR * lev_ref, 1.0)
    assert float((gt_usm.double().cpu() - usm64).abs().max()) <= 1e-5


def test_chain_with_poisson_noise_against_the_torch_chain():
    """apply against apply_torch on the GPU, the same plan and generator state, Poisson noise in both stages.  The draws depend on
    the image through its 1/255 levels: where the two arithmetics round a pixel to different levels the draw of that pixel differs
    too, so single pixels may differ by a whole noise sample; all others agree to the final grid.  Allowed: 2 % of the pixels."""
    from mrefsr_amd import degradation as D
    deg = D.HighOrderDegradation(dict(gaussian_noise_prob=0.0, gaussian_noise_prob2=0.0, gray_noise_prob=0.5, gray_noise_prob2=0.5,
                                      resize_range=[0.25, 1.5]))
    plan = deg.sample(2, (48, 64), 11)
    assert plan.noise1.poisson and plan.noise2.poisson
    gt = cases.image(2, 48, 64, 0.03, 31).cuda()
    ga, gb = torch.Generator(device='cuda').manual_seed(9), torch.Generator(device='cuda').manual_seed(9)
    lq, usm = deg.apply(gt, plan, ga)
    lq_t, usm_t = deg.apply_torch(gt, plan, gb)
    frac, lev = _grid_stats(lq, lq_t)
    print(f'poisson chain: {frac:.4f} of the pixels differ, by <= {lev:.0f} levels')
    assert lq.shape == lq_t.shape == (2, 3, 12, 16) and frac <= 0.02
    assert float((usm - usm_t).abs().max()) <= 1e-5
    assert float((lq * 255 - (lq * 255).round()).abs().max()) <= 1e-4
