"""The degradation chain's host side (mrefsr_amd/degradation.py) on the CPU: the float64 *_torch restatements against the reference's
own outputs (tests/golden/degrade.npz, made by tests/golden/gen_golden_degrade.py), the blur-kernel constructors, the sampler, the
training pair pool, the option checks and the library's shape checks (which return before any launch: no GPU is touched).

Tolerances against the fp32 goldens: the reference computed in fp32, so the float64 form differs from it by the reference's own
rounding -- bounded per operator below from the number of fp32 operations on values of magnitude <= 1 (or <= 255 inside JPEG)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import degrade_cases as cases  # noqa: E402

from mrefsr_amd import degradation as D  # noqa: E402

EPS32 = 2.0 ** -24   # half an fp32 ulp of 1


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'degrade.npz')))


def t64(a):
    return torch.from_numpy(a).double()


def test_filter2d_float64_equals_the_reference(golden):
    img = t64(golden['filter_img'])
    for name, kern in (('filter_out21', golden['filter_k21']), ('filter_out7', golden['filter_k7']), ('filter_out_shared', golden['filter_k21'][:1])):
        out = D.filter2d_torch(img, t64(kern))
        # a convex combination of k^2 values <= 1 summed in fp32: at most k^2 roundings of half an ulp (far fewer in a blocked sum)
        bound = kern.shape[-1] ** 2 * EPS32
        err = float((out - t64(golden[name])).abs().max())
        assert err <= bound, (name, err, bound)


def test_usm_float64_equals_the_reference_away_from_the_threshold(golden):
    for key in cases.USM_CASES:
        img = t64(golden[f'{key}_img'])
        ref32 = t64(golden[f'{key}_out'])
        out = D.usm_sharp_torch(img)
        # the fp32 form of the restatement is the reference bit for bit up to summation order: pin it in fp32
        out32 = D.usm_sharp_torch(torch.from_numpy(golden[f'{key}_img']))
        assert float((out32.double() - ref32).abs().max()) <= 16 * EPS32
        g = torch.from_numpy(D.gaussian_kernel1d(51))
        kernel = torch.outer(g, g).unsqueeze(0)
        r = img - D.filter2d_torch(img, kernel)
        img32 = torch.from_numpy(golden[f'{key}_img'])
        r32 = img32 - D.filter2d_torch(img32, kernel.float())
        eps = 4 * float(((r32.double() - r).abs() * 255).max())   # 4 x the fp32 residual's measured error, in threshold units
        n = int(((r.abs() * 255 - 10).abs() < eps).sum())
        assert n <= 1e-3 * img.numel()
        # a pixel whose mask bit differs moves the soft mask by at most g0^2 and the output by g0^2 * weight * max|r|
        slack = n * float(g.max() ** 2) * 0.5 * float(r.abs().max())
        err = float((out - ref32).abs().max())
        assert err <= 4 * 51 * 51 * EPS32 + slack, (key, err, slack)


def _macroblock_risk(coef, eps, hp, wp):
    b = coef.shape[0]
    near = (coef - torch.floor(coef) - 0.5).abs() < eps
    ny = (hp // 8) * (wp // 8) * 64
    y = near[:, :ny].view(b, hp // 8, wp // 8, 64).any(-1).view(b, hp // 16, 2, wp // 16, 2).any(4).any(2)
    c = near[:, ny:].view(b, 2, hp // 16, wp // 16, 64).any(-1).any(1)
    return y | c


def test_jpeg_float64_equals_the_reference_off_the_rounding_cliffs(golden):
    for key, (b, h, w, _, _, _) in cases.JPEG_CASES.items():
        img, q = t64(golden[f'{key}_img']), t64(golden[f'{key}_quality'])
        hp, wp = h + -h % 16, w + -w % 16
        coeffs, _ = D.jpeg_coefficients_torch(img, q)
        mine = torch.cat([c.reshape(b, -1) for c in coeffs], dim=1)
        c64 = t64(golden[f'{key}_coef64'])
        assert float((mine - c64).abs().max()) <= 1e-9          # the un-rounded coefficients: float64 against float64
        eps = 4 * float((t64(golden[f'{key}_coef32']) - c64).abs().max())
        risk = _macroblock_risk(c64, eps, hp, wp)
        assert risk.double().mean() <= 0.25
        out = D.jpeg_torch(img, q)
        assert out.shape == img.shape and bool(torch.isfinite(out).all()) and float(out.min()) >= 0 and float(out.max()) <= 1
        keep = (~risk).repeat_interleave(16, 1).repeat_interleave(16, 2)[:, None, :h, :w].expand_as(out)
        # off the cliffs both round alike; what is left is the fp32 rounding of ~200 operations on values <= 255, over 255
        err = float(((out - t64(golden[f'{key}_out'])).abs() * keep).max())
        assert err <= 200 * EPS32 * 2, (key, err)


def test_kernel_constructors_equal_the_reference(golden):
    for key, (kind, size, sx, sy, theta, beta) in cases.KERNEL_CASES.items():
        k = D.mixed_kernel(kind, size, sx, sy, theta, beta)
        assert k.dtype == np.float64 and k.shape == (size, size)
        assert float(np.abs(k - golden[key]).max()) <= 1e-12, key
    for key, (cutoff, size, pad_to) in cases.SINC_CASES.items():
        k = D.circular_lowpass_kernel(cutoff, size, pad_to=pad_to)
        assert k.shape == golden[key].shape and float(np.abs(k - golden[key]).max()) <= 1e-12, key
    with pytest.raises(ValueError):
        D.mixed_kernel('skew', 21, 1.0)
    with pytest.raises(ValueError):
        D.circular_lowpass_kernel(1.0, 8)


def test_chain_of_torch_forms_equals_the_reference_chain(golden):
    """fp32 against fp32: the same operators in the same order on the same draws.  The chain rounds three times (two JPEGs, the
    final 1/255 grid), so single roundings may fall the other way where the tensordot's summation order differs: the outputs are
    on the 1/255 grid, nearly all equal, and none differs by more than a few levels."""
    deg = D.HighOrderDegradation({})
    lq, gt_usm = deg.apply_torch(torch.from_numpy(golden['chain_gt']), cases.golden_plan(golden))
    assert float((gt_usm - torch.from_numpy(golden['chain_gt_usm'])).abs().max()) <= 16 * EPS32
    ref = torch.from_numpy(golden['chain_lq'])
    assert lq.shape == ref.shape == (2, 3, 12, 16)
    levels = lq * 255
    assert float((levels - levels.round()).abs().max()) <= 1e-4
    diff = ((lq - ref).abs() * 255).round()
    assert float((diff > 0).float().mean()) <= 0.02 and float(diff.max()) <= 3, (float((diff > 0).float().mean()), float(diff.max()))


def test_noise_and_levels_forms():
    img = cases.image(3, 9, 11, 0.05, 7)
    vals = D.levels_torch(img)
    for i in range(3):
        n = len(torch.unique(torch.clamp((img[i] * 255).round(), 0, 255)))
        assert float(vals[i, 0]) == 2.0 ** int(np.ceil(np.log2(n)))
    flat = torch.full((1, 3, 4, 4), 0.5)
    assert D.levels_torch(flat).tolist() == [[1.0, 1.0]]
    g = torch.Generator().manual_seed(0)
    n, ng = torch.randn(3, 3, 9, 11, generator=g), torch.randn(3, 1, 9, 11, generator=g)
    sigma, gray = torch.tensor([5.0, 10.0, 20.0]), torch.tensor([0.0, 1.0, 0.0])
    out = D.noise_torch(img, n, ng, sigma, gray)
    assert torch.equal(out[0], torch.clamp(img[0] + n[0] * 5.0 / 255., 0, 1))
    assert torch.equal(out[1], torch.clamp(img[1] + (ng[1] * 10.0 / 255.).expand(3, 9, 11), 0, 1))
    rate, rate_gray = D.poisson_rates_torch(img, vals)
    p, pg = torch.poisson(rate, generator=g), torch.poisson(rate_gray, generator=g)
    out = D.noise_torch(img, p, pg, torch.tensor([1.0, 2.0, 0.5]), gray, vals, poisson=True)
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0 and float(out.max()) <= 1
    lvl = torch.clamp((img[0] * 255).round(), 0, 255) / 255.
    assert torch.allclose(out[0], torch.clamp(img[0] + (p[0] / vals[0, 0] - lvl) * 1.0, 0, 1), atol=1e-7)


OPT01 = dict(resize_prob=[1, 0, 0], resize_prob2=[0, 0, 1], gaussian_noise_prob=1.0, gaussian_noise_prob2=0.0, gray_noise_prob=1.0,
             gray_noise_prob2=0.0, second_blur_prob=0.0, sinc_prob=1.0, sinc_prob2=0.0, final_sinc_prob=0.0)


def test_sample_is_reproducible_and_honours_probabilities_of_0_and_1():
    deg = D.HighOrderDegradation(OPT01)
    a, b = deg.sample(3, (64, 96), 5), deg.sample(3, (64, 96), 5)
    c = deg.sample(3, (64, 96), np.random.default_rng(6))
    for name in ('kernel1', 'kernel2', 'sinc_kernel', 'jpeg1', 'jpeg2'):
        assert np.array_equal(getattr(a, name), getattr(b, name)) and getattr(a, name).dtype == np.float32
    assert a.resize1 == b.resize1 and a.resize2 == b.resize2 and a.final_mode == b.final_mode
    assert not np.array_equal(a.kernel1, c.kernel1)
    for seed in range(12):
        p = deg.sample(2, (48, 48), seed)
        assert 1.0 <= p.resize1[0] <= 1.5 and p.resize2[0] == 1.0 and p.resize1[1] in D.RESIZE_MODES
        assert not p.noise1.poisson and p.noise2.poisson and p.noise1.gray.tolist() == [1, 1] and p.noise2.gray.tolist() == [0, 0]
        assert 1 <= p.noise1.param.min() and p.noise1.param.max() <= 30 and 0.05 <= p.noise2.param.min() and p.noise2.param.max() <= 2.5
        assert not p.second_blur and 30 <= p.jpeg1.min() and p.jpeg2.max() <= 95
        pulse = np.zeros((21, 21), np.float32)
        pulse[10, 10] = 1
        assert all(np.array_equal(k, pulse) for k in p.sinc_kernel)            # no final sinc: the pulse
        assert p.kernel1.shape == (2, 21, 21) and np.allclose(p.kernel1.sum((1, 2)), 1, atol=1e-5)
        assert (p.kernel1 < 0).any() and (p.kernel2 >= 0).all()              # stage 1 always sinc (it rings), stage 2 never
    orders = {deg.sample(1, (48, 48), s).resize_before_jpeg for s in range(20)}
    assert orders == {True, False}
    with pytest.raises(ValueError, match='multiple of 4'):
        deg.sample(1, (40, 64), 0)
    with pytest.raises(ValueError, match='below 11'):
        deg.sample(1, (32, 32), 0)
    with pytest.raises(ValueError, match='resize_range '):      # 64 * 0.15 = 9 pixels in front of the second 21 x 21 blur
        D.HighOrderDegradation({}).sample(1, (64, 64), 0)
    D.HighOrderDegradation(dict(resize_range=[0.2, 1.5])).sample(1, (64, 64), 0)


def test_options_are_refused_by_name():
    with pytest.raises(ValueError, match=r"\['resize_probs'\]"):
        D.HighOrderDegradation(dict(resize_probs=[1, 0, 0]))
    with pytest.raises(ValueError, match='resize_prob2'):
        D.HighOrderDegradation(dict(resize_prob2=[1, 0]))
    with pytest.raises(ValueError, match='jpeg_range'):
        D.HighOrderDegradation(dict(jpeg_range=[0, 50]))
    with pytest.raises(ValueError, match='kernel_list2'):
        D.HighOrderDegradation(dict(kernel_list2=['iso', 'skew'], kernel_prob2=[0.5, 0.5]))
    assert D.HighOrderDegradation(dict(queue_size=8, scale=2)).queue_size == 8


def test_training_pair_pool_fills_then_swaps_and_keeps_samples_together():
    with pytest.raises(ValueError):
        D.TrainingPairPool(0)
    pool = D.TrainingPairPool(4)
    with pytest.raises(ValueError, match='divisible'):
        D.TrainingPairPool(4).step(dict(lq=torch.zeros(3, 1)))

    def batch(i):   # every tensor of sample s carries the id s
        ids = torch.tensor([2 * i, 2 * i + 1])
        return dict(lq=ids.float().view(2, 1, 1, 1).expand(2, 3, 2, 2).clone(), gt=ids.float().view(2, 1, 1, 1).expand(2, 3, 8, 8).clone(),
                    refs=ids.float().view(2, 1, 1, 1, 1).expand(2, 2, 3, 8, 8).clone(), ref_valid=ids.int())
    g = torch.Generator().manual_seed(3)
    for i in range(2):   # filling: the batch comes back as it is
        out = pool.step(batch(i), g)
        assert all(torch.equal(out[k], v) for k, v in batch(i).items())
    seen = []
    for i in range(2, 6):
        out = pool.step(batch(i), g)
        ids = out['ref_valid'].tolist()
        for j, s in enumerate(ids):
            assert float(out['lq'][j].min()) == float(out['lq'][j].max()) == s
            assert float(out['gt'][j].min()) == float(out['gt'][j].max()) == s
            assert float(out['refs'][j].min()) == float(out['refs'][j].max()) == s
        assert all(s < 2 * i for s in ids)   # nothing of the batch just fed leaves at once
        seen += ids
    assert len(set(seen)) == len(seen)       # a sample leaves once
    held = sorted(pool.queue['ref_valid'].tolist())
    assert sorted(seen + held) == list(range(12))
    with pytest.raises(ValueError):
        pool.step(dict(lq=torch.zeros(2, 3, 2, 2)))


def test_library_refuses_bad_shapes_before_any_launch():
    from mrefsr_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)   # never dereferenced: every call below fails its checks first
    f = ctypes.c_float
    taps = (ctypes.c_float * 51)(*([1 / 51] * 51))

    def refused(rc, word):
        assert rc != 0 and word in lib.mrefsr_last_error().decode(), lib.mrefsr_last_error().decode()
    refused(lib.mrefsr_degrade_filter2d_f32(p, p, 1, 3, 32, 32, 4, 0, ctypes.c_void_p(128), None), 'odd')
    refused(lib.mrefsr_degrade_filter2d_f32(p, p, 1, 3, 32, 32, 23, 0, ctypes.c_void_p(128), None), 'odd')
    refused(lib.mrefsr_degrade_filter2d_f32(p, p, 1, 3, 10, 32, 21, 0, ctypes.c_void_p(128), None), 'reflect')
    refused(lib.mrefsr_degrade_filter2d_f32(p, p, 1, 3, 32, 10, 21, 0, ctypes.c_void_p(128), None), 'reflect')
    refused(lib.mrefsr_degrade_filter2d_f32(p, p, 0, 3, 32, 32, 21, 0, ctypes.c_void_p(128), None), 'batch')
    refused(lib.mrefsr_degrade_filter2d_f32(p, p, 1, 3, 32, 32, 21, 0, p, None), 'in-place')
    refused(lib.mrefsr_degrade_usm_f32(p, taps, 1, 3, 25, 40, 51, f(0.5), f(10), ctypes.c_void_p(128), ctypes.c_void_p(256), None), 'reflect')
    refused(lib.mrefsr_degrade_usm_f32(p, taps, 1, 3, 40, 40, 53, f(0.5), f(10), ctypes.c_void_p(128), ctypes.c_void_p(256), None), 'odd')
    refused(lib.mrefsr_degrade_resize_f32(p, 1, 3, 8, 8, 0, 4, 1, f(1), f(1), ctypes.c_void_p(128), None), 'sides')
    refused(lib.mrefsr_degrade_resize_f32(p, 1, 3, 8, 8, 4, 4, 3, f(1), f(1), ctypes.c_void_p(128), None), 'mode')
    refused(lib.mrefsr_degrade_resize_f32(p, 1, 3, 8, 8, 4, 4, 2, f(0), f(1), ctypes.c_void_p(128), None), 'positive')
    refused(lib.mrefsr_degrade_noise_f32(p, p, p, p, p, None, 1, 8, 8, 1, ctypes.c_void_p(128), None), 'vals')
    refused(lib.mrefsr_degrade_noise_f32(p, p, p, p, p, p, 1, 8, 8, 2, ctypes.c_void_p(128), None), 'mode')
    refused(lib.mrefsr_degrade_levels_f32(p, 1, 0, 8, p, p, None), 'h=0')
    refused(lib.mrefsr_degrade_jpeg_f32(p, p, 30000, 8, 8, p, None), 'batch')
    refused(lib.mrefsr_degrade_jpeg_f32(p, None, 1, 8, 8, p, None), 'null')
    assert lib.mrefsr_degrade_levels_workspace_words(3) == 51 and lib.mrefsr_degrade_levels_workspace_words(0) < 0


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from mrefsr_amd import hip
    img = torch.zeros(1, 3, 16, 16)
    with pytest.raises(NotImplementedError):
        hip.degrade_filter2d(img, torch.zeros(1, 3, 3))
    assert hip.degrade_resize_geometry((37, 41), size=(9, 10)) == ((9, 10), (37 / 9, 41 / 10))
    assert hip.degrade_resize_geometry((37, 41), scale_factor=0.25) == ((9, 10), (4.0, 4.0))
    with pytest.raises(ValueError):
        hip.degrade_resize_geometry((37, 41))
    with pytest.raises(ValueError):
        hip.degrade_resize_geometry((4, 4), scale_factor=0.1)
