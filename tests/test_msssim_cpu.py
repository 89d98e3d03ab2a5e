"""CPU: the definition of the MS-SSIM loss (losses.msssim_loss_torch, what losses.MSSSIMLoss runs for CPU tensors) and the numpy
metric (metrics.calculate_msssim).

  1. one level with weight 1 is the SSIM loss (float64, 1e-12)
  2. the float64 autograd gradient against central differences along 8 random directions
  3. the zero rule: a plane with a level whose mean is not positive counts 0 and gets gradient exactly 0 -- no NaN from 0 * inf
  4. a mixed batch: the anti-correlated sample gets exactly 0, the ordinary one half of its gradient alone
  5. refusals: the number and the values of the weights, an image too small for the levels
  6. calculate_msssim: 1.0 for equal images, 1 - the float64 torch expression on the metric's own planes, a small image refused
  7. the validation loop: val.msssim adds MS-SSIM_Y to the log lines, the tb scalars and the result; without it they are today's"""
import logging

import numpy as np
import pytest
import torch

from test_ssim_loss_kernels_gpu import make_inputs


def smooth(shape, seed):
    """the smooth image of tests/test_ssim_loss_kernels_gpu.py, float64"""
    return make_inputs('smooth', shape, seed)[1].double()


def anti_correlated(shape, seed):
    """(pred, target) float64: target = the smooth image + 0.1 Gaussian noise, clamped; pred = 1 - target"""
    g = torch.Generator().manual_seed(seed + 77)
    b, h, w = shape
    target = (smooth(shape, seed) + 0.1 * torch.randn(b, 3, h, w, generator=g, dtype=torch.float64)).clamp(0, 1)
    return 1.0 - target, target


def ordinary(shape, seed):
    pred, target = make_inputs('smooth', shape, seed)
    return pred.double(), target.double()


def level_means(pred, target, channel, weights):
    """F [planes, M] in the inputs' dtype: the per-level means of the definition, spelled out here once more"""
    import torch.nn.functional as F
    from mrefsr_amd.metrics import _gaussian_window
    if channel == 'y':
        coef = pred.new_tensor([65.481, 128.553, 24.966]).view(1, 3, 1, 1)
        x, y = (pred * coef).sum(1, keepdim=True) + 16.0, (target * coef).sum(1, keepdim=True) + 16.0
    else:
        x, y = 255.0 * pred, 255.0 * target
    x, y = x.reshape(-1, 1, *x.shape[2:]), y.reshape(-1, 1, *y.shape[2:])
    k = torch.from_numpy(_gaussian_window(11, 1.5)).to(pred.dtype)
    filt = lambda z: F.conv2d(F.conv2d(z, k.view(1, 1, 11, 1)), k.view(1, 1, 1, 11))   # noqa: E731
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    out = []
    for j in range(len(weights)):
        if j:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
        mx, my = filt(x), filt(y)
        sx, sy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
        m = (2 * sxy + c2) / (sx + sy + c2)
        if j == len(weights) - 1:
            m = m * (2 * mx * my + c1) / (mx * mx + my * my + c1)
        out.append(m.mean(dim=(1, 2, 3)))
    return torch.stack(out, 1)


def test_one_level_with_weight_one_is_the_ssim_loss():
    from mrefsr_amd.losses import msssim_loss_torch, ssim_loss_torch
    pred, target = ordinary((3, 27, 43), 1)
    for channel in ('y', 'rgb'):
        a, b = msssim_loss_torch(pred, target, channel, (1.0,)), ssim_loss_torch(pred, target, channel)
        print(f'{channel}: M = 1 {float(a):.15e}  SSIM loss {float(b):.15e}  difference {abs(float(a) - float(b)):.1e}')
        assert 0.01 < float(b) < 0.99 and abs(float(a) - float(b)) <= 1e-12


@pytest.mark.parametrize('channel', ('y', 'rgb'))
def test_gradient_against_central_differences(channel):
    from mrefsr_amd.losses import msssim_loss_torch
    weights = (0.4, 0.6)
    pred, target = ordinary((1, 23, 45), 2)
    p = pred.clone().requires_grad_(True)
    msssim_loss_torch(p, target, channel, weights).backward()
    g = torch.Generator().manual_seed(5)
    step = 1e-5
    for _ in range(8):
        d = torch.randn(pred.shape, generator=g, dtype=torch.float64)
        num = (msssim_loss_torch(pred + step * d, target, channel, weights) - msssim_loss_torch(pred - step * d, target, channel, weights)) / (2 * step)
        ana = (p.grad * d).sum()
        print(f'{channel}: directional derivative autograd {float(ana):.10e} central differences {float(num):.10e}')
        assert abs(float(ana) - float(num)) <= 1e-6 * abs(float(num))


@pytest.mark.parametrize('shape,weights', [((2, 23, 45), (0.4, 0.6)), ((2, 54, 91), (0.3, 0.3, 0.4))])
def test_zero_rule_gives_loss_weight_and_a_zero_gradient(shape, weights):
    from mrefsr_amd.losses import MSSSIMLoss
    pred, target = anti_correlated(shape, 3)
    f = level_means(pred, target, 'rgb', weights)
    print(f'{shape}: F_1 of the planes {f[:, 0].tolist()}')
    assert bool((f[:, 0] < 0).all())
    for dtype in (torch.float64, torch.float32):
        p = pred.detach().to(dtype, copy=True).requires_grad_(True)
        loss = MSSSIMLoss(loss_weight=0.7, channel='rgb', weights=weights)(p, target.to(dtype))
        loss.backward()
        assert loss.dtype == dtype and float(loss.detach()) == float(torch.tensor(0.7, dtype=dtype))
        assert bool(torch.isfinite(p.grad).all()) and not bool(p.grad.any())


@pytest.mark.parametrize('channel', ('y', 'rgb'))
def test_mixed_batch_zero_for_the_anti_correlated_sample_half_for_the_other(channel):
    from mrefsr_amd.losses import MSSSIMLoss
    weights = (0.4, 0.6)
    bad_p, bad_t = anti_correlated((1, 23, 45), 4)
    good_p, good_t = ordinary((1, 23, 45), 5)
    crit = MSSSIMLoss(channel=channel, weights=weights)
    alone = good_p.clone().requires_grad_(True)
    loss_alone = crit(alone, good_t)
    loss_alone.backward()
    both = torch.cat([bad_p, good_p]).requires_grad_(True)
    loss = crit(both, torch.cat([bad_t, good_t]))
    loss.backward()
    assert float(alone.grad.abs().max()) > 0 and bool(torch.isfinite(both.grad).all())
    assert not bool(both.grad[0].any())
    assert torch.allclose(both.grad[1], 0.5 * alone.grad[0], rtol=1e-12, atol=0)
    assert abs(float(loss.detach()) - (0.5 + 0.5 * float(loss_alone.detach()))) <= 1e-12


def test_refusals():
    from mrefsr_amd.losses import LOSS_REGISTRY, MSSSIMLoss
    assert LOSS_REGISTRY.get('MSSSIMLoss') is MSSSIMLoss
    assert MSSSIMLoss().weights == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    for weights in ((), (0.2,) * 6):
        with pytest.raises(ValueError, match='weights'):
            MSSSIMLoss(weights=weights)
    for bad in (0.0, -0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='finite and > 0'):
            MSSSIMLoss(weights=(0.5, bad))
    with pytest.raises(NotImplementedError, match='window_size'):
        MSSSIMLoss(window_size=7)
    with pytest.raises(NotImplementedError, match='sigma'):
        MSSSIMLoss(sigma=1.0)
    with pytest.raises(NotImplementedError, match='channel'):
        MSSSIMLoss(channel='ycbcr')
    x = torch.rand(1, 3, 160, 160)
    with pytest.raises(ValueError, match=r'160 x 160.*M = 5.*at most M = 4'):
        MSSSIMLoss()(x, x)
    assert float(MSSSIMLoss(weights=(0.25,) * 4)(x, x)) == pytest.approx(0.0, abs=1e-5)
    with pytest.raises(NotImplementedError, match='B,3,H,W'):
        MSSSIMLoss(weights=(1.0,))(torch.rand(1, 1, 32, 32), torch.rand(1, 1, 32, 32))
    with pytest.raises(ValueError, match='differ'):
        MSSSIMLoss(weights=(1.0,))(torch.rand(1, 3, 32, 32), torch.rand(1, 3, 32, 33))


def validation_images(h, w, seed):
    """(output, GT) HWC uint8: a smooth colour image with noise, and a noisier copy"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    base = 128 + 60 * np.sin(0.11 * yy)[..., None] + 50 * np.cos(0.07 * xx + 0.05 * yy)[..., None] + np.array([0.0, 10.0, -10.0])
    gt = np.clip(base + rng.normal(0, 4, (h, w, 3)), 0, 255).round().astype(np.uint8)
    sr = np.clip(gt + rng.normal(0, 9, (h, w, 3)), 0, 255).round().astype(np.uint8)
    return sr, gt


@pytest.mark.parametrize('y', (True, False))
def test_calculate_msssim_is_the_torch_expression_on_the_metrics_planes(y):
    from mrefsr_amd.losses import msssim_planes_torch
    from mrefsr_amd.metrics import MSSSIM_WEIGHTS, calculate_msssim, rgb_to_y
    sr, gt = validation_images(200, 191, 6)
    assert calculate_msssim(gt, gt, 4, test_y_channel=y) == 1.0
    got = calculate_msssim(sr, gt, 4, test_y_channel=y)
    a, b = sr[4:-4, 4:-4], gt[4:-4, 4:-4]
    if y:
        a, b = rgb_to_y(a), rgb_to_y(b)
    planes = [torch.from_numpy(np.ascontiguousarray(v.astype(np.float64).transpose(2, 0, 1)))[:, None] for v in (a, b)]
    want = float(msssim_planes_torch(planes[0], planes[1], MSSSIM_WEIGHTS).mean())
    print(f'calculate_msssim {got:.12f}, torch float64 expression {want:.12f}')
    assert 0.3 < got < 0.999 and abs(got - want) <= 1e-10


def test_calculate_msssim_refuses_a_small_image():
    from mrefsr_amd.metrics import calculate_msssim
    img = np.zeros((100, 100, 3), np.uint8)
    with pytest.raises(ValueError, match='calculate_msssim.*100 x 100.*too small'):
        calculate_msssim(img, img, 0)
    with pytest.raises(ValueError, match='too small'):
        calculate_msssim(np.zeros((180, 180, 3), np.uint8), np.zeros((180, 180, 3), np.uint8), 4, test_y_channel=True)


def FakeValidationModel(out, gt, val_opt, is_train):
    """the validation loop of MultiRefRestorationModel over the image pairs out[i], gt[i] ([N,3,H,W] in [0, 1]) without networks:
    feed_data picks pair i, test() has nothing to do.  run(tb) -> the result of _nondist_validation"""
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel

    class Fake(MultiRefRestorationModel):
        def __init__(self):
            self.opt = dict(val=dict(val_opt), crop_border=4, is_train=is_train, name='fake')
            self.is_train = is_train

        def feed_data(self, data):
            i = int(data['idx'])
            self.output, self.gt = out[i:i + 1], gt[i:i + 1]

        def test(self):
            pass

        def run(self, tb=None):
            loader = [dict(idx=i, lq_path=[f'img{i}.png']) for i in range(out.shape[0])]
            return self._nondist_validation(loader, 7, tb, False)
    return Fake()


class _Tb:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, name, value, it):
        self.scalars[name] = (value, it)


def test_validation_loop_with_and_without_val_msssim(caplog):
    from mrefsr_amd.metrics import calculate_msssim
    pairs = [validation_images(200, 184, seed) for seed in (11, 12)]
    to_t = lambda k: torch.from_numpy(np.stack([p[k] for p in pairs]).transpose(0, 3, 1, 2).astype(np.float32) / 255.0)   # noqa: E731
    out, gt = to_t(0), to_t(1)
    got = {}
    for val_opt in ({}, dict(msssim=False), dict(msssim=True)):
        tb = _Tb()
        caplog.clear()
        with caplog.at_level(logging.INFO, logger='basicsr'):
            res = FakeValidationModel(out, gt, val_opt, is_train=False).run(tb)
        got[val_opt.get('msssim')] = (res, [r.getMessage() for r in caplog.records if r.getMessage().startswith('#')], tb.scalars)
    res, lines, scalars = got[True]
    want = np.mean([calculate_msssim(sr, hr, 4, test_y_channel=True) for sr, hr in pairs])
    assert set(res) == {'psnr', 'psnr_y', 'ssim_y', 'msssim_y'} and abs(res['msssim_y'] - want) <= 1e-12
    assert scalars['msssim_y'] == (res['msssim_y'], 7) and set(scalars) == {'psnr', 'psnr_y', 'ssim_y', 'msssim_y'}
    assert len(lines) == 3 and all(ln.endswith(f' # MS-SSIM_Y: {v:.4e}.') for ln, v in
                                   zip(lines, [calculate_msssim(sr, hr, 4, test_y_channel=True) for sr, hr in pairs] + [want]))
    # absent or false: the lines, scalars and result of today -- the lines above without their MS-SSIM part
    assert got[None] == got[False]
    res0, lines0, scalars0 = got[None]
    assert set(res0) == set(scalars0) == {'psnr', 'psnr_y', 'ssim_y'} and all(res0[k] == res[k] for k in res0)
    assert lines0 == [ln[:ln.index(' # MS-SSIM_Y')] + '.' for ln in lines]
