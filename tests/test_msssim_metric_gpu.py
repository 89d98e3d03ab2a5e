"""GPU: five-level MS-SSIM (Y) of validation on the forward kernels of csrc/msssim.hip (metrics.validation_metrics(msssim=True))
against the numpy metric (metrics.calculate_msssim), and the validation loop with val.msssim and val.metrics_on_device.

Error bar: 4 x the error of the fp32 torch expression (losses.msssim_planes_torch) on the same quantised, cropped Y planes against
the same expression in float64 -- the larger of the two images' errors, as the kernel tests take the largest of a class."""
import logging

import numpy as np
import pytest
import torch

from test_msssim_cpu import FakeValidationModel, validation_images

pytestmark = pytest.mark.gpu

H, W, CB = 200, 184, 4
SIZES = [(200, 184), (197, 184)]      # valid regions: the whole image, and an odd height; both stay >= 176 behind the border


def _pair():
    sr, gt = zip(*(validation_images(H, W, seed) for seed in (11, 12)))
    to_t = lambda imgs: torch.from_numpy(np.stack(imgs).transpose(0, 3, 1, 2).astype(np.float32) / 255.0).contiguous().cuda()   # noqa: E731
    return to_t(sr), to_t(gt)


def test_device_msssim_y_against_the_numpy_metric():
    from mrefsr_amd import metrics
    from mrefsr_amd.losses import msssim_planes_torch
    out, gt = _pair()
    sizes = SIZES
    dev = metrics.validation_metrics(out, gt, CB, sizes=sizes, msssim=True)
    assert set(dev) == {'psnr', 'psnr_y', 'ssim_y', 'finite', 'msssim_y'} and len(dev['msssim_y']) == 2 and all(dev['finite'])
    errs, yard = [], []
    for i, (oh, ow) in enumerate(sizes):
        a, b = metrics.tensor2img(out[i:i + 1])[:oh, :ow], metrics.tensor2img(gt[i:i + 1])[:oh, :ow]
        want = metrics.calculate_msssim(a, b, CB, test_y_channel=True)
        planes = [torch.from_numpy(np.ascontiguousarray(metrics.rgb_to_y(v[CB:-CB, CB:-CB]).astype(np.float64).transpose(2, 0, 1)))[:, None]
                  for v in (a, b)]
        v64 = float(msssim_planes_torch(planes[0], planes[1], metrics.MSSSIM_WEIGHTS)[0])
        v32 = float(msssim_planes_torch(planes[0].float(), planes[1].float(), metrics.MSSSIM_WEIGHTS)[0])
        assert abs(v64 - want) <= 1e-10 and 0.3 < want < 0.999
        errs.append(abs(dev['msssim_y'][i] - want))
        yard.append(abs(v32 - v64))
        print(f'image {i} {oh} x {ow}: MS-SSIM_Y numpy {want:.10f} device {dev["msssim_y"][i]:.10f}  |err| {errs[-1]:.2e}  torch-fp32 {yard[-1]:.2e}')
    assert max(errs) <= 4.0 * max(yard)
    # the same numbers from a second call; equal images give 1 within the bar
    assert metrics.validation_metrics(out, gt, CB, sizes=sizes, msssim=True)['msssim_y'] == dev['msssim_y']
    same = metrics.validation_metrics(gt, gt, CB, sizes=sizes, msssim=True)['msssim_y']
    assert all(abs(v - 1.0) <= 4.0 * max(yard) + 2.0 ** -22 for v in same)
    with pytest.raises(ValueError, match='too small'):
        metrics.validation_metrics(out, gt, CB, sizes=[(200, 184), (180, 184)], msssim=True)


def test_without_the_option_the_keys_are_todays():
    from mrefsr_amd import metrics
    out, gt = _pair()
    assert set(metrics.validation_metrics(out, gt, CB)) == {'psnr', 'psnr_y', 'ssim_y', 'finite'}
    assert set(metrics.validation_metrics(out, gt, CB, return_img=True, msssim=False)) == {'psnr', 'psnr_y', 'ssim_y', 'finite', 'img'}


def test_validation_loop_on_device_equals_the_host(caplog):
    out, gt = _pair()
    res, lines = {}, {}
    for on_device in (False, True):
        model = FakeValidationModel(out, gt, dict(msssim=True, metrics_on_device=on_device), is_train=False)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger='basicsr'):
            res[on_device] = model.run()
        lines[on_device] = [r.getMessage() for r in caplog.records if r.getMessage().startswith('#')]
    assert set(res[True]) == {'psnr', 'psnr_y', 'ssim_y', 'msssim_y'}
    assert abs(res[True]['msssim_y'] - res[False]['msssim_y']) <= 1e-5 and res[True]['psnr'] == res[False]['psnr']
    assert len(lines[True]) == 3 and all('# MS-SSIM_Y: ' in ln for ln in lines[True])
