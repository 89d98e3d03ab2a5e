"""GPU: the validation metrics of csrc/metrics.hip against the numpy functions of mrefsr_amd/metrics.py (tensor2img, calculate_psnr,
calculate_ssim), and MultiRefRestorationModel.nondist_validation with val.metrics_on_device against the numpy path.

Gates: uint8 images bit-equal; RGB PSNR equal (==); PSNR-Y, SSIM-Y and RGB SSIM within 1e-10; two runs bit-identical."""
import logging
import os
import zlib

import numpy as np
import pytest
import torch

from mrefsr_amd import hip, metrics

pytestmark = pytest.mark.gpu
TOL = 1e-10


def _halfway_values():
    """fp32 values v in [0, 1] with v * 255 (in fp32) exactly k + 0.5: tensor2img rounds them half to even"""
    k = np.arange(255)
    v = ((k + 0.5) / 255.0).astype(np.float32)
    hit = v[v * np.float32(255.) == (k + 0.5).astype(np.float32)]
    near = np.concatenate([np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(1))])
    near = near[near * np.float32(255.) == np.round(near * np.float32(255.)) + np.float32(0.5)]
    return np.concatenate([hit, near]).astype(np.float32)


HALFWAY = _halfway_values()


def _pair(kind, n, h, w, seed):
    """fp32 [n,3,h,w] (output, GT) on the GPU"""
    r = np.random.default_rng(seed)
    gt = r.random((n, 3, h, w)).astype(np.float32)
    if kind == 'random':         # values outside [0, 1] on both sides, and exact half-way products
        out = r.uniform(-0.2, 1.2, (n, 3, h, w)).astype(np.float32)
        if len(HALFWAY):
            idx = r.random(out.shape) < 0.2
            out[idx] = r.choice(HALFWAY, int(idx.sum()))
            idx = r.random(gt.shape) < 0.2
            gt[idx] = r.choice(HALFWAY, int(idx.sum()))
    elif kind == 'near':         # 50-60 dB
        out = gt.copy()
        idx = r.random(out.shape) < 0.2
        out[idx] += np.float32(1.0 / 255.)
    else:                        # identical
        out = gt.copy()
    return torch.from_numpy(out).cuda(), torch.from_numpy(gt).cuda()


def _numpy(out, gt, cb, size=None):
    """the host protocol of nondist_validation for image 0 of out / gt"""
    a, b = metrics.tensor2img(out[:1]), metrics.tensor2img(gt[:1])
    if size is not None:
        a, b = a[:size[0], :size[1]], b[:size[0], :size[1]]
    return dict(img=a, psnr=metrics.calculate_psnr(a, b, cb), psnr_y=metrics.calculate_psnr(a, b, cb, True),
                ssim_y=metrics.calculate_ssim(a, b, cb, True), ssim_rgb=metrics.calculate_ssim(a, b, cb, False))


def _check(out, gt, cb, sizes=None):
    n = out.shape[0]
    dev = metrics.validation_metrics(out, gt, cb, sizes=sizes, return_img=True)
    psnr = metrics.calculate_psnr_device(out, gt, cb, sizes=sizes)
    psnr_y = metrics.calculate_psnr_device(out, gt, cb, test_y_channel=True, sizes=sizes)
    ssim_y = metrics.calculate_ssim_device(out, gt, cb, test_y_channel=True, sizes=sizes)
    ssim_rgb = metrics.calculate_ssim_device(out, gt, cb, sizes=sizes)
    imgs = metrics.tensor2img_device(out).cpu().numpy()
    assert np.array_equal(dev['img'].cpu().numpy(), imgs)
    got = []
    for i in range(n):
        size = None if sizes is None else sizes[i]
        want = _numpy(out[i:i + 1], gt[i:i + 1], cb, size)
        assert np.array_equal(imgs[i], metrics.tensor2img(out[i:i + 1]))
        assert np.array_equal(metrics.tensor2img_device(out[i]).cpu().numpy(), metrics.tensor2img(out[i:i + 1]))
        assert dev['psnr'][i] == want['psnr'] and psnr[i] == want['psnr'], (i, dev['psnr'][i], want['psnr'])
        for name, vals in (('psnr_y', (dev['psnr_y'][i], psnr_y[i])), ('ssim_y', (dev['ssim_y'][i], ssim_y[i])), ('ssim_rgb', (ssim_rgb[i], ))):
            for v in vals:
                if np.isinf(want[name]):
                    assert v == want[name], (name, v)
                else:
                    assert abs(v - want[name]) <= TOL, (name, i, v, want[name])
        assert dev['finite'][i]
        got.append(want)
    # two runs: the same bits
    flags = hip.VALM_SSIM_Y | hip.VALM_SSIM_RGB
    r1, _ = hip.val_metrics(out, gt, cb, sizes=sizes, flags=flags)
    r2, _ = hip.val_metrics(out, gt, cb, sizes=sizes, flags=flags)
    assert torch.equal(r1, r2)
    return got


def test_halfway_values_exist():
    assert len(HALFWAY) > 50


@pytest.mark.parametrize('kind', ['random', 'near', 'identical'])
@pytest.mark.parametrize('hw', [(500, 500), (333, 492)])
def test_full_images(kind, hw):
    out, gt = _pair(kind, 1, *hw, seed=zlib.crc32(f'{kind}{hw}'.encode()))
    want = _check(out, gt, 4)[0]
    if kind == 'near':
        assert 50 <= want['psnr'] <= 60, want['psnr']
    if kind == 'identical':
        assert want['psnr'] == want['psnr_y'] == float('inf') and want['ssim_y'] == 1.0


@pytest.mark.parametrize('kind', ['random', 'near', 'identical'])
@pytest.mark.parametrize('cb', [0, 4])
def test_minimum_size(kind, cb):
    s = 11 + 2 * cb
    out, gt = _pair(kind, 1, s, s, seed=7 + cb)
    _check(out, gt, cb)
    out, gt = _pair(kind, 1, s, s + 9, seed=8 + cb)
    _check(out, gt, cb)
    with pytest.raises(Exception, match='at least 11x11'):
        metrics.validation_metrics(out[..., :s - 1, :], gt[..., :s - 1, :], cb)


@pytest.mark.parametrize('kind', ['random', 'near'])
def test_padding_crop(kind):
    """valid region smaller than the tensors; the GT tensor itself only as large as the region (the CUFED5 set's layout)"""
    out, gt = _pair(kind, 1, 96, 112, seed=11)
    _check(out, gt, 4, sizes=[(61, 87)])
    _check(out, gt[..., :61, :87].contiguous(), 4, sizes=[(61, 87)])
    assert metrics.calculate_psnr_device(out[0], gt[0], 4, sizes=(61, 87)) == _numpy(out, gt, 4, (61, 87))['psnr']


def test_batches():
    """N > 1 with a region per image, and a batch larger than one set of launches (32 images)"""
    out, gt = _pair('random', 3, 72, 80, seed=3)
    near, gt2 = _pair('near', 3, 72, 80, seed=4)
    out = torch.cat([out, near, gt2[:1]])
    gt = torch.cat([gt, gt2, gt2[:1]])
    _check(out, gt, 4, sizes=[(72, 80), (40, 51), (19, 70), (72, 19), (33, 33), (64, 77), (50, 50)])
    out, gt = _pair('near', 37, 24, 30, seed=5)
    _check(out, gt, 2, sizes=[(24 - i % 5, 30 - i % 7) for i in range(37)])


def test_non_finite_inputs_are_flagged():
    out, gt = _pair('random', 2, 40, 40, seed=9)
    out[0, 1, 30, 30] = float('nan')
    out[1, 0, 39, 39] = float('inf')                 # outside image 1's valid region
    res = metrics.validation_metrics(out, gt, 4, sizes=[(40, 40), (36, 36)])
    assert res['finite'] == [False, True]
    gt[1, 2, 5, 5] = float('-inf')
    assert metrics.validation_metrics(out, gt, 4, sizes=[(40, 40), (36, 36)])['finite'] == [False, False]


# ------------------------------------------------------------------ the model
def _validate(model, loader, on_device, save_dir, caplog):
    model.opt['val'] = dict(save_img=True, metrics_on_device=on_device)
    model.opt['path'] = dict(visualization=str(save_dir))
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='basicsr'):
        res = model.validation(loader, 0, None, save_img=True)
    lines = [r.getMessage() for r in caplog.records if r.name == 'basicsr' and r.getMessage().startswith('#')]
    files = {}
    for root, _, names in os.walk(save_dir):
        for n in names:
            files[os.path.relpath(os.path.join(root, n), save_dir)] = open(os.path.join(root, n), 'rb').read()
    return res, lines, files


def test_nondist_validation_on_device_equals_numpy(golden, tmp_path, caplog):
    """the CUFED5 loader (500 x 500 zero-padded outputs, GT at the original size) through model.validation with the option off and
    on: the same dict (1e-10), the same log lines at .4e, the same PNG bytes"""
    import make_dataset_files as mk
    from test_archs_gpu import _model
    from mrefsr_amd.data import build_dataset
    model, _ = _model(golden('e2e'), False)
    ds = build_dataset(mk.make_cufed(str(tmp_path / 'cufed')))
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0)
    res0, lines0, files0 = _validate(model, loader, False, tmp_path / 'host', caplog)
    res1, lines1, files1 = _validate(model, loader, True, tmp_path / 'device', caplog)
    assert set(res0) == set(res1) == {'psnr', 'psnr_y', 'ssim_y'}
    assert res1['psnr'] == res0['psnr']
    for k in res0:
        assert abs(res1[k] - res0[k]) <= TOL, (k, res0[k], res1[k])
    assert len(lines0) == len(ds) + 1 and lines1 == lines0
    assert len(files0) == len(ds) and files1 == files0


def test_nondist_validation_takes_numpy_for_non_finite_outputs(golden, tmp_path, monkeypatch):
    """an image whose output holds NaN is measured by the numpy path: the same numbers as with the option off"""
    import make_dataset_files as mk
    from test_archs_gpu import _model
    from mrefsr_amd.data import build_dataset
    model, _ = _model(golden('e2e'), False)
    ds = build_dataset(mk.make_cufed(str(tmp_path / 'cufed')))
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0)
    test = type(model).test

    def nan_test(self):
        test(self)
        self.output[0, 0, 10, 10] = float('nan')
    monkeypatch.setattr(type(model), 'test', nan_test)
    calls = []
    real = metrics.tensor2img
    monkeypatch.setattr(metrics, 'tensor2img', lambda *a, **k: calls.append(1) or real(*a, **k))
    model.opt['val'] = dict(metrics_on_device=False)
    res0 = model.validation(loader, 0, None)
    n0 = len(calls)
    model.opt['val'] = dict(metrics_on_device=True)
    res1 = model.validation(loader, 0, None)
    assert len(calls) == 2 * n0 and res1 == res0
