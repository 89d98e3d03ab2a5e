#!/usr/bin/env python3
"""Generate tests/golden/degrade.npz: the reference's own degradation operators on the inputs of tests/golden/degrade_cases.py.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_degrade.py
The reference is imported through _refimport.install() as it is, plus two stubs of this file: cv2.getGaussianKernel (its documented
formula for sigma <= 0: sigma = 0.3 ((k - 1) / 2 - 1) + 0.8, normalised exp(-x^2 / 2 sigma^2)) and
torchvision.transforms.functional_tensor.rgb_to_grayscale (0.2989 R + 0.587 G + 0.114 B).  Stored, all from the reference in fp32
unless said:

  filter_*    filter2D (basicsr/utils/img_process_util.py:7-31) on 2 x 3 x 23 x 37 with per-sample 21 x 21 and 7 x 7 kernels and a
              shared one
  usm_*       USMSharp()(img) (:63-83) at 32 x 40 and 40 x 56
  jpeg_*      DiffJPEG(differentiable=False) (basicsr/utils/diffjpeg.py:449-491) at 40 x 56 and 33 x 47 with per-sample qualities;
              `_coef64` / `_coef32`: the un-rounded quantised coefficients (CompressJpeg(rounding=identity)) in float64 and fp32,
              Y, Cb, Cr concatenated per sample
  k_*         bivariate_Gaussian, bivariate_generalized_Gaussian, bivariate_plateau, circular_lowpass_kernel
              (basicsr/data/degradations.py) in float64
  chain_*     one whole chain composed of these functions as basicsr/models/realesrgan_model.py:83-168 composes them, for the
              fixed plan degrade_cases.chain_plan() (Gaussian noise in both stages; the drawn noise tensors are stored)

Asserted here: at most one JPEG macroblock in four has a coefficient within eps of a half-integer, eps = 4 x the reference's
fp32-vs-float64 coefficient error; at most 0.1 % of the USM pixels lie within eps of the mask threshold."""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refimport  # noqa: E402
import degrade_cases as cases  # noqa: E402


def _gaussian_kernel(ksize, sigma):
    if sigma <= 0:
        sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    g = np.exp(-(x * x) / (2 * sigma * sigma))
    return (g / g.sum()).reshape(ksize, 1)


def load_reference():
    _refimport.install()
    sys.modules['cv2'].getGaussianKernel = _gaussian_kernel
    ft = types.ModuleType('torchvision.transforms.functional_tensor')

    def rgb_to_grayscale(img, num_output_channels=1):
        r, g, b = img.unbind(dim=-3)
        return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(dim=-3)
    ft.rgb_to_grayscale = rgb_to_grayscale
    sys.modules['torchvision.transforms.functional_tensor'] = ft
    ipu = importlib.import_module('basicsr.utils.img_process_util')
    dj = importlib.import_module('basicsr.utils.diffjpeg')
    deg = importlib.import_module('basicsr.data.degradations')
    return ipu, dj, deg


def jpeg_coefficients(dj, img, quality, dtype):
    """CompressJpeg(rounding=identity) of the image padded as DiffJPEG.forward pads it: [B, n] per sample, Y, Cb, Cr in turn"""
    comp = dj.CompressJpeg(rounding=lambda x: x).to(dtype)
    factor = torch.tensor([dj.quality_to_factor(float(q)) for q in quality], dtype=torch.float64).to(dtype)
    h, w = img.shape[-2:]
    x = F.pad(img.to(dtype), (0, -w % 16, 0, -h % 16), mode='constant', value=0)
    # (YQuantize / CQuantize call image.float(): run them by hand in `dtype`)
    y, cb, cr = comp.l1(x * 255)
    out = []
    for name, plane in (('y', y), ('cb', cb), ('cr', cr)):
        c = comp.l2(plane)
        table = (dj.y_table if name == 'y' else dj.c_table).detach().to(dtype)
        out.append((c / (table.expand(len(quality), 1, 8, 8) * factor.view(-1, 1, 1, 1))).reshape(len(quality), -1))
    return torch.cat(out, dim=1)


def at_risk_macroblocks(coef, eps, hp, wp):
    """bool [B, hp/16, wp/16]: a Y, Cb or Cr coefficient of the macroblock lies within eps of a half-integer"""
    b = coef.shape[0]
    near = ((coef - torch.floor(coef) - 0.5).abs() < eps)
    ny = (hp // 8) * (wp // 8) * 64
    nc = (hp // 16) * (wp // 16) * 64
    y = near[:, :ny].view(b, hp // 8, wp // 8, 64).any(-1).view(b, hp // 16, 2, wp // 16, 2).any(4).any(2)
    c = near[:, ny:].view(b, 2, hp // 16, wp // 16, 64).any(-1).any(1)
    assert near.shape[1] == ny + 2 * nc
    return y | c


def main():
    sys.dont_write_bytecode = True
    ipu, dj, deg = load_reference()
    from mrefsr_amd import degradation as D
    arrays = {}
    with torch.no_grad():
        # filter2D
        img = cases.image(*cases.FILTER_SHAPE[:1], *cases.FILTER_SHAPE[2:], 0.05, 3)
        k21, k7 = cases.filter_kernels()
        arrays.update(filter_img=img.numpy(), filter_k21=k21.numpy(), filter_k7=k7.numpy(), filter_out21=ipu.filter2D(img, k21).numpy(),
                      filter_out7=ipu.filter2D(img, k7).numpy(), filter_out_shared=ipu.filter2D(img, k21[:1]).numpy())
        # USMSharp
        usm = ipu.USMSharp()
        for key, (b, h, w, noise, seed) in cases.USM_CASES.items():
            img = cases.image(b, h, w, noise, seed)
            out = usm(img)
            r64 = img.double() - D.filter2d_torch(img.double(), usm.kernel.double())
            r32 = img - ipu.filter2D(img, usm.kernel)
            eps = 4 * float(((r32.double() - r64).abs() * 255).max())
            n = int((((r64.abs() * 255) - 10).abs() < eps).sum())
            print(f'{key}: eps {eps:.2e}, {n} of {img.numel()} pixels at the threshold')
            assert n <= 1e-3 * img.numel()
            arrays.update({f'{key}_img': img.numpy(), f'{key}_out': out.numpy()})
        # DiffJPEG
        jpeger = dj.DiffJPEG(differentiable=False)
        for key, (b, h, w, noise, seed, quality) in cases.JPEG_CASES.items():
            img = cases.image(b, h, w, noise, seed)
            q = torch.tensor(quality, dtype=torch.float32)
            out = jpeger(img, quality=q.clone())
            c64, c32 = jpeg_coefficients(dj, img, quality, torch.float64), jpeg_coefficients(dj, img, quality, torch.float32)
            eps = 4 * float((c32.double() - c64).abs().max())
            risk = at_risk_macroblocks(c64, eps, h + -h % 16, w + -w % 16)
            print(f'{key}: eps {eps:.2e}, {int(risk.sum())} of {risk.numel()} macroblocks at risk, max |coef| {float(c64.abs().max()):.0f}')
            assert risk.double().mean() <= 0.25
            arrays.update({f'{key}_img': img.numpy(), f'{key}_quality': q.numpy(), f'{key}_out': out.numpy(), f'{key}_coef64': c64.numpy(),
                           f'{key}_coef32': c32.numpy()})
        # kernel constructors
        for key, (kind, size, sx, sy, theta, beta) in cases.KERNEL_CASES.items():
            iso = not kind.endswith('aniso')
            if kind in ('iso', 'aniso'):
                k = deg.bivariate_Gaussian(size, sx, sy, theta, isotropic=iso)
            elif kind.startswith('generalized'):
                k = deg.bivariate_generalized_Gaussian(size, sx, sy, theta, beta, isotropic=iso)
            else:
                k = deg.bivariate_plateau(size, sx, sy, theta, beta, isotropic=iso)
            arrays[key] = k
        for key, (cutoff, size, pad_to) in cases.SINC_CASES.items():
            arrays[key] = deg.circular_lowpass_kernel(cutoff, size, pad_to=pad_to)

        # one whole chain (realesrgan_model.py:83-168)
        def pad21(k):
            p = (21 - k.shape[0]) // 2
            return np.pad(k, ((p, p), (p, p)))
        pulse = np.zeros((21, 21))
        pulse[10, 10] = 1
        kernel1 = np.stack([pad21(arrays['k_iso']), pad21(arrays['k_aniso'])]).astype(np.float32)
        kernel2 = np.stack([pad21(arrays['k_giso']), pad21(arrays['k_ganiso'])]).astype(np.float32)
        sinc = np.stack([arrays['k_sinc7pad'], pulse]).astype(np.float32)
        p = cases.chain_plan()
        b, h, w = cases.CHAIN_GT
        gt = cases.image(b, h, w, 0.03, 31)

        def gaussian_stage(x, sigma, gray, seed):
            torch.manual_seed(seed)
            out = deg.add_gaussian_noise_pt(x, torch.from_numpy(sigma), torch.from_numpy(gray), clip=True, rounds=False)
            torch.manual_seed(seed)   # the same draws again, to store them (degradations.py:482, 486)
            ng = torch.randn(*x.shape[2:4])
            n = torch.randn(*x.shape)
            return out, n, ng
        gt_usm = usm(gt)
        out = ipu.filter2D(gt_usm, torch.from_numpy(kernel1))
        out = F.interpolate(out, scale_factor=p['resize1'][0], mode=p['resize1'][1])
        out, n1, ng1 = gaussian_stage(out, p['sigma1'], p['gray1'], p['noise_seeds'][0])
        out = jpeger(torch.clamp(out, 0, 1), quality=torch.from_numpy(p['jpeg1']).clone()).contiguous()   # (a permuted view: filter2D views it)
        out = ipu.filter2D(out, torch.from_numpy(kernel2))
        s2 = p['resize2'][0]
        out = F.interpolate(out, size=(int(h / p['scale'] * s2), int(w / p['scale'] * s2)), mode=p['resize2'][1])
        out, n2, ng2 = gaussian_stage(out, p['sigma2'], p['gray2'], p['noise_seeds'][1])
        assert p['resize_before_jpeg'] and p['second_blur']
        out = F.interpolate(out, size=(h // p['scale'], w // p['scale']), mode=p['final_mode'])
        out = ipu.filter2D(out, torch.from_numpy(sinc))
        out = jpeger(torch.clamp(out, 0, 1), quality=torch.from_numpy(p['jpeg2']).clone())
        lq = torch.clamp((out * 255.0).round(), 0, 255) / 255.
        arrays.update(chain_gt=gt.numpy(), chain_kernel1=kernel1, chain_kernel2=kernel2, chain_sinc=sinc, chain_n1=n1.numpy(),
                      chain_ng1=ng1.numpy(), chain_n2=n2.numpy(), chain_ng2=ng2.numpy(), chain_gt_usm=gt_usm.numpy(), chain_lq=lq.numpy())
    path = os.path.join(HERE, 'degrade.npz')
    np.savez_compressed(path, **arrays)
    print(f'{path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
