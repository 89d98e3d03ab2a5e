"""Real-ESRGAN's second-order degradation: synthesise the low-quality input of a training batch on the device (opt['degradation']).

Three layers:

* ``*_torch``: every operator of the chain restated in plain torch, dtype-generic.  They are the definition the kernels of
  csrc/degrade.hip are tested against; in float64 they equal the reference's own functions (basicsr/utils/img_process_util.py,
  basicsr/utils/diffjpeg.py, basicsr/data/degradations.py; tests/golden/degrade.npz).
* blur-kernel synthesis on the host in numpy float64 (B kernels of 21 x 21 per step; not a hot path): deterministic constructors
  with explicit parameters, and ``sample_blur_kernel`` / ``sample_final_kernel``, which draw them as
  basicsr/data/realesrgan_dataset.py:129-183 does.
* ``HighOrderDegradation``: ``sample`` draws every random decision of basicsr/models/realesrgan_model.py:83-165 into a plain
  ``DegradationPlan``; ``apply`` runs the chain on the HIP kernels (``apply_torch``: on the torch forms, the same draws).
  ``TrainingPairPool`` is the reference's _dequeue_and_enqueue (:31-66) over a dict of tensors.
"""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

RESIZE_MODES = ('area', 'bilinear', 'bicubic')
KERNEL_KINDS = ('iso', 'aniso', 'generalized_iso', 'generalized_aniso', 'plateau_iso', 'plateau_aniso')
KERNEL_RANGE = tuple(2 * v + 1 for v in range(3, 11))   # 7 ... 21 (realesrgan_dataset.py:79), padded to 21


# ------------------------------------------------------------------------------------------------ torch restatements
def filter2d_torch(img, kernel):
    """filter2D (img_process_util.py:7-31): img [B,C,H,W], kernel [B,k,k] or [1,k,k], k odd"""
    k = kernel.size(-1)
    if k % 2 != 1:
        raise ValueError('Wrong kernel size')
    b, c, h, w = img.shape
    pad = F.pad(img, (k // 2,) * 4, mode='reflect')
    ph, pw = pad.shape[-2:]
    if kernel.size(0) == 1:
        return F.conv2d(pad.reshape(b * c, 1, ph, pw), kernel.view(1, 1, k, k)).view(b, c, h, w)
    weight = kernel.view(b, 1, k, k).repeat(1, c, 1, 1).view(b * c, 1, k, k)
    return F.conv2d(pad.reshape(1, b * c, ph, pw), weight, groups=b * c).view(b, c, h, w)


def gaussian_kernel1d(k):
    """cv2.getGaussianKernel(k, 0)'s formula in float64: sigma = 0.3 ((k - 1) / 2 - 1) + 0.8, normalised exp(-x^2 / 2 sigma^2).
    (For k <= 7 cv2 itself returns fixed binomial-like tables; USMSharp's radius is 51.)"""
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def usm_sharp_torch(img, radius=51, weight=0.5, threshold=10):
    """USMSharp(radius).forward(img, weight, threshold) (img_process_util.py:63-83) in img's dtype (the reference forces the mask to
    fp32; here it takes the image's dtype, which is the same thing for fp32 images)"""
    k = radius + 1 if radius % 2 == 0 else radius
    g = gaussian_kernel1d(k)[:, None]
    kernel = torch.from_numpy(np.dot(g, g.T)).to(device=img.device, dtype=img.dtype).unsqueeze(0)
    residual = img - filter2d_torch(img, kernel)
    mask = (torch.abs(residual) * 255 > threshold).to(img.dtype)
    soft = filter2d_torch(mask, kernel)
    sharp = torch.clip(img + weight * residual, 0, 1)
    return soft * sharp + (1 - soft) * img


def resize_torch(img, size=None, scale_factor=None, mode='bicubic'):
    """F.interpolate as realesrgan_model.py:95 (scale_factor) and :126, :151, :164 (size) call it"""
    if mode not in RESIZE_MODES:
        raise ValueError(f'resize: mode {mode!r} not in {RESIZE_MODES}')
    return F.interpolate(img, size=size, scale_factor=scale_factor, mode=mode)


def gray_torch(img):
    """torchvision's rgb_to_grayscale, one channel: 0.2989 R + 0.587 G + 0.114 B"""
    r, g, b = img.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(-3)


def _level255(x):
    return torch.clamp((x * 255.0).round(), 0, 255)


def levels_torch(img):
    """[B,2]: 2^ceil(log2(#distinct levels)) of the three channels and of the gray image (degradations.py:630-648)"""
    gray = gray_torch(img)
    rows = [[2.0 ** math.ceil(math.log2(len(torch.unique(_level255(t[i]))))) for t in (img, gray)] for i in range(img.shape[0])]
    return torch.tensor(rows, dtype=img.dtype, device=img.device)


def noise_torch(img, noise, noise_gray, param, gray, vals=None, poisson=False):
    """random_add_gaussian_noise_pt / random_add_poisson_noise_pt (degradations.py:461-514, 610-684; clip=True, rounds=False) as a
    deterministic function of the drawn tensors, in the reference's operation order.  noise [B,3,H,W], noise_gray [B,1,H,W];
    param (sigma, or scale with poisson) and gray (0 / 1) [B].  Gaussian: the draws are standard normal.  Poisson: the draws are
    torch.poisson of level * vals[:, 0] and gray level * vals[:, 1] (poisson_rates_torch)."""
    b = img.shape[0]
    p, g = param.view(b, 1, 1, 1), gray.view(b, 1, 1, 1)
    if not poisson:
        n = (noise * p / 255.) * (1 - g) + (noise_gray * p / 255.) * g
        return torch.clamp(img + n, 0, 1)
    v0, v1 = vals[:, 0].view(b, 1, 1, 1), vals[:, 1].view(b, 1, 1, 1)
    n_gray = noise_gray / v1 - _level255(gray_torch(img)) / 255.
    n = noise / v0 - _level255(img) / 255.
    n = n * (1 - g) + n_gray * g
    return torch.clamp(img + n * p, 0, 1)


def poisson_rates_torch(img, vals):
    """the rates of the two Poisson draws of noise_torch(poisson=True): ([B,3,H,W], [B,1,H,W])"""
    b = img.shape[0]
    return (_level255(img) / 255. * vals[:, 0].view(b, 1, 1, 1), _level255(gray_torch(img)) / 255. * vals[:, 1].view(b, 1, 1, 1))


_Y_TABLE = np.array(
    [[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56], [14, 17, 22, 29, 51, 87, 80, 62],
     [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92], [49, 64, 78, 87, 103, 121, 120, 101],
     [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.float64).T   # (transposed, as diffjpeg.py:14-18 holds it)
_C_TABLE = np.full((8, 8), 99.0)
_C_TABLE[:4, :4] = np.array([[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]], dtype=np.float64).T


def _dct_basis():
    n = np.arange(8)
    c = np.cos((2 * n[:, None] + 1) * n[None, :] * np.pi / 16)   # c[x, u]
    # (the reference holds its constants as fp32 parameters: the float64 form computes with those values)
    return np.einsum('xu,yv->xyuv', c, c).astype(np.float32).astype(np.float64)


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def quality_to_factor_torch(quality):
    """diffjpeg.py:32-45 on a tensor"""
    return torch.where(quality < 50, 5000. / quality, 200. - quality * 2) / 100.


def jpeg_coefficients_torch(img, quality):
    """The un-rounded quantised DCT coefficients (CompressJpeg with rounding = identity) of the image zero-padded to multiples of
    16: (y [B,Hp/8*Wp/8,8,8], cb, cr [B,Hp/16*Wp/16,8,8]), and the per-sample (table_y, table_c) [B,1,8,8]"""
    dt, dev = img.dtype, img.device
    b, _, h, w = img.shape
    x = F.pad(img, (0, -w % 16, 0, -h % 16), mode='constant', value=0) * 255
    m = torch.from_numpy(_f32([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]])).to(device=dev, dtype=dt).T
    ycc = torch.tensordot(x.permute(0, 2, 3, 1), m, dims=1) + torch.tensor([0., 128., 128.], dtype=dt, device=dev)
    planes = [ycc[..., 0]] + [F.avg_pool2d(ycc[..., i].unsqueeze(1), 2, 2).squeeze(1) for i in (1, 2)]
    basis = torch.from_numpy(_dct_basis()).to(device=dev, dtype=dt)
    alpha = np.array([1. / np.sqrt(2)] + [1] * 7)
    scale = torch.from_numpy(_f32(np.outer(alpha, alpha) * 0.25)).to(device=dev, dtype=dt)
    factor = quality_to_factor_torch(quality.to(dt)).view(b, 1, 1, 1)
    tables = [torch.from_numpy(t).to(device=dev, dtype=dt).expand(b, 1, 8, 8) * factor for t in (_Y_TABLE, _C_TABLE)]
    coeffs = []
    for i, p in enumerate(planes):
        ph, pw = p.shape[1:]
        blocks = p.view(b, ph // 8, 8, pw // 8, 8).permute(0, 1, 3, 2, 4).reshape(b, -1, 8, 8)
        coeffs.append(scale * torch.tensordot(blocks - 128, basis, dims=2) / tables[min(i, 1)])
    return coeffs, tables


def jpeg_torch(img, quality):
    """DiffJPEG(differentiable=False)(img, quality) (diffjpeg.py:449-491) in img's dtype; quality [B] is not modified"""
    dt, dev = img.dtype, img.device
    b, _, h, w = img.shape
    hp, wp = h + -h % 16, w + -w % 16
    coeffs, tables = jpeg_coefficients_torch(img, quality)
    alpha = np.array([1. / np.sqrt(2)] + [1] * 7)
    alpha2 = torch.from_numpy(_f32(np.outer(alpha, alpha))).to(device=dev, dtype=dt)
    ibasis = torch.from_numpy(_dct_basis().transpose(2, 3, 0, 1).copy()).to(device=dev, dtype=dt)   # [x, y, u, v] = cos((2u+1)x..)cos((2v+1)y..)
    planes = []
    for i, c in enumerate(coeffs):
        deq = torch.round(c) * tables[min(i, 1)]
        rec = 0.25 * torch.tensordot(deq * alpha2, ibasis, dims=2) + 128
        ph, pw = (hp, wp) if i == 0 else (hp // 2, wp // 2)
        planes.append(rec.view(b, ph // 8, pw // 8, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, ph, pw))
    up = [planes[0]] + [p.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) for p in planes[1:]]
    ycc = torch.stack(up, dim=3) + torch.tensor([0., -128., -128.], dtype=dt, device=dev)
    m = torch.from_numpy(_f32([[1., 0., 1.402], [1, -0.344136, -0.714136], [1, 1.772, 0]])).to(device=dev, dtype=dt).T
    rgb = torch.tensordot(ycc, m, dims=1).permute(0, 3, 1, 2)
    return (torch.clamp(rgb, 0, 255) / 255)[:, :, :h, :w]


def finish_torch(out):
    """realesrgan_model.py:168: onto the 1/255 grid"""
    return torch.clamp((out * 255.0).round(), 0, 255) / 255.


# ------------------------------------------------------------------------------------------------ blur kernels (numpy float64)
def mesh_grid(kernel_size):
    ax = np.arange(-kernel_size // 2 + 1., kernel_size // 2 + 1.)
    xx, yy = np.meshgrid(ax, ax)
    return np.stack([xx, yy], axis=2)


def sigma_matrix2(sig_x, sig_y, theta):
    d = np.array([[sig_x ** 2, 0], [0, sig_y ** 2]])
    u = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    return np.dot(u, np.dot(d, u.T))


def _quadratic_form(kernel_size, sig_x, sig_y, theta, isotropic):
    grid = mesh_grid(kernel_size)
    sigma = np.array([[sig_x ** 2, 0], [0, sig_x ** 2]]) if isotropic else sigma_matrix2(sig_x, sig_y, theta)
    return np.sum(np.dot(grid, np.linalg.inv(sigma)) * grid, 2)


def bivariate_gaussian(kernel_size, sig_x, sig_y=None, theta=0.0, isotropic=True):
    """degradations.py:84-109"""
    kernel = np.exp(-0.5 * _quadratic_form(kernel_size, sig_x, sig_y, theta, isotropic))
    return kernel / np.sum(kernel)


def bivariate_generalized_gaussian(kernel_size, sig_x, sig_y, theta, beta, isotropic=True):
    """degradations.py:112-144"""
    kernel = np.exp(-0.5 * np.power(_quadratic_form(kernel_size, sig_x, sig_y, theta, isotropic), beta))
    return kernel / np.sum(kernel)


def bivariate_plateau(kernel_size, sig_x, sig_y, theta, beta, isotropic=True):
    """degradations.py:147-176"""
    kernel = np.reciprocal(np.power(_quadratic_form(kernel_size, sig_x, sig_y, theta, isotropic), beta) + 1)
    return kernel / np.sum(kernel)


def circular_lowpass_kernel(cutoff, kernel_size, pad_to=0):
    """degradations.py:392-410: the 2-D sinc filter, J1 by scipy.special.j1 as there (torch.special.bessel_j1 differs from it by
    1e-8 in float64)"""
    from scipy import special
    if kernel_size % 2 != 1:
        raise ValueError('Kernel size must be an odd number.')
    c = (kernel_size - 1) / 2
    x, y = np.meshgrid(np.arange(kernel_size, dtype=np.float64), np.arange(kernel_size, dtype=np.float64), indexing='ij')
    r = np.sqrt((x - c) ** 2 + (y - c) ** 2)
    j1 = special.j1(cutoff * r)
    with np.errstate(divide='ignore', invalid='ignore'):
        kernel = cutoff * j1 / (2 * np.pi * r)
    kernel[(kernel_size - 1) // 2, (kernel_size - 1) // 2] = cutoff ** 2 / (4 * np.pi)
    kernel = kernel / np.sum(kernel)
    if pad_to > kernel_size:
        pad = (pad_to - kernel_size) // 2
        kernel = np.pad(kernel, ((pad, pad), (pad, pad)))
    return kernel


def mixed_kernel(kind, kernel_size, sig_x, sig_y=None, theta=0.0, beta=1.0):
    """one of random_mixed_kernels' six kinds (degradations.py:327-386) from explicit parameters"""
    if kind not in KERNEL_KINDS:
        raise ValueError(f'kernel kind {kind!r} not in {KERNEL_KINDS}')
    iso = kind.endswith('iso') and not kind.endswith('aniso')
    if kind in ('iso', 'aniso'):
        return bivariate_gaussian(kernel_size, sig_x, sig_y, theta, isotropic=iso)
    if kind.startswith('generalized'):
        return bivariate_generalized_gaussian(kernel_size, sig_x, sig_y, theta, beta, isotropic=iso)
    return bivariate_plateau(kernel_size, sig_x, sig_y, theta, beta, isotropic=iso)


def _pad21(kernel):
    pad = (21 - kernel.shape[0]) // 2
    return np.pad(kernel, ((pad, pad), (pad, pad)))


def sample_mixed_kernel(rng, kernel_list, kernel_prob, kernel_size, sigma_range, betag_range, betap_range):
    """random_mixed_kernels with noise_range=None, the draws made on `rng` (a numpy Generator)"""
    prob = np.asarray(kernel_prob, dtype=np.float64)
    kind = kernel_list[int(rng.choice(len(kernel_list), p=prob / prob.sum()))]
    if kind not in KERNEL_KINDS:
        raise ValueError(f'kernel_list: {kind!r} not in {KERNEL_KINDS}')
    sig_x = rng.uniform(sigma_range[0], sigma_range[1])
    sig_y, theta = sig_x, 0.0
    if kind.endswith('aniso'):
        sig_y, theta = rng.uniform(sigma_range[0], sigma_range[1]), rng.uniform(-math.pi, math.pi)
    beta = 1.0
    if kind not in ('iso', 'aniso'):
        lo, hi = betag_range if kind.startswith('generalized') else betap_range
        beta = rng.uniform(lo, 1) if rng.uniform() < 0.5 else rng.uniform(1, hi)
    return mixed_kernel(kind, kernel_size, sig_x, sig_y, theta, beta)


def sample_blur_kernel(rng, opt, suffix=''):
    """one 21 x 21 kernel of a degradation stage (realesrgan_dataset.py:129-150; suffix '2' for the second stage)"""
    size = int(rng.choice(KERNEL_RANGE))
    if rng.uniform() < opt['sinc_prob' + suffix]:
        omega = rng.uniform(np.pi / 3, np.pi) if size < 13 else rng.uniform(np.pi / 5, np.pi)
        kernel = circular_lowpass_kernel(omega, size, pad_to=0)
    else:
        kernel = sample_mixed_kernel(rng, opt['kernel_list' + suffix], opt['kernel_prob' + suffix], size, opt['blur_sigma' + suffix],
                                     opt['betag_range' + suffix], opt['betap_range' + suffix])
    return _pad21(kernel)


def sample_final_kernel(rng, opt):
    """realesrgan_dataset.py:175-182: a sinc filter, or the pulse (no effect) when none is drawn"""
    if rng.uniform() < opt['final_sinc_prob']:
        size = int(rng.choice(KERNEL_RANGE))
        return circular_lowpass_kernel(rng.uniform(np.pi / 3, np.pi), size, pad_to=21)
    pulse = np.zeros((21, 21))
    pulse[10, 10] = 1
    return pulse


# ------------------------------------------------------------------------------------------------ the chain
@dataclass
class NoisePlan:
    poisson: bool
    param: np.ndarray            # [B] float32: sigma (Gaussian) or scale (Poisson)
    gray: np.ndarray             # [B] float32 flags 0 / 1
    drawn: Optional[tuple] = None   # (noise [B,3,H,W], noise_gray [B,1,H,W]) to use instead of drawing (Gaussian only)


@dataclass
class DegradationPlan:
    """every random decision of one batch's degradation (realesrgan_model.py:83-165); plain data"""
    gt_hw: tuple
    scale: int
    kernel1: np.ndarray          # [B,21,21] float32
    kernel2: np.ndarray
    sinc_kernel: np.ndarray
    resize1: tuple               # (scale_factor, mode): F.interpolate(scale_factor=...)
    noise1: NoisePlan
    jpeg1: np.ndarray            # [B] float32 qualities
    second_blur: bool
    resize2: tuple               # (scale_factor, mode): to int(h / scale * s) x int(w / scale * s) by size
    noise2: NoisePlan
    final_mode: str              # the mode of the resize back to gt_hw / scale
    resize_before_jpeg: bool     # [resize back + sinc] then JPEG; or JPEG first
    jpeg2: np.ndarray


_STAGE_KEYS = ('resize_prob', 'resize_range', 'gaussian_noise_prob', 'noise_range', 'poisson_scale_range', 'gray_noise_prob', 'jpeg_range')
_KERNEL_KEYS = ('blur_kernel_size', 'kernel_list', 'kernel_prob', 'blur_sigma', 'betag_range', 'betap_range', 'sinc_prob')
OPTION_KEYS = frozenset([k + s for k in _STAGE_KEYS + _KERNEL_KEYS for s in ('', '2')] + ['second_blur_prob', 'final_sinc_prob', 'scale',
                                                                                          'queue_size'])
# the reference's train_realesrgan_x4plus.yml
DEFAULTS = dict(
    resize_prob=[0.2, 0.7, 0.1], resize_range=[0.15, 1.5], gaussian_noise_prob=0.5, noise_range=[1, 30], poisson_scale_range=[0.05, 3],
    gray_noise_prob=0.4, jpeg_range=[30, 95], second_blur_prob=0.8, resize_prob2=[0.3, 0.4, 0.3], resize_range2=[0.3, 1.2],
    gaussian_noise_prob2=0.5, noise_range2=[1, 25], poisson_scale_range2=[0.05, 2.5], gray_noise_prob2=0.4, jpeg_range2=[30, 95],
    blur_kernel_size=21, kernel_list=list(KERNEL_KINDS), kernel_prob=[0.45, 0.25, 0.12, 0.03, 0.12, 0.03], sinc_prob=0.1,
    blur_sigma=[0.2, 3], betag_range=[0.5, 4], betap_range=[1, 2], blur_kernel_size2=21, kernel_list2=list(KERNEL_KINDS),
    kernel_prob2=[0.45, 0.25, 0.12, 0.03, 0.12, 0.03], sinc_prob2=0.1, blur_sigma2=[0.2, 1.5], betag_range2=[0.5, 4], betap_range2=[1, 2],
    final_sinc_prob=0.8, scale=4)


class _HipOps:
    """the chain's operators on the kernels of csrc/degrade.hip"""

    def __init__(self):
        from . import hip
        self.filter2d, self.usm, self.resize, self.jpeg = hip.degrade_filter2d, hip.degrade_usm, hip.degrade_resize, hip.degrade_jpeg
        self.levels, self.noise = hip.degrade_levels, hip.degrade_noise


class _TorchOps:
    filter2d, usm, resize, jpeg = staticmethod(filter2d_torch), staticmethod(usm_sharp_torch), staticmethod(resize_torch), staticmethod(jpeg_torch)
    levels, noise = staticmethod(levels_torch), staticmethod(noise_torch)


class HighOrderDegradation:
    """opt: the reference yml's degradation and kernel keys (OPTION_KEYS; absent ones take the values of its
    train_realesrgan_x4plus.yml, DEFAULTS).  Unknown keys are refused by name."""

    def __init__(self, opt):
        opt = dict(opt or {})
        unknown = sorted(set(opt) - OPTION_KEYS)
        if unknown:
            raise ValueError(f'degradation: unknown key(s) {unknown} (the options are {sorted(OPTION_KEYS)})')
        self.queue_size = opt.pop('queue_size', None)
        self.opt = {**DEFAULTS, **opt}
        o = self.opt
        for s in ('', '2'):
            if len(o['resize_prob' + s]) != 3 or min(o['resize_prob' + s]) < 0 or sum(o['resize_prob' + s]) <= 0:
                raise ValueError(f"degradation: resize_prob{s} {o['resize_prob' + s]}: three weights (up, down, keep) expected")
            for key in ('resize_range', 'noise_range', 'poisson_scale_range', 'jpeg_range', 'blur_sigma', 'betag_range', 'betap_range'):
                r = o[key + s]
                if len(r) != 2 or not r[0] <= r[1]:
                    raise ValueError(f'degradation: {key}{s} {r}: [low, high] expected')
            if not (0 < o['jpeg_range' + s][0] and o['jpeg_range' + s][1] <= 100):
                raise ValueError(f"degradation: jpeg_range{s} {o['jpeg_range' + s]} outside (0, 100]")
            if o['resize_range' + s][0] <= 0:
                raise ValueError(f"degradation: resize_range{s} {o['resize_range' + s]} must be positive")
            if o['blur_kernel_size' + s] != 21:
                raise ValueError(f"degradation: blur_kernel_size{s} {o['blur_kernel_size' + s]}: kernels are drawn from 7 ... 21 and padded to 21")
            if len(o['kernel_list' + s]) != len(o['kernel_prob' + s]) or any(k not in KERNEL_KINDS for k in o['kernel_list' + s]):
                raise ValueError(f'degradation: kernel_list{s} / kernel_prob{s}: equally long, kinds from {KERNEL_KINDS}')
        self.scale = int(o['scale'])
        if self.scale < 1:
            raise ValueError(f"degradation: scale {o['scale']}")

    # -------------------------------------------------------------------------------------------- the draws
    @staticmethod
    def _resize_draw(rng, prob, rng_range):
        p = np.asarray(prob, dtype=np.float64)
        kind = int(rng.choice(3, p=p / p.sum()))   # up, down, keep
        scale = rng.uniform(1, rng_range[1]) if kind == 0 else rng.uniform(rng_range[0], 1) if kind == 1 else 1.0
        return float(scale), RESIZE_MODES[int(rng.integers(3))]

    def _noise_draw(self, rng, b, s):
        o = self.opt
        poisson = not rng.uniform() < o['gaussian_noise_prob' + s]
        lo, hi = o['poisson_scale_range' + s] if poisson else o['noise_range' + s]
        param = (rng.uniform(size=b) * (hi - lo) + lo).astype(np.float32)
        gray = (rng.uniform(size=b) < o['gray_noise_prob' + s]).astype(np.float32)
        return NoisePlan(poisson=bool(poisson), param=param, gray=gray)

    def sample(self, b, gt_hw, rng=None):
        """the plan of a batch of b images of gt_hw; rng: a numpy Generator, a seed, or None"""
        rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        h, w = int(gt_hw[0]), int(gt_hw[1])
        self.check_size(h, w)
        o = self.opt
        k1 = np.stack([sample_blur_kernel(rng, o) for _ in range(b)]).astype(np.float32)
        k2 = np.stack([sample_blur_kernel(rng, o, '2') for _ in range(b)]).astype(np.float32)
        ks = np.stack([sample_final_kernel(rng, o) for _ in range(b)]).astype(np.float32)
        resize1 = self._resize_draw(rng, o['resize_prob'], o['resize_range'])
        noise1 = self._noise_draw(rng, b, '')
        jpeg1 = rng.uniform(o['jpeg_range'][0], o['jpeg_range'][1], size=b).astype(np.float32)
        second_blur = bool(rng.uniform() < o['second_blur_prob'])
        resize2 = self._resize_draw(rng, o['resize_prob2'], o['resize_range2'])
        noise2 = self._noise_draw(rng, b, '2')
        before = bool(rng.uniform() < 0.5)
        final_mode = RESIZE_MODES[int(rng.integers(3))]
        jpeg2 = rng.uniform(o['jpeg_range2'][0], o['jpeg_range2'][1], size=b).astype(np.float32)
        return DegradationPlan(gt_hw=(h, w), scale=self.scale, kernel1=k1, kernel2=k2, sinc_kernel=ks, resize1=resize1, noise1=noise1,
                               jpeg1=jpeg1, second_blur=second_blur, resize2=resize2, noise2=noise2, final_mode=final_mode,
                               resize_before_jpeg=before, jpeg2=jpeg2)

    def check_size(self, h, w):
        """the GT sides: multiples of 4 * scale"""
        m = 4 * self.scale
        if h % m or w % m or h < m or w < m:
            raise ValueError(f'degradation: GT size {(h, w)} is not a multiple of 4 * scale = {m}')
        # a 21 x 21 blur reflect-pads by 10: every image it meets needs sides of 11 at least, whatever is drawn (checked here, for
        # the ranges, so that no batch fails on an unlucky draw)
        o, side = self.opt, min(h, w)
        if side // self.scale < 11:
            raise ValueError(f'degradation: GT size {(h, w)} / scale {self.scale} is below 11, the least side a 21 x 21 kernel filters')
        low = o['resize_range'][0] if o['resize_prob'][1] > 0 else 1.0
        if o['second_blur_prob'] > 0 and math.floor(side * min(low, 1.0)) < 11:
            raise ValueError(f"degradation: resize_range {o['resize_range']} can shrink a GT side of {side} below 11, the least side the "
                             'second 21 x 21 blur filters; raise its lower end or the GT size')
        low2 = o['resize_range2'][0] if o['resize_prob2'][1] > 0 else 1.0
        if int(side / self.scale * min(low2, 1.0)) < 1:
            raise ValueError(f"degradation: resize_range2 {o['resize_range2']} leaves no pixel of a GT side of {side} / {self.scale}")

    # -------------------------------------------------------------------------------------------- the chain
    @staticmethod
    def _noise(ops, out, plan, generator):
        b, _, h, w = out.shape
        dev, dt = out.device, out.dtype
        param, gray = torch.from_numpy(plan.param).to(dev, dt), torch.from_numpy(plan.gray).to(dev, dt)
        if not plan.poisson:
            if plan.drawn is not None:
                n, ng = (t.to(dev, dt).contiguous() for t in plan.drawn)
            else:   # the gray pattern is one (h, w) draw for the batch, scaled per sample (degradations.py:482-483)
                ng = torch.randn((1, 1, h, w), generator=generator, device=dev, dtype=dt).expand(b, 1, h, w).contiguous()
                n = torch.randn(out.shape, generator=generator, device=dev, dtype=dt)
            return ops.noise(out, n, ng, param, gray)
        vals = ops.levels(out)
        rate, rate_gray = poisson_rates_torch(out, vals)
        ng = torch.poisson(rate_gray, generator=generator)
        n = torch.poisson(rate, generator=generator)
        return ops.noise(out, n, ng, param, gray, vals, poisson=True)

    def _chain(self, ops, gt, plan, generator):
        if gt.dim() != 4 or gt.shape[1] != 3 or tuple(gt.shape[2:]) != tuple(plan.gt_hw) or gt.shape[0] != plan.kernel1.shape[0]:
            raise ValueError(f'degradation: gt {tuple(gt.shape)} does not fit the plan ({plan.kernel1.shape[0]} images of {plan.gt_hw})')
        dev, dt = gt.device, gt.dtype
        h, w = plan.gt_hw
        as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)   # noqa: E731
        gt = gt.contiguous()
        gt_usm = ops.usm(gt)
        out = ops.filter2d(gt_usm, as_t(plan.kernel1))
        out = ops.resize(out, scale_factor=plan.resize1[0], mode=plan.resize1[1])
        out = self._noise(ops, out, plan.noise1, generator)
        out = ops.jpeg(torch.clamp(out, 0, 1), as_t(plan.jpeg1))
        if plan.second_blur:
            out = ops.filter2d(out, as_t(plan.kernel2))
        s2 = plan.resize2[0]
        out = ops.resize(out, size=(int(h / plan.scale * s2), int(w / plan.scale * s2)), mode=plan.resize2[1])
        out = self._noise(ops, out, plan.noise2, generator)
        size = (h // plan.scale, w // plan.scale)
        if plan.resize_before_jpeg:
            out = ops.filter2d(ops.resize(out, size=size, mode=plan.final_mode), as_t(plan.sinc_kernel))
            out = ops.jpeg(torch.clamp(out, 0, 1), as_t(plan.jpeg2))
        else:
            out = ops.jpeg(torch.clamp(out, 0, 1), as_t(plan.jpeg2))
            out = ops.filter2d(ops.resize(out, size=size, mode=plan.final_mode), as_t(plan.sinc_kernel))
        return finish_torch(out), gt_usm

    @torch.no_grad()
    def apply(self, gt, plan, generator=None):
        """gt [B,3,H,W] fp32 on the GPU -> (lq [B,3,H/scale,W/scale] on the 1/255 grid, gt_usm) on the kernels of csrc/degrade.hip;
        generator: the torch.Generator of the noise draws (the device's default one when None)"""
        return self._chain(_HipOps(), gt, plan, generator)

    @torch.no_grad()
    def apply_torch(self, gt, plan, generator=None):
        """the same chain on the *_torch operators (any device and dtype), the same draws from `generator`"""
        return self._chain(_TorchOps, gt, plan, generator)


class TrainingPairPool:
    """The reference's training pair pool (realesrgan_model.py:31-66) over a dict of tensors whose first dimension is the batch
    (lq, gt, the reference stack, the ref_valid words ...): the first queue_size / B batches are stored and returned as they are;
    from then on the pool is shuffled, its first B entries leave and the new batch takes their place.  Entries of one sample stay
    together.  torch indexing only; works on any device."""

    def __init__(self, queue_size):
        if isinstance(queue_size, bool) or not isinstance(queue_size, int) or queue_size < 1:
            raise ValueError(f'queue_size {queue_size!r}: a positive int expected')
        self.queue_size, self.queue, self.ptr, self.batch = queue_size, None, 0, None

    @torch.no_grad()
    def step(self, batch, generator=None):
        """batch: {name: tensor [B, ...]} -> the batch to train on (the same keys); generator: a CPU torch.Generator of the shuffle"""
        sizes = {int(t.shape[0]) for t in batch.values()}
        if len(sizes) != 1:
            raise ValueError(f'TrainingPairPool: tensors of one batch size expected, got {sorted(sizes)}')
        b = sizes.pop()
        if self.queue is None:
            if self.queue_size % b:
                raise ValueError(f'queue size {self.queue_size} should be divisible by batch size {b}')
            self.queue = {k: t.new_zeros((self.queue_size,) + tuple(t.shape[1:])) for k, t in batch.items()}
            self.batch = b
        if b != self.batch or set(batch) != set(self.queue) or any(batch[k].shape[1:] != q.shape[1:] for k, q in self.queue.items()):
            raise ValueError('TrainingPairPool: the batch does not have the keys and shapes the pool was filled with')
        if self.ptr == self.queue_size:
            idx = torch.randperm(self.queue_size, generator=generator)
            out = {}
            for k, q in self.queue.items():
                q = q[idx.to(q.device)]
                out[k] = q[:b].clone()
                q[:b] = batch[k]
                self.queue[k] = q
            return out
        for k, q in self.queue.items():
            q[self.ptr:self.ptr + b] = batch[k]
        self.ptr += b
        return dict(batch)
