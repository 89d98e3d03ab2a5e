"""L1Loss, MSELoss, CharbonnierLoss, PerceptualLoss, TextureLoss, GANLoss and GradientPenaltyLoss with the reference's constructor signatures
and values (basicsr/models/losses.py:17-124, 141-238, 275-532), GANLoss's wgan_softplus type and r1_penalty from the newer
basicsr/losses/losses.py:258-360, 391-405.  LDLLoss is the artifact loss of LDL (basicsr/losses/loss_util.py:99-145 as used by
basicsr/models/realesrgan_model.py:211-226), on the kernels of csrc/ldl_loss.hip.  SSIMLoss has no counterpart in the reference: it is the structural-similarity term the
validation metric (mrefsr_amd/metrics.py: calculate_ssim) measures, as a criterion, on the kernels of csrc/ssim_loss.hip.  FFTLoss and FocalFrequencyLoss have none either: the L1 distance of the spectra
(MIMO-UNet, DeepRFT) and the focal frequency loss (Jiang et al., ICCV 2021), on the dense-DFT kernels of csrc/freq_loss.hip.
ContextualLoss has none either: the contextual loss of Mechrez et al. (ECCV 2018) between VGG features, on the kernels of
csrc/contextual.hip (archs/nhwc_train.py: _VggContextual).  MSSSIMLoss has none either: multi-scale SSIM (Wang, Simoncelli, Bovik 2003) with the
validation metric's window at every level, on the kernels of csrc/msssim.hip.

The pixel criteria stay element-wise torch operations (at 4 x 3 x 160 x 160 they are noise beside the VGG).  They implement
what the model passes -- reduction='mean', no element weight -- and refuse the rest.  PerceptualLoss runs its VGG19 through ONE
autograd node of the training engine (archs/nhwc_train.py: _VggLoss): output and GT as one batch through the HIP convolution
kernels, the input-gradient pass of the output image back through the same kernels, pooling / criterion / Gram matrices on
csrc/percep.hip.  GPU tensors only, like the ops.  r1_penalty's per-sample sum of squares and its backward are the kernels of
csrc/gan_reg.hip for GPU tensors and the torch expression for CPU tensors.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn

from ..archs.vgg_arch import VGGFeatureExtractor
from ..hip import MSSSIM_MAX_LEVELS   # (5: the levels the kernels of csrc/msssim.hip take)
from ..metrics import MSSSIM_WEIGHTS   # (0.0448, 0.2856, 0.3001, 0.2363, 0.1333): Wang, Simoncelli, Bovik 2003
from ..utils.registry import LOSS_REGISTRY


def _only_mean(name, reduction):
    if reduction != 'mean':
        raise NotImplementedError(f"{name}: reduction={reduction!r}; only 'mean' (what the model passes) is implemented")


def _no_weight(name, weight):
    if weight is not None:
        raise NotImplementedError(f'{name}: element-wise weights are not implemented (the model passes none)')


@LOSS_REGISTRY.register()
class L1Loss(nn.Module):
    """loss_weight * mean |pred - target|"""

    def __init__(self, loss_weight=1.0, reduction='mean'):
        super().__init__()
        _only_mean('L1Loss', reduction)
        self.loss_weight, self.reduction = loss_weight, reduction

    def forward(self, pred, target, weight=None, **kwargs):
        _no_weight('L1Loss', weight)
        return self.loss_weight * F.l1_loss(pred, target)


@LOSS_REGISTRY.register()
class MSELoss(nn.Module):
    """loss_weight * mean (pred - target)^2"""

    def __init__(self, loss_weight=1.0, reduction='mean'):
        super().__init__()
        _only_mean('MSELoss', reduction)
        self.loss_weight, self.reduction = loss_weight, reduction

    def forward(self, pred, target, weight=None, **kwargs):
        _no_weight('MSELoss', weight)
        return self.loss_weight * F.mse_loss(pred, target, reduction='none').mean()   # (the reference's operations: its gradient's bits)


@LOSS_REGISTRY.register()
class CharbonnierLoss(nn.Module):
    """loss_weight * mean sqrt((pred - target)^2 + eps).  The constructor's eps (default 1e-12) is what the reference's forward
    passes to charbonnier_loss (whose own default, 1e-6, is therefore never used)."""

    def __init__(self, loss_weight=1.0, reduction='mean', eps=1e-12):
        super().__init__()
        _only_mean('CharbonnierLoss', reduction)
        self.loss_weight, self.reduction, self.eps = loss_weight, reduction, eps

    def forward(self, pred, target, weight=None, **kwargs):
        _no_weight('CharbonnierLoss', weight)
        return self.loss_weight * torch.sqrt((pred - target)**2 + self.eps).mean()


@LOSS_REGISTRY.register()
class PerceptualLoss(nn.Module):
    """Perceptual loss with the style (Gram) loss.  forward(x, gt) -> (perceptual, style), each None when its weight is 0.

    norm_img: (x + 1) * 0.5 on both images before the VGG (the reference applies it although its images are in [0, 1]).
    Taps are the named layers of the VGG (conv taps before their ReLU).  Perceptual term: sum_k crit(x_k, gt_k) * w_k, times
    perceptual_weight, crit 'l1' (mean) or 'fro' (Frobenius norm).  Style term: sum_k l1(gram(x_k), gram(gt_k)) * w_k, times
    style_weight, gram = F F^T / (c h w) per image."""

    def __init__(self, layer_weights, vgg_type='vgg19', use_input_norm=True, perceptual_weight=1.0, style_weight=0, norm_img=True,
                 criterion='l1'):
        super().__init__()
        if criterion == 'l2':
            raise NotImplementedError("PerceptualLoss: criterion 'l2' -- the reference builds torch.nn.L2loss, which does not exist "
                                      "(it raises there as well); use 'l1' or 'fro'")
        if criterion not in ('l1', 'fro'):
            raise NotImplementedError(f'{criterion} criterion has not been supported in this version.')
        if style_weight > 0 and criterion == 'fro':
            raise NotImplementedError("PerceptualLoss: style_weight > 0 with criterion 'fro' -- the reference's style term then calls "
                                      'its criterion, which is None for fro; use criterion l1 for a style loss')
        if 'bn' in vgg_type:
            raise NotImplementedError(f'PerceptualLoss: vgg_type {vgg_type} (batch-normalised VGGs have no kernel here)')
        self.norm_img = norm_img
        self.perceptual_weight = perceptual_weight
        self.style_weight = style_weight
        self.layer_weights = layer_weights
        self.criterion_type = criterion
        self.vgg = VGGFeatureExtractor(layer_name_list=list(layer_weights.keys()), vgg_type=vgg_type, use_input_norm=use_input_norm)
        self._plan = None

    def forward(self, x, gt):
        from ..archs import nhwc_train
        if not (x.is_cuda and gt.is_cuda):
            raise NotImplementedError('PerceptualLoss: mrefsr_amd has no CPU path (HIP kernels only)')
        if not (self.perceptual_weight > 0 or self.style_weight > 0):
            return None, None
        if self._plan is None:
            self._plan = nhwc_train.VggLossPlan(self.vgg.vgg_net, self.layer_weights, self.criterion_type, self.perceptual_weight,
                                                self.style_weight, self.norm_img)
        totals = nhwc_train.perceptual(self.vgg, x, gt.detach(), self._plan)
        return (totals[0] if self.perceptual_weight > 0 else None), (totals[1] if self.style_weight > 0 else None)


@LOSS_REGISTRY.register()
class TextureLoss(nn.Module):
    """Texture loss of reference-based SR (basicsr/models/losses.py:430-532): the Gram matrices of the output's VGG features against
    those of the swapped reference maps, both weighted by the match confidence.

    forward(x, maps, weights) -> scalar.  maps: {layer: [B,C,s h,s w]} for the keys of layer_weights (relu3_1, relu2_1, relu1_1 at
    s = 1, 2, 4; the values of layer_weights are ignored, as in the reference); weights [B,1,h-2,w-2]: replicate-padded by 1, resized
    bicubically (align_corners) by s, coeff = sigmoid(-20 w + 0.65); per layer ||G(x_feat coeff) - G(maps coeff)||_F over the whole
    [B,C,C] tensor (G = F F^T per image, not normalised) / 4 / (x.shape[-1]^2 div)^2 with div = 256, 512, 1024; their sum / 3 *
    loss_weight.  The gradient reaches x only, and is exactly 0 for a layer whose norm is 0.  The caller's maps are not written to
    (the reference multiplies them by coeff in place).  Everything runs on the kernels of csrc/texture.hip and the VGG node of the
    training engine (archs/nhwc_train.py: _VggTexture); ``last_terms`` holds the per-layer terms of the last call (network order).

    Refused: use_weights=False (the reference's forward then reads a divisor it never set: UnboundLocalError), a dict of weights,
    other layers, batch-normalised VGGs, CPU tensors."""

    def __init__(self, use_weights=False, loss_weight=1.0, vgg_type='vgg19', layer_weights={'relu1_1': 1.0, 'relu2_1': 1.0, 'relu3_1': 1.0},
                 use_input_norm=True):
        super().__init__()
        if not use_weights:
            raise NotImplementedError("TextureLoss / texture_opt: use_weights: true is required -- without it the reference's forward fails "
                                      '(UnboundLocalError: div_num is only set on the use_weights path)')
        if 'bn' in vgg_type:
            raise NotImplementedError(f'TextureLoss: vgg_type {vgg_type} (batch-normalised VGGs have no kernel here)')
        from ..archs.nhwc_train import TEXTURE_LAYERS
        bad = [k for k in layer_weights if k not in TEXTURE_LAYERS]
        if bad or not layer_weights:
            raise NotImplementedError(f'TextureLoss: layers {sorted(layer_weights)}; only relu1_1, relu2_1 and relu3_1 have a scale and a '
                                      'divisor in the reference (it raises for any other)')
        self.use_weights = use_weights
        self.loss_weight = loss_weight
        self.vgg = VGGFeatureExtractor(layer_name_list=list(layer_weights.keys()), vgg_type=vgg_type, use_input_norm=use_input_norm)
        self._plan = None
        self.last_terms = None

    def forward(self, x, maps, weights=0):
        from ..archs import nhwc_train
        if isinstance(weights, dict):
            raise NotImplementedError('TextureLoss: a dict of per-layer weights is not implemented; pass the [B,1,h-2,w-2] tensor')
        if not torch.is_tensor(weights):
            raise NotImplementedError('TextureLoss: weights must be the [B,1,h-2,w-2] tensor of match values (use_weights)')
        if not (x.is_cuda and weights.is_cuda and all(torch.is_tensor(m) and m.is_cuda for m in maps.values())):
            raise NotImplementedError('TextureLoss: mrefsr_amd has no CPU path (HIP kernels only)')
        if self._plan is None:
            self._plan = nhwc_train.TextureLossPlan(self.vgg.vgg_net, list(self.vgg.layer_name_list), self.loss_weight)
        missing = [n for n in self._plan.names if n not in maps]
        if missing:
            raise ValueError(f'TextureLoss: maps has no entry for {missing}')
        total, terms = nhwc_train.texture(self.vgg, x, maps, weights, self._plan)
        self.last_terms = terms
        return total[0]


_SSIM_C1, _SSIM_C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def _ssim_planes(pred, target, channel):
    """(x, y) [P,1,H,W] at 255 scale of [B,3,H,W] images in the nominal range [0, 1]: channel 'y', one plane per image, X = 65.481 R +
    128.553 G + 24.966 B + 16 (metrics.rgb_to_y without its float32 round trip); 'rgb', three per image, X = 255 x"""
    if channel == 'y':
        coef = pred.new_tensor([65.481, 128.553, 24.966]).view(1, 3, 1, 1)
        x, y = (pred * coef).sum(1, keepdim=True) + 16.0, (target * coef).sum(1, keepdim=True) + 16.0
    else:
        x, y = 255.0 * pred, 255.0 * target
    return x.reshape(-1, 1, *x.shape[2:]), y.reshape(-1, 1, *y.shape[2:])


def _ssim_moments(x, y):
    """(mu1_sq, mu2_sq, mu1_mu2, s1, s2, s12) of planes x, y [P,1,H,W]: the window moments under the normalised 11-tap Gaussian of
    metrics._gaussian_window, applied separably on the valid region (metrics._filter_valid), in the planes' dtype"""
    from ..metrics import _gaussian_window
    k = torch.from_numpy(_gaussian_window(11, 1.5)).to(device=x.device, dtype=x.dtype)

    def filt(z):
        return F.conv2d(F.conv2d(z, k.view(1, 1, 11, 1)), k.view(1, 1, 1, 11))
    mu1, mu2 = filt(x), filt(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    return mu1_sq, mu2_sq, mu1_mu2, filt(x * x) - mu1_sq, filt(y * y) - mu2_sq, filt(x * y) - mu1_mu2


def _ssim_check_options(name, window_size, sigma, channel):
    if window_size != 11 or sigma != 1.5:
        raise NotImplementedError(f'{name}: window_size={window_size!r}, sigma={sigma!r}; only the 11-tap window with sigma 1.5 of '
                                  'the validation metric is implemented')
    if channel not in ('y', 'rgb'):
        raise NotImplementedError(f"{name}: channel={channel!r}; 'y' or 'rgb'")


def _ssim_check_images(name, pred, target, check_size):
    """the input checks of SSIMLoss and MSSSIMLoss in their order: [B,3,H,W], one shape, check_size(H, W), fp32 on the GPU"""
    if pred.dim() != 4 or pred.shape[1] != 3:
        raise NotImplementedError(f'{name}: [B,3,H,W] images expected, got {tuple(pred.shape)}')
    if target.shape != pred.shape:
        raise ValueError(f'{name}: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ')
    check_size(pred.shape[2], pred.shape[3])
    if pred.is_cuda and (pred.dtype != torch.float32 or target.dtype != torch.float32):
        raise NotImplementedError(f'{name}: {pred.dtype} / {target.dtype} images; fp32 only on the GPU')


def ssim_loss_torch(pred, target, channel='y'):
    """1 - mean SSIM map of [B,3,H,W] images in the nominal range [0, 1], as torch operations in the tensors' dtype and on their
    device: the definition SSIMLoss implements (and what it runs for CPU tensors).  Per plane of _ssim_planes the moments of
    _ssim_moments and the map of metrics._ssim with C1 = (0.01 255)^2, C2 = (0.03 255)^2.  Nothing is clamped or quantised."""
    mu1_sq, mu2_sq, mu1_mu2, s1, s2, s12 = _ssim_moments(*_ssim_planes(pred, target, channel))
    c1, c2 = _SSIM_C1, _SSIM_C2
    return 1.0 - (((2 * mu1_mu2 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))).mean()


class _SSIMLossFn(torch.autograd.Function):
    """(pred, target) [B,3,H,W] contiguous fp32 on the GPU -> loss_weight (1 - mean SSIM map), one launch of csrc/ssim_loss.hip; when
    pred needs a gradient the same launch writes the three coefficient maps its backward launch reads.  Differentiable once, towards
    pred only; the upstream gradient stays on the device."""

    @staticmethod
    def forward(ctx, pred, target, rgb, loss_weight):
        from .. import hip
        ctx.rgb, ctx.loss_weight = rgb, loss_weight
        loss, maps = hip.ssim_loss_fwd(pred, target, rgb, loss_weight, want_grad=ctx.needs_input_grad[0])
        if maps is not None:
            ctx.save_for_backward(pred, target, *maps)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        from .. import hip
        pred, target, *maps = ctx.saved_tensors
        return hip.ssim_loss_bwd(pred, target, maps, grad_loss.contiguous().float(), ctx.rgb, ctx.loss_weight), None, None, None


@LOSS_REGISTRY.register()
class SSIMLoss(nn.Module):
    """loss_weight * (1 - mean SSIM) between [B,3,H,W] images in the nominal range [0, 1]: the structural similarity the validation
    loop reports (metrics.calculate_ssim: 11 x 11 Gaussian window, sigma 1.5, valid region), as a differentiable criterion on the
    unquantised, unclamped images.  channel 'y': on the Y plane of every image (the SSIM-Y of validation); 'rgb': on the three colour
    planes at 255 scale.  The mean runs over images, planes and the (H - 10) x (W - 10) map positions; ssim_loss_torch spells the
    definition out.  target is a constant (detached); the gradient reaches pred, once.

    GPU fp32 tensors run on the kernels of csrc/ssim_loss.hip (one forward and one backward launch, a fixed summation order); CPU
    tensors of any float dtype take ssim_loss_torch.  Refused: window_size other than 11, sigma other than 1.5, another channel,
    inputs that are not 3-channel (NotImplementedError); H or W below 11, differing shapes (ValueError)."""

    def __init__(self, loss_weight=1.0, channel='y', window_size=11, sigma=1.5):
        super().__init__()
        _ssim_check_options('SSIMLoss', window_size, sigma, channel)
        self.loss_weight, self.channel, self.window_size, self.sigma = loss_weight, channel, window_size, sigma

    def check_size(self, h, w):
        if h < self.window_size or w < self.window_size:
            raise ValueError(f'SSIMLoss: {h} x {w} images are smaller than the {self.window_size}-tap window')

    def forward(self, pred, target, **kwargs):
        _ssim_check_images('SSIMLoss', pred, target, self.check_size)
        target = target.detach()
        if not pred.is_cuda:
            return self.loss_weight * ssim_loss_torch(pred, target, self.channel)
        return _SSIMLossFn.apply(pred.contiguous(), target.contiguous(), self.channel == 'rgb', float(self.loss_weight))


def msssim_levels_allowed(h, w):
    """the largest number of levels an H x W plane allows: every level at least 11 x 11 (0 when the plane itself is smaller)"""
    m = 0
    while m < MSSSIM_MAX_LEVELS and (min(h, w) >> m) >= 11:
        m += 1
    return m


def _msssim_check_size(name, h, w, levels):
    allowed = msssim_levels_allowed(h, w)
    if levels > allowed:
        raise ValueError(f'{name}: {h} x {w} images with M = {levels} levels: every level must be at least 11 x 11 '
                         f'(min(H, W) >> (M - 1) >= 11); this shape allows at most M = {allowed}')


def msssim_planes_torch(x, y, weights=MSSSIM_WEIGHTS):
    """v_p [P]: the MS-SSIM of each pair of planes x, y [P,1,H,W] at 255 scale, as torch operations in their dtype.  Level 1 is the
    plane, level j + 1 = F.avg_pool2d(level j, 2) (a trailing odd row or column is dropped); at every level the moments of
    _ssim_moments, C1 = (0.01 255)^2, C2 = (0.03 255)^2; F_j = mean cs for j < M, F_M = mean l cs;
    v = prod_j F_j^w_j when every F_j > 0, otherwise 0 with gradient exactly 0 (a rule: relu(F)^w would give 0 inf = NaN there)."""
    c1, c2 = _SSIM_C1, _SSIM_C2
    fs = []
    for j in range(len(weights)):
        if j:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
        mu1_sq, mu2_sq, mu1_mu2, s1, s2, s12 = _ssim_moments(x, y)
        m = (2 * s12 + c2) / (s1 + s2 + c2)
        if j == len(weights) - 1:
            m = m * ((2 * mu1_mu2 + c1) / (mu1_sq + mu2_sq + c1))
        fs.append(m.mean(dim=(1, 2, 3)))
    fs = torch.stack(fs, dim=1)                                        # [P, M]
    positive = (fs > 0).all(dim=1)
    safe = torch.where(positive[:, None], fs, torch.ones_like(fs))     # (no gradient reaches a plane under the zero rule)
    v = torch.exp((fs.new_tensor(list(weights)) * torch.log(safe)).sum(dim=1))
    return torch.where(positive, v, torch.zeros_like(v))


def msssim_loss_torch(pred, target, channel='y', weights=None):
    """1 - mean_p MS-SSIM of [B,3,H,W] images in the nominal range [0, 1], as torch operations in the tensors' dtype and on their
    device: the definition MSSSIMLoss implements (and what it runs for CPU tensors).  The planes of _ssim_planes (channel 'y': one
    per image; 'rgb': three per image), per plane msssim_planes_torch with weights (w_1 .. w_M), default MSSSIM_WEIGHTS, used as
    given.  Nothing is clamped or quantised."""
    weights = MSSSIM_WEIGHTS if weights is None else tuple(weights)
    return 1.0 - msssim_planes_torch(*_ssim_planes(pred, target, channel), weights).mean()


class _MSSSIMLossFn(torch.autograd.Function):
    """(pred, target) [B,3,H,W] contiguous fp32 on the GPU -> loss_weight (1 - mean MS-SSIM), three launches of csrc/msssim.hip; when
    pred needs a gradient they also write the pyramid, the coefficient maps and the multipliers the two backward launches read.
    Differentiable once, towards pred only; the upstream gradient stays on the device."""

    @staticmethod
    def forward(ctx, pred, target, rgb, loss_weight, weights):
        from .. import hip
        ctx.rgb, ctx.loss_weight, ctx.shape = rgb, loss_weight, tuple(pred.shape)
        loss, saved, _ = hip.msssim_loss_fwd(pred, target, weights, rgb, loss_weight, want_grad=ctx.needs_input_grad[0])
        if saved is not None:
            ctx.save_for_backward(*saved)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        from .. import hip
        return hip.msssim_loss_bwd(ctx.saved_tensors, grad_loss.contiguous().float(), ctx.shape, ctx.rgb, ctx.loss_weight), None, None, None, None


@LOSS_REGISTRY.register()
class MSSSIMLoss(nn.Module):
    """loss_weight * (1 - mean MS-SSIM) between [B,3,H,W] images in the nominal range [0, 1]: multi-scale SSIM (Wang, Simoncelli,
    Bovik 2003) with the window and constants of the validation metric at every level, as a differentiable criterion on the
    unquantised, unclamped images; msssim_loss_torch spells the definition out.  channel 'y' / 'rgb' as in SSIMLoss.  weights: one
    per level, M = 1 .. 5 of them, each finite and > 0, used as given (not renormalised); default MSSSIM_WEIGHTS (five levels).
    Level j + 1 is the 2 x 2 mean of level j; a trailing odd row or column is dropped (implementations differ there; for sides that
    are multiples of 2^(M-1) there is no odd line).  A plane with a level whose mean is not positive counts 0 and gets gradient 0.
    target is a constant (detached); the gradient reaches pred, once.

    GPU fp32 tensors run on the kernels of csrc/msssim.hip (three forward and two backward launches, fixed summation orders); CPU
    tensors of any float dtype take msssim_loss_torch.  Refused: window_size other than 11, sigma other than 1.5, another channel,
    inputs that are not 3-channel (NotImplementedError); bad weights, differing shapes, and images too small for M levels -- every
    level must be at least 11 x 11, so five levels need min(H, W) >= 176; fewer levels are never taken silently (ValueError)."""

    def __init__(self, loss_weight=1.0, channel='y', weights=None, window_size=11, sigma=1.5):
        super().__init__()
        _ssim_check_options('MSSSIMLoss', window_size, sigma, channel)
        weights = MSSSIM_WEIGHTS if weights is None else tuple(float(v) for v in weights)
        if not 1 <= len(weights) <= MSSSIM_MAX_LEVELS:
            raise ValueError(f'MSSSIMLoss: {len(weights)} weights; one per level, 1 to {MSSSIM_MAX_LEVELS} levels')
        if not all(math.isfinite(v) and v > 0 for v in weights):
            raise ValueError(f'MSSSIMLoss: weights={weights!r}; each must be finite and > 0')
        self.loss_weight, self.channel, self.weights, self.window_size, self.sigma = loss_weight, channel, weights, window_size, sigma

    def check_size(self, h, w):
        """ValueError when H x W images are too small for this criterion's levels"""
        _msssim_check_size('MSSSIMLoss', h, w, len(self.weights))

    def forward(self, pred, target, **kwargs):
        _ssim_check_images('MSSSIMLoss', pred, target, self.check_size)
        target = target.detach()
        if not pred.is_cuda:
            return self.loss_weight * msssim_loss_torch(pred, target, self.channel, self.weights)
        return _MSSSIMLossFn.apply(pred.contiguous(), target.contiguous(), self.channel == 'rgb', float(self.loss_weight), self.weights)


def _freq_residual_spectrum(pred, target, norm):
    return torch.fft.fft2(pred, norm=norm) - torch.fft.fft2(target, norm=norm)


def fft_loss_torch(pred, target, norm='backward'):
    """mean(|Re D| + |Im D|) / 2, D = fft2(pred, norm) - fft2(target, norm) over the last two dimensions of [B,C,H,W] tensors, full
    spectrum: F.l1_loss over the stacked real and imaginary parts, the FFT loss of MIMO-UNet / DeepRFT.  torch operations in the
    tensors' dtype and on their device: the definition FFTLoss implements (and what it runs for CPU tensors).  The subgradient at a
    zero component is 0."""
    d = torch.view_as_real(_freq_residual_spectrum(pred, target, norm))
    return d.abs().mean()


def focal_frequency_weight_torch(pred, target, alpha=1.0):
    """the spectrum weight matrix of the focal frequency loss [B,C,H,W], detached: |D|^alpha over its maximum in each (b, c) plane,
    NaN -> 0 (0 / 0 for equal images), clamped to [0, 1]; D the ortho-normalised residual spectrum"""
    d = torch.view_as_real(_freq_residual_spectrum(pred, target, 'ortho')).detach()
    w = torch.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2) ** alpha
    w = w / w.amax(dim=(-2, -1), keepdim=True)
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)
    return w.clamp(0.0, 1.0)


def focal_frequency_loss_torch(pred, target, alpha=1.0, weight=None):
    """mean(w (Re D^2 + Im D^2)) with D = fft2(pred, 'ortho') - fft2(target, 'ortho') and w = focal_frequency_weight_torch (a
    constant), the focal frequency loss of Jiang et al. ("Focal Frequency Loss for Image Reconstruction and Synthesis", ICCV 2021)
    with patch_factor 1 and without ave_spectrum / log_matrix / batch_matrix.  torch operations in the tensors' dtype and on their
    device: the definition FocalFrequencyLoss implements (and what it runs for CPU tensors).  ``weight``: a given weight matrix
    held fixed in place of the computed one."""
    d = torch.view_as_real(_freq_residual_spectrum(pred, target, 'ortho'))
    w = focal_frequency_weight_torch(pred, target, alpha) if weight is None else weight.detach()
    return (w * (d[..., 0] ** 2 + d[..., 1] ** 2)).mean()


class _FreqLossFn(torch.autograd.Function):
    """(pred, target) [B,C,H,W] contiguous fp32 on the GPU -> the frequency-domain loss on the kernels of csrc/freq_loss.hip; when
    pred needs a gradient the forward writes the coefficient-gradient map its backward transforms back.  Differentiable once,
    towards pred only; the upstream gradient stays on the device."""

    @staticmethod
    def forward(ctx, pred, target, focal, norm, alpha, loss_weight):
        from .. import hip
        ctx.loss_weight, ctx.shape = loss_weight, tuple(pred.shape)
        loss, g = hip.freq_loss_fwd(pred, target, focal, norm, alpha, loss_weight, want_grad=ctx.needs_input_grad[0])
        if g is not None:
            ctx.save_for_backward(g)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        from .. import hip
        g, = ctx.saved_tensors
        return hip.freq_loss_bwd(g, grad_loss.contiguous().float(), ctx.shape, ctx.loss_weight), None, None, None, None, None


def _freq_checked(name, pred, target):
    if pred.dim() != 4:
        raise ValueError(f'{name}: [B,C,H,W] images expected, got {tuple(pred.shape)}')
    if target.shape != pred.shape:
        raise ValueError(f'{name}: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ')
    if not (1 <= pred.shape[2] <= 1024 and 1 <= pred.shape[3] <= 1024):
        raise ValueError(f'{name}: {pred.shape[2]} x {pred.shape[3]} images; H and W of 1 ... 1024')
    if pred.is_cuda and not (pred.dtype == target.dtype == torch.float32):
        raise NotImplementedError(f'{name}: {pred.dtype} / {target.dtype} images; fp32 only on the GPU')
    return pred.is_cuda, target.detach()


@LOSS_REGISTRY.register()
class FFTLoss(nn.Module):
    """loss_weight * mean(|Re D| + |Im D|) / 2 with D = fft2(pred, norm) - fft2(target, norm) over the last two dimensions of
    [B,C,H,W] images (any C): the L1 distance of the stacked real and imaginary parts of the spectra (fft_loss_torch spells the
    definition out).  norm 'backward' (unnormalised, the widespread default) or 'ortho'.  target is a constant (detached); the
    gradient reaches pred, once; the subgradient at a zero component is 0.

    GPU fp32 tensors run on the kernels of csrc/freq_loss.hip (a dense DFT of pred - target on the f32 MFMA: two forward and two
    backward launches, fixed summation orders, no FFT library); CPU tensors of any float dtype take fft_loss_torch.  Refused: a
    reduction other than 'mean', another norm, non-fp32 tensors on the GPU (NotImplementedError); inputs that are not [B,C,H,W],
    differing shapes, H or W outside 1 ... 1024 (ValueError)."""

    def __init__(self, loss_weight=1.0, reduction='mean', norm='backward'):
        super().__init__()
        _only_mean('FFTLoss', reduction)
        if norm not in ('backward', 'ortho'):
            raise NotImplementedError(f"FFTLoss: norm={norm!r}; 'backward' or 'ortho'")
        self.loss_weight, self.reduction, self.norm = loss_weight, reduction, norm

    def forward(self, pred, target, **kwargs):
        on_gpu, target = _freq_checked('FFTLoss', pred, target)
        if not on_gpu:
            return self.loss_weight * fft_loss_torch(pred, target, self.norm)
        return _FreqLossFn.apply(pred.contiguous(), target.contiguous(), False, self.norm, 1.0, float(self.loss_weight))


@LOSS_REGISTRY.register()
class FocalFrequencyLoss(nn.Module):
    """loss_weight * mean(w |D|^2), the focal frequency loss (Jiang et al., ICCV 2021) of [B,C,H,W] images (any C): D the difference
    of the ortho-normalised spectra, w = |D|^alpha over its maximum in each (b, c) plane, NaN -> 0, clamped to [0, 1], a constant
    (focal_frequency_loss_torch spells the definition out).  alpha: any finite float >= 0 (0: w = 1, the mean squared error by
    Parseval).  target is a constant (detached); the gradient reaches pred, once.

    GPU fp32 tensors run on the kernels of csrc/freq_loss.hip (three forward and two backward launches, fixed orders); CPU tensors
    of any float dtype take focal_frequency_loss_torch.  Refused: patch_factor other than 1, ave_spectrum, log_matrix, batch_matrix,
    non-fp32 tensors on the GPU (NotImplementedError); an alpha that is not a finite number >= 0, inputs that are not [B,C,H,W],
    differing shapes, H or W outside 1 ... 1024 (ValueError)."""

    def __init__(self, loss_weight=1.0, alpha=1.0, patch_factor=1, ave_spectrum=False, log_matrix=False, batch_matrix=False):
        super().__init__()
        if isinstance(patch_factor, bool) or patch_factor != 1 or ave_spectrum or log_matrix or batch_matrix:
            raise NotImplementedError(f'FocalFrequencyLoss: patch_factor={patch_factor!r}, ave_spectrum={ave_spectrum!r}, log_matrix='
                                      f'{log_matrix!r}, batch_matrix={batch_matrix!r}; only patch_factor 1 with the three switches off '
                                      'is implemented')
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not (0.0 <= alpha < float('inf')):
            raise ValueError(f'FocalFrequencyLoss: alpha={alpha!r} is not a finite number >= 0')
        self.loss_weight, self.alpha = loss_weight, float(alpha)
        self.patch_factor, self.ave_spectrum, self.log_matrix, self.batch_matrix = 1, False, False, False

    def forward(self, pred, target, **kwargs):
        on_gpu, target = _freq_checked('FocalFrequencyLoss', pred, target)
        if not on_gpu:
            return self.loss_weight * focal_frequency_loss_torch(pred, target, self.alpha)
        return _FreqLossFn.apply(pred.contiguous(), target.contiguous(), True, 'ortho', self.alpha, float(self.loss_weight))


def _lowest_index_of(hit, dim):
    """the lowest index along ``dim`` at which the boolean tensor ``hit`` is set (every slice has one)"""
    n = hit.shape[dim]
    shape = [1] * hit.dim()
    shape[dim] = n
    idx = torch.arange(n, device=hit.device).view(shape)
    return torch.where(hit, idx, torch.full_like(idx, n)).amin(dim)


def _is_weight_sp(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and 0.0 <= v < 1.0


def contextual_loss_torch(x_feats, y_feats, band_width=0.5, jmin=None, imax=None, parts=False, weight_sp=0.0):
    """The contextual loss of one tap (Mechrez et al., "The Contextual Loss for Image Transformation with Non-Aligned Data", ECCV
    2018) as torch operations in the tensors' dtype and on their device: the definition ContextualLoss implements.  x_feats
    (features of the output) and y_feats (of the target, a constant) [B,C,h,w], N = h w; i runs over positions of x, j of y.
        mu[b,c] = mean_p y[b,c,p] (per sample);  xn = (x - mu) / max(|x - mu|_2, 1e-12) per position, yn the same from y;
        d[b,i,j] = 1 - <xn[b,:,i], yn[b,:,j]>;  m[b,i] = min_j d at jmin[b,i] (the lowest j on ties);
        w = exp((1 - d / (m + 1e-5)) / band_width);  cx = w / sum_j w;
        CX[b] = mean_j max_i cx[b,i,j] (the maximum at imax[b,j], the lowest i on ties);  loss = mean_b -log(CX[b] + 1e-5).
    weight_sp = ws in [0, 1) makes it the contextual bilateral loss, CoBi (Zhang et al., "Zoom to Learn, Learn to Zoom", ICCV 2019):
    with i = r_i w + c_i on the map's own grid,
        d_sp[i,j] = ((r_i - r_j)^2 + (c_i - c_j)^2) / (h^2 + w^2)   (an integer numerator, one division; in [0, 1));
        d[b,i,j]  = (1 - ws) (1 - <xn_i, yn_j>) + ws d_sp[i,j],
    and the row minimum, w, the normaliser, the column maximum and -log run on this d unchanged.  As in the authors' code the RAW
    distances are mixed and the mix is then made relative -- not a mix of two CX matrices; the normalisation of the squared offset by
    the grid's squared diagonal is this project's (the term is in [0, 1) like the cosine distance of centred features is in
    [0, 2], whatever the tap's size).  ws = 0 evaluates the expressions above as they stand.
    The gradient reaches x_feats only: through the selected element of each column, that row's normaliser, the row minimum at jmin,
    the normalisation and the centring (d_sp is a constant).  jmin [B,N] / imax [B,N] (integer tensors): given selections in place
    of the computed ones (the values, and so the gradient, route through them).  parts: -> (loss, dict(jmin, imax, CX [B],
    d [B,N,N], cx [B,N,N]))."""
    if x_feats.dim() != 4 or x_feats.shape != y_feats.shape:
        raise ValueError(f'contextual_loss_torch: two [B,C,h,w] feature maps of one shape expected, got {tuple(x_feats.shape)} and '
                         f'{tuple(y_feats.shape)}')
    if not (isinstance(band_width, (int, float)) and not isinstance(band_width, bool) and 0.0 < band_width < float('inf')):
        raise ValueError(f'contextual_loss_torch: band_width={band_width!r} is not a finite number > 0')
    if not _is_weight_sp(weight_sp):
        raise ValueError(f'contextual_loss_torch: weight_sp={weight_sp!r} is not a number in [0, 1)')
    b, c = x_feats.shape[:2]
    x, y = x_feats.reshape(b, c, -1), y_feats.detach().reshape(b, c, -1)
    if x.shape[2] < 2:
        raise ValueError(f'contextual_loss_torch: at least 2 positions expected, got {tuple(x_feats.shape)}')
    mu = y.mean(2, keepdim=True)
    xc, yc = x - mu, y - mu
    xn = xc / xc.norm(dim=1, keepdim=True).clamp_min(1e-12)
    yn = yc / yc.norm(dim=1, keepdim=True).clamp_min(1e-12)
    d = 1.0 - torch.bmm(xn.transpose(1, 2), yn)                                # [B, i, j]
    if weight_sp != 0:
        gh, gw = x_feats.shape[2:]
        p = torch.arange(gh * gw, device=d.device)
        r, q = p // gw, p % gw
        num = (r[:, None] - r[None, :]) ** 2 + (q[:, None] - q[None, :]) ** 2   # [i, j], integers
        d = (1.0 - weight_sp) * d + weight_sp * (num.to(d.dtype) / float(gh * gh + gw * gw))
    if jmin is None:
        jmin = _lowest_index_of(d == d.amin(2, keepdim=True), 2)
    m = d.gather(2, jmin.long().unsqueeze(2))                                  # [B, i, 1]
    w = torch.exp((1.0 - d / (m + 1e-5)) / band_width)
    cx = w / w.sum(2, keepdim=True)
    if imax is None:
        imax = _lowest_index_of(cx == cx.amax(1, keepdim=True), 1)
    cx_b = cx.gather(1, imax.long().unsqueeze(1)).squeeze(1).mean(1)           # [B]
    loss = (-torch.log(cx_b + 1e-5)).mean()
    if parts:
        return loss, dict(jmin=jmin, imax=imax, CX=cx_b.detach(), d=d.detach(), cx=cx.detach())
    return loss


def cx_patches_torch(img, size, stride):
    """img [B,3,H,W] -> its size x size patches at ``stride`` as a feature map [B, 3 size^2, oh, ow], oh = (H - size) // stride + 1,
    ow likewise, the channels in F.unfold's (c, dy, dx) order: what the RGB tap of ContextualLoss (rgb_patch) compares"""
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f'cx_patches_torch: a [B,3,H,W] image expected, got {tuple(img.shape)}')
    for name, v in (('size', size), ('stride', stride)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f'cx_patches_torch: {name}={v!r} is not an integer >= 1')
    b, _, h, w = img.shape
    if h < size or w < size:
        raise ValueError(f'cx_patches_torch: patches of {size} x {size} in an image of {h} x {w}')
    oh, ow = (h - size) // stride + 1, (w - size) // stride + 1
    rows = (torch.arange(oh, device=img.device) * stride)[:, None] + torch.arange(size, device=img.device)[None, :]   # [oh, dy]
    cols = (torch.arange(ow, device=img.device) * stride)[:, None] + torch.arange(size, device=img.device)[None, :]   # [ow, dx]
    p = img[:, :, rows[:, :, None, None], cols[None, None, :, :]]              # [B, 3, oh, dy, ow, dx]
    return p.permute(0, 1, 3, 5, 2, 4).reshape(b, 3 * size * size, oh, ow)


@LOSS_REGISTRY.register()
class ContextualLoss(nn.Module):
    """loss_weight * (rgb_patch.weight * tap_rgb + sum_k layer_weights[k] * contextual_loss(VGG_k(x), VGG_k(gt))), the RGB tap first,
    the named VGG taps in network order: the contextual loss of Mechrez et al. (ECCV 2018) with the cosine distance, the non-local
    term for targets that are not registered with the output to the pixel (contextual_loss_torch spells one tap out; the feature
    means are taken per sample, so a sample's loss and gradient are those it would get alone).  gt is a constant (detached); the
    gradient reaches x, once.  The VGG handling is PerceptualLoss's (taps are the named layers, conv taps before their ReLU;
    norm_img: (x + 1) * 0.5 on both images first).

    The three options of the contextual bilateral loss, CoBi (Zhang et al., "Zoom to Learn, Learn to Zoom", ICCV 2019):
      weight_sp   in [0, 1): the weight of the spatial term in every tap's distance (contextual_loss_torch), on the grid the tap is
                  evaluated on -- the strided or the patch grid.  0: the plain loss, on the plain kernels.
      tap_stride  {layer name: s >= 1}: that tap is evaluated on its positions (r s, c s) only; 1 where a name is absent.  Shallow
                  taps (relu2_2 of a 160^2 GT: 6400 positions) fit the bound of hip.CX_MAX_N positions that way.
      rgb_patch   {size, stride, weight}: one more tap, CoBi_RGB: the size x size patches of the images as given (after norm_img,
                  without the ImageNet mean / std) at that stride as features of 3 size^2 channels (cx_patches_torch).  With it
                  layer_weights may be empty: no VGG is built then.

    Everything runs on the VGG node of the training engine (archs/nhwc_train.py: _VggContextual) and the kernels of
    csrc/contextual.hip: the all-pairs similarity and the gradient product on the f32 MFMA, fixed summation orders (the same bits
    from call to call).  A tap may have at most hip.CX_MAX_N positions on the grid it is evaluated on (relu3 / conv3 taps of 256^2
    images at stride 1).

    Refused: batch-normalised VGGs, CPU tensors, non-fp32 tensors on the GPU, a tap over the bound (the message names the tap and
    suggests a stride), patches of more than 512 channels (size > 13) (NotImplementedError); inputs that are not [B,3,H,W],
    differing shapes, a band_width that is not a finite number > 0, a weight_sp outside [0, 1), a stride or size that is not an
    integer >= 1, a tap_stride for a layer that is no tap, empty layer_weights without rgb_patch (ValueError)."""

    def __init__(self, layer_weights, vgg_type='vgg19', use_input_norm=True, norm_img=False, band_width=0.5, loss_weight=1.0,
                 weight_sp=0.0, tap_stride=None, rgb_patch=None):
        super().__init__()
        if not isinstance(layer_weights, dict) or (not layer_weights and rgb_patch is None):
            raise ValueError(f'ContextualLoss: layer_weights={layer_weights!r}; a non-empty dict of VGG layer names and weights (it '
                             'may be empty with rgb_patch)')
        if isinstance(band_width, bool) or not isinstance(band_width, (int, float)) or not (0.0 < band_width < float('inf')):
            raise ValueError(f'ContextualLoss: band_width={band_width!r} is not a finite number > 0')
        if not _is_weight_sp(weight_sp):
            raise ValueError(f'ContextualLoss: weight_sp={weight_sp!r} is not a number in [0, 1)')
        if tap_stride is not None:
            if not isinstance(tap_stride, dict) or any(n not in layer_weights for n in tap_stride):
                raise ValueError(f'ContextualLoss: tap_stride={tap_stride!r}; a dict of strides for taps of layer_weights '
                                 f'{sorted(layer_weights)}')
            for n, s in tap_stride.items():
                if isinstance(s, bool) or not isinstance(s, int) or s < 1:
                    raise ValueError(f'ContextualLoss: tap {n}: tap_stride={s!r} is not an integer >= 1')
        if rgb_patch is not None:
            if not isinstance(rgb_patch, dict) or 'size' not in rgb_patch or set(rgb_patch) - {'size', 'stride', 'weight'}:
                raise ValueError(f'ContextualLoss: rgb_patch={rgb_patch!r}; a dict of size, stride (1) and weight (1.0)')
            rgb_patch = dict(size=rgb_patch['size'], stride=rgb_patch.get('stride', 1), weight=rgb_patch.get('weight', 1.0))
            for k in ('size', 'stride'):
                if isinstance(rgb_patch[k], bool) or not isinstance(rgb_patch[k], int) or rgb_patch[k] < 1:
                    raise ValueError(f'ContextualLoss: tap rgb_patch: {k}={rgb_patch[k]!r} is not an integer >= 1')
            if isinstance(rgb_patch['weight'], bool) or not isinstance(rgb_patch['weight'], (int, float)):
                raise ValueError(f'ContextualLoss: tap rgb_patch: weight={rgb_patch["weight"]!r} is not a number')
            if 3 * rgb_patch['size'] ** 2 > 512:
                raise NotImplementedError(f'ContextualLoss: tap rgb_patch: patches of size {rgb_patch["size"]} have '
                                          f'{3 * rgb_patch["size"] ** 2} channels; at most 512 (size <= 13)')
        if layer_weights and 'bn' in vgg_type:
            raise NotImplementedError(f'ContextualLoss: vgg_type {vgg_type} (batch-normalised VGGs have no kernel here)')
        self.layer_weights, self.norm_img = layer_weights, norm_img
        self.band_width, self.loss_weight = float(band_width), loss_weight
        self.weight_sp, self.tap_stride, self.rgb_patch = float(weight_sp), dict(tap_stride or {}), rgb_patch
        self.vgg = VGGFeatureExtractor(layer_name_list=list(layer_weights.keys()), vgg_type=vgg_type,
                                       use_input_norm=use_input_norm) if layer_weights else None
        self._plan = None

    def forward(self, x, gt):
        from ..archs import nhwc_train
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f'ContextualLoss: [B,3,H,W] images expected, got {tuple(x.shape)}')
        if gt.shape != x.shape:
            raise ValueError(f'ContextualLoss: x {tuple(x.shape)} and gt {tuple(gt.shape)} differ')
        if not (x.is_cuda and gt.is_cuda):
            raise NotImplementedError('ContextualLoss: mrefsr_amd has no CPU path (HIP kernels only; contextual_loss_torch is the '
                                      'definition of one tap in torch)')
        if not (x.dtype == gt.dtype == torch.float32):
            raise NotImplementedError(f'ContextualLoss: {x.dtype} / {gt.dtype} images; fp32 only on the GPU')
        if self._plan is None:
            self._plan = nhwc_train.ContextualLossPlan(self.vgg.vgg_net if self.vgg is not None else None, self.layer_weights,
                                                       self.band_width, self.loss_weight, self.norm_img, weight_sp=self.weight_sp,
                                                       tap_stride=self.tap_stride, rgb_patch=self.rgb_patch)
        return nhwc_train.contextual(self.vgg, x, gt.detach(), self._plan)[0]


def _ldl_residuals(gt, out, ema):
    """r = sum_c |gt - out| and r_e = sum_c |gt - ema|, [B,1,H,W], the channels added in the order 0, 1, 2"""
    d, e = (gt - out).abs(), (gt - ema).abs()
    return d[:, 0:1] + d[:, 1:2] + d[:, 2:3], e[:, 0:1] + e[:, 1:2] + e[:, 2:3]


def ldl_artifact_map_torch(gt, out, ema, ksize=7):
    """The artifact map w [B,1,H,W] of LDL (Liang et al., "Details or Artifacts: A Locally Discriminative Learning Approach to
    Realistic Image Super-Resolution", CVPR 2022; get_refined_artifact_map of basicsr/losses/loss_util.py) as torch operations in
    the tensors' dtype and on their device, differentiable towards ``out``: with r = sum_c |gt - out| and r_e = sum_c |gt - ema|,
        w = g v m,   g_b = Var(r_b)^(1/5) (unbiased, over the H W pixels of sample b),
                     v_p = the unbiased variance of r over the ksize x ksize window at p of the image reflect-padded by ksize // 2
                           (two passes: the window mean, then the squares about it),
                     m_p = [r_p >= r_e,p] (a constant).
    One deviation: a sample whose residual has exactly zero variance has g = 0 AND a zero gradient through g (the reference's
    autograd gives 0 * 0^(-4/5) = NaN there)."""
    if ksize % 2 != 1 or ksize < 3:
        raise ValueError(f'ldl_artifact_map_torch: ksize={ksize!r} is not an odd window size of at least 3')
    pad = ksize // 2
    if gt.dim() != 4 or min(gt.shape[2:]) <= pad:
        raise ValueError(f'ldl_artifact_map_torch: [B,C,H,W] images with H, W > {pad} expected, got {tuple(gt.shape)}')
    r, r_e = _ldl_residuals(gt, out, ema)
    flat = r.flatten(1)
    var = ((flat - flat.mean(1, keepdim=True)) ** 2).sum(1) / (flat.shape[1] - 1)
    positive = var > 0
    g = torch.where(positive, torch.where(positive, var, torch.ones_like(var)) ** 0.2, torch.zeros_like(var)).view(-1, 1, 1, 1)
    win = F.pad(r, [pad] * 4, mode='reflect').unfold(2, ksize, 1).unfold(3, ksize, 1).flatten(4)   # [B,1,H,W,ksize^2]
    v = ((win - win.mean(4, keepdim=True)) ** 2).sum(4) / (ksize * ksize - 1)
    return g * v * (r >= r_e).to(r.dtype)


def ldl_loss_torch(pred, target, pred_ema, ksize=7):
    """mean over [B,3,H,W] of |w pred - w target|, w = ldl_artifact_map_torch(target, pred, pred_ema, ksize) NOT detached (the
    reference differentiates through the map: realesrgan_model.py:211-226): the definition LDLLoss implements and what it runs for
    CPU tensors.  As w >= 0 this is sum_p w_p r_p / (3 B H W)."""
    w = ldl_artifact_map_torch(target, pred, pred_ema, ksize)
    return (w * pred - w * target).abs().mean()


class _LDLLossFn(torch.autograd.Function):
    """(pred, target, pred_ema) [B,3,H,W] contiguous fp32 on the GPU -> loss_weight mean |w pred - w target|, one launch of
    csrc/ldl_loss.hip; when pred needs a gradient the same launch writes the maps (m r, the window means, v m) and the per-sample
    scalars its backward launch reads.  Differentiable once, towards pred only; the upstream gradient stays on the device."""

    @staticmethod
    def forward(ctx, pred, target, pred_ema, loss_weight):
        from .. import hip
        ctx.loss_weight = loss_weight
        loss, saved, _ = hip.ldl_loss_fwd(pred, target, pred_ema, loss_weight, want_grad=ctx.needs_input_grad[0])
        if saved is not None:
            ctx.save_for_backward(pred, target, *saved)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        from .. import hip
        pred, target, *saved = ctx.saved_tensors
        return hip.ldl_loss_bwd(pred, target, saved, grad_loss.contiguous().float(), ctx.loss_weight), None, None, None


@LOSS_REGISTRY.register()
class LDLLoss(nn.Module):
    """The artifact loss of LDL (train.ldl_opt): loss_weight * mean |w pred - w target| with the artifact map w of
    ldl_artifact_map_torch built from pred, target and pred_ema, the output of the EMA network on the same input.  It penalises the
    pixels where pred is further from target than pred_ema is, each by how irregular the residual is around it.  w is not detached:
    the gradient towards pred flows through the local variances and the per-sample variance as well (DESIGN 3.16 has the closed
    form); target and pred_ema are constants.  A sample with a residual of exactly zero variance contributes no loss and no gradient.

    GPU fp32 tensors run on the kernels of csrc/ldl_loss.hip (one forward and one backward launch, fixed summation orders); CPU
    tensors of any float dtype take ldl_loss_torch.  ``artifact_map`` returns w [B,1,H,W] without a gradient.  Refused: ksize other
    than 7, inputs that are not [B,3,H,W], non-fp32 tensors on the GPU (NotImplementedError); H or W below 4, differing shapes
    (ValueError)."""

    def __init__(self, loss_weight=1.0, ksize=7):
        super().__init__()
        if isinstance(ksize, bool) or ksize != 7:
            raise NotImplementedError(f'LDLLoss: ksize={ksize!r}; only the 7 x 7 window of the paper is implemented')
        self.loss_weight, self.ksize = loss_weight, 7

    def _checked(self, pred, target, pred_ema):
        if pred.dim() != 4 or pred.shape[1] != 3:
            raise NotImplementedError(f'LDLLoss: [B,3,H,W] images expected, got {tuple(pred.shape)}')
        if target.shape != pred.shape or pred_ema.shape != pred.shape:
            raise ValueError(f'LDLLoss: pred {tuple(pred.shape)}, target {tuple(target.shape)} and pred_ema {tuple(pred_ema.shape)} differ')
        if pred.shape[2] < 4 or pred.shape[3] < 4:
            raise ValueError(f'LDLLoss: {pred.shape[2]} x {pred.shape[3]} images; H and W of at least 4 (the reflect padding of 3)')
        on_gpu = pred.is_cuda
        if on_gpu and not (pred.dtype == target.dtype == pred_ema.dtype == torch.float32):
            raise NotImplementedError(f'LDLLoss: {pred.dtype} / {target.dtype} / {pred_ema.dtype} images; fp32 only on the GPU')
        return on_gpu, target.detach(), pred_ema.detach()

    def forward(self, pred, target, pred_ema, **kwargs):
        on_gpu, target, pred_ema = self._checked(pred, target, pred_ema)
        if not on_gpu:
            return self.loss_weight * ldl_loss_torch(pred, target, pred_ema, self.ksize)
        return _LDLLossFn.apply(pred.contiguous(), target.contiguous(), pred_ema.contiguous(), float(self.loss_weight))

    def artifact_map(self, pred, target, pred_ema):
        """w [B,1,H,W] of the three images, without a gradient (the forward launch plus one that scales v m by g)"""
        on_gpu, target, pred_ema = self._checked(pred, target, pred_ema)
        with torch.no_grad():
            if not on_gpu:
                return ldl_artifact_map_torch(target, pred, pred_ema, self.ksize)
            from .. import hip
            return hip.ldl_loss_fwd(pred.detach().contiguous(), target.contiguous(), pred_ema.contiguous(), float(self.loss_weight),
                                    want_map=True)[2]


@LOSS_REGISTRY.register()
class GANLoss(nn.Module):
    """GAN loss of the adversarial step (basicsr/models/losses.py:275-356; wgan_softplus: basicsr/losses/losses.py:284-318): gan_type
    'vanilla', 'lsgan', 'wgan', 'wgan_softplus' or 'hinge'.

    forward(input, target_is_real, is_disc=False): vanilla = BCEWithLogits(input, label) (applied, as in the reference, to the
    discriminator's sigmoid output), lsgan = mean (input - label)^2, wgan = -mean(input) for real, mean(input) for fake,
    wgan_softplus = mean softplus(-input) for real, mean softplus(input) for fake (StyleGAN2's logistic loss for the discriminator,
    non-saturating loss for the generator), hinge = mean relu(1 -/+ input) for the discriminator and -mean(input) for the generator.
    Labels are real_label_val / fake_label_val (wgan and wgan_softplus: the bool itself); loss_weight multiplies the generator's loss
    only.  O(B) scalars: plain torch element-wise operations, which also gives every type its double backward towards the input
    (WGAN-GP and R1 differentiate the discriminator twice, not the loss) and a CPU path."""

    def __init__(self, gan_type, real_label_val=1.0, fake_label_val=0.0, loss_weight=1.0):
        super().__init__()
        if gan_type not in ('vanilla', 'lsgan', 'wgan', 'wgan_softplus', 'hinge'):
            raise NotImplementedError(f'GAN type {gan_type} is not implemented (vanilla, lsgan, wgan, wgan_softplus and hinge are).')
        self.gan_type, self.loss_weight = gan_type, loss_weight
        self.real_label_val, self.fake_label_val = real_label_val, fake_label_val
        self.loss = {'vanilla': nn.BCEWithLogitsLoss(), 'lsgan': nn.MSELoss(), 'wgan': self._wgan_loss,
                     'wgan_softplus': self._wgan_softplus_loss, 'hinge': nn.ReLU()}[gan_type]

    @staticmethod
    def _wgan_loss(input, target):
        return -input.mean() if target else input.mean()

    @staticmethod
    def _wgan_softplus_loss(input, target):
        return F.softplus(-input).mean() if target else F.softplus(input).mean()

    def get_target_label(self, input, target_is_real):
        if self.gan_type in ('wgan', 'wgan_softplus'):
            return target_is_real
        return input.new_ones(input.size()) * (self.real_label_val if target_is_real else self.fake_label_val)

    def forward(self, input, target_is_real, is_disc=False):
        if self.gan_type == 'hinge':
            if is_disc:
                loss = self.loss(1 + (-input if target_is_real else input)).mean()
            else:
                loss = -input.mean()
        else:
            loss = self.loss(input, self.get_target_label(input, target_is_real))
        return loss if is_disc else loss * self.loss_weight


def gradient_penalty_loss(discriminator, real_data, fake_data, mask=None):
    """WGAN-GP penalty mean_b (||d D(x_b) / d x_b||_2 - 1)^2 at x = alpha real + (1 - alpha) fake (basicsr/models/losses.py:
    359-395).  alpha [B,1,1,1] is drawn by torch.rand on the CPU generator, so under one seed it is the reference's.  The
    interpolate is a detached leaf: the penalty reaches the discriminator's parameters only.  The discriminator is differentiated
    twice (create_graph=True); ImageDiscriminator's nodes support that (archs/nhwc_disc.py)."""
    alpha = torch.rand(real_data.size(0), 1, 1, 1).to(real_data.device)
    interpolates = (alpha * real_data + (1. - alpha) * fake_data).detach().requires_grad_(True)
    disc_interpolates = discriminator(interpolates)
    gradients = torch.autograd.grad(outputs=disc_interpolates, inputs=interpolates, grad_outputs=torch.ones_like(disc_interpolates),
                                    create_graph=True, retain_graph=True, only_inputs=True)[0]
    if mask is not None:
        gradients = gradients * mask
    gradients = gradients.view(gradients.size(0), -1)
    return ((gradients.norm(2, dim=1) - 1)**2).mean()


class _R1SqNorm(torch.autograd.Function):
    """g [B, ...] -> [B]: the per-sample sum of squares of r1_penalty on the kernels of csrc/gan_reg.hip (fixed summation order).
    Its backward, 2 gs[b] g, is a kernel too and is not differentiable again: nothing differentiates the penalty a third time."""

    @staticmethod
    def forward(ctx, g):
        from .. import hip
        g = g.contiguous()
        ctx.save_for_backward(g)
        return hip.r1_sqnorm(g)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gs):
        from .. import hip
        g, = ctx.saved_tensors
        return hip.r1_sqnorm_bwd(g, gs.contiguous())


def r1_penalty(real_pred, real_img):
    """R1 regularisation mean_b ||d sum(D(x)) / d x_b||_2^2 on the real images (basicsr/losses/losses.py:391-405; Mescheder et al.,
    "Which training methods for GANs do actually converge?", eq. 9).  real_img is a leaf that requires grad and real_pred =
    D(real_img); the discriminator is differentiated twice (create_graph=True) through the nodes WGAN-GP uses.  GPU tensors: the sum
    of squares is one autograd node over csrc/gan_reg.hip (fp32 only); CPU tensors: the torch expression."""
    grad_real = torch.autograd.grad(outputs=real_pred.sum(), inputs=real_img, create_graph=True)[0]
    if not grad_real.is_cuda:
        return grad_real.pow(2).view(grad_real.shape[0], -1).sum(1).mean()
    if grad_real.dtype != torch.float32:
        raise NotImplementedError(f'r1_penalty: {grad_real.dtype} gradient; fp32 only on the GPU')
    return _R1SqNorm.apply(grad_real).mean()


@LOSS_REGISTRY.register()
class GradientPenaltyLoss(nn.Module):
    """loss_weight * gradient_penalty_loss (basicsr/models/losses.py:398-427)"""

    def __init__(self, loss_weight=1.):
        super().__init__()
        self.loss_weight = loss_weight

    def forward(self, discriminator, real_data, fake_data, mask=None):
        return gradient_penalty_loss(discriminator, real_data, fake_data, mask=mask) * self.loss_weight
