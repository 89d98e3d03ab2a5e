"""PSNR / SSIM protocol of the reference's validation loop, numpy only (no cv2):
tensor2img (basicsr/utils/img_util.py:38-94: squeeze, clamp to [0,1], HWC, *255, round, uint8) and
calculate_psnr (basicsr/metrics/psnr_ssim.py:11-48: crop_border, float64 MSE, 10 log10(255^2/mse)).
The reference swaps RGB->BGR with cv2 before the metric; PSNR over all channels is invariant to
that permutation, so it is not reproduced (Y-channel metrics use explicit BT.601 weights).

The functions named *_device, and validation_metrics, are the same metrics on the HIP kernels of csrc/metrics.hip: they take the
fp32 model tensors on the GPU (CPU tensors raise NotImplementedError) and copy back only a few scalars per image.  RGB PSNR is
bit-identical to calculate_psnr(tensor2img(.), tensor2img(.)); PSNR-Y and SSIM differ from the numpy functions only by the order of
their final sums (gate 1e-10; 7e-15 measured at 500 x 500)."""
import numpy as np
import torch


def tensor2img(tensor, out_type=np.uint8, min_max=(0, 1)):
    """(1|-,3|1,H,W) tensor -> HWC (or HW) ndarray, RGB order kept."""
    t = tensor.squeeze(0).float().detach().cpu().clamp_(*min_max)
    t = (t - min_max[0]) / (min_max[1] - min_max[0])
    if t.dim() == 3:
        img = t.numpy().transpose(1, 2, 0)
        if img.shape[2] == 1:
            img = np.squeeze(img, axis=2)
    elif t.dim() == 2:
        img = t.numpy()
    else:
        raise TypeError(f'Only support 3D or 2D tensor per image. But received with dimension: {t.dim()}')
    if out_type == np.uint8:
        img = (img * 255.0).round()
    return img.astype(out_type)


def rgb_to_y(img):
    """uint8/float [0,255] RGB HWC -> Y of YCbCr in [0,255] (float, not rounded):
    metric_util.py:31-45 via color_util bgr2ycbcr(y_only=True) coefficients."""
    img = img.astype(np.float32) / 255.
    y = np.dot(img, [65.481, 128.553, 24.966]) + 16.0
    return (y / 255.)[..., None] * 255.


def calculate_psnr(img, img2, crop_border, test_y_channel=False):
    assert img.shape == img2.shape, f'Image shapes are different: {img.shape}, {img2.shape}.'
    if img.ndim == 2:
        img, img2 = img[..., None], img2[..., None]
    if crop_border != 0:
        img = img[crop_border:-crop_border, crop_border:-crop_border, ...]
        img2 = img2[crop_border:-crop_border, crop_border:-crop_border, ...]
    if test_y_channel:
        img, img2 = rgb_to_y(img), rgb_to_y(img2)
    mse = np.mean((img.astype(np.float64) - img2.astype(np.float64))**2)
    if mse == 0:
        return float('inf')
    return 10. * np.log10(255. * 255. / mse)


def _gaussian_window(size=11, sigma=1.5):
    """the 1-D taps cv2.getGaussianKernel(11, 1.5) returns: exp(-(i - c)^2 / (2 sigma^2)), normalised to sum 1"""
    x = np.arange(size, dtype=np.float64) - (size - 1) / 2.0
    k = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return k / k.sum()


def _filter_valid(img, k):
    """separable correlation with taps k along both axes, 'valid' region only (= cv2.filter2D(...)[5:-5, 5:-5] with the
    outer-product window of psnr_ssim.py:187-190; the border handling of filter2D never reaches that region)"""
    n = len(k)
    rows = sum(k[i] * img[i:img.shape[0] - n + 1 + i, :] for i in range(n))
    return sum(k[j] * rows[:, j:rows.shape[1] - n + 1 + j] for j in range(n))


def _ssim(img, img2):
    """single-channel SSIM map mean (psnr_ssim.py:172-200): 11 x 11 Gaussian window sigma 1.5, c1 = (0.01*255)^2, c2 = (0.03*255)^2"""
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    k = _gaussian_window()
    mu1, mu2 = _filter_valid(img, k), _filter_valid(img2, k)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = _filter_valid(img * img, k) - mu1_sq
    s2 = _filter_valid(img2 * img2, k) - mu2_sq
    s12 = _filter_valid(img * img2, k) - mu1_mu2
    return float((((2 * mu1_mu2 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))).mean())


def calculate_ssim(img, img2, crop_border, test_y_channel=False):
    """psnr_ssim.py:85-129 (HWC uint8 / [0,255] images): per-channel SSIM averaged; Y channel as in calculate_psnr"""
    assert img.shape == img2.shape, f'Image shapes are different: {img.shape}, {img2.shape}.'
    if img.ndim == 2:
        img, img2 = img[..., None], img2[..., None]
    if crop_border != 0:
        img = img[crop_border:-crop_border, crop_border:-crop_border, ...]
        img2 = img2[crop_border:-crop_border, crop_border:-crop_border, ...]
    if test_y_channel:
        img, img2 = rgb_to_y(img), rgb_to_y(img2)
    img, img2 = img.astype(np.float64), img2.astype(np.float64)
    return float(np.mean([_ssim(img[..., i], img2[..., i]) for i in range(img.shape[2])]))


MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # Wang, Simoncelli, Bovik (Asilomar 2003): five levels


def _msssim_size(name, h, w):
    """every one of the five levels must hold the 11-tap window: min(h, w) >> 4 >= 11"""
    need = 11 << (len(MSSSIM_WEIGHTS) - 1)
    if min(h, w) < need:
        raise ValueError(f'{name}: a {h} x {w} image (after cropping) is too small for {len(MSSSIM_WEIGHTS)}-level MS-SSIM: '
                         f'both sides must be at least {need}')


def _msssim(img, img2, weights=MSSSIM_WEIGHTS):
    """single-channel MS-SSIM in float64: level j + 1 is the 2 x 2 mean of level j (a trailing odd row or column is dropped), every
    level with the window and constants of _ssim; prod_j F_j^w_j with F_j = mean cs below the last level and mean l cs there, 0 when
    an F_j is not positive (the definition of losses.msssim_loss_torch)"""
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    k = _gaussian_window()
    x, y = img, img2
    value = 1.0
    for j, wt in enumerate(weights):
        if j:
            h2, w2 = x.shape[0] // 2, x.shape[1] // 2
            x = x[:2 * h2, :2 * w2].reshape(h2, 2, w2, 2).mean(axis=(1, 3))
            y = y[:2 * h2, :2 * w2].reshape(h2, 2, w2, 2).mean(axis=(1, 3))
        mu1, mu2 = _filter_valid(x, k), _filter_valid(y, k)
        mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        s1 = _filter_valid(x * x, k) - mu1_sq
        s2 = _filter_valid(y * y, k) - mu2_sq
        s12 = _filter_valid(x * y, k) - mu1_mu2
        m = (2 * s12 + c2) / (s1 + s2 + c2)
        if j == len(weights) - 1:
            m = m * ((2 * mu1_mu2 + c1) / (mu1_sq + mu2_sq + c1))
        f = float(m.mean())
        if not f > 0:
            return 0.0
        value *= f ** wt
    return value


def calculate_msssim(img, img2, crop_border, test_y_channel=False):
    """five-level MS-SSIM of HWC uint8 / [0,255] images with calculate_ssim's cropping and Y plane: per-channel values averaged.
    The cropped image must be at least 176 x 176 (ValueError otherwise)"""
    assert img.shape == img2.shape, f'Image shapes are different: {img.shape}, {img2.shape}.'
    if img.ndim == 2:
        img, img2 = img[..., None], img2[..., None]
    if crop_border != 0:
        img = img[crop_border:-crop_border, crop_border:-crop_border, ...]
        img2 = img2[crop_border:-crop_border, crop_border:-crop_border, ...]
    _msssim_size('calculate_msssim', img.shape[0], img.shape[1])
    if test_y_channel:
        img, img2 = rgb_to_y(img), rgb_to_y(img2)
    img, img2 = img.astype(np.float64), img2.astype(np.float64)
    return float(np.mean([_msssim(img[..., i], img2[..., i]) for i in range(img.shape[2])]))


def imwrite(img, path):
    """HWC uint8 RGB image -> PNG (the reference converts to BGR and lets cv2.imwrite convert back: same file)"""
    import os
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(img).save(path)


def batch_psnr(output, gt, crop_border=4):
    """mean PSNR over a batch of (B,3,H,W) tensors with the protocol above."""
    vals = [calculate_psnr(tensor2img(output[i:i + 1]), tensor2img(gt[i:i + 1]), crop_border) for i in range(output.shape[0])]
    return float(np.mean(vals)), vals


# ------------------------------------------------------------------ device twins (csrc/metrics.hip)
def _device_batch(t):
    """[N,C,H,W] or [C,H,W] tensor -> (contiguous fp32 [N,C,H,W], whether it was one image)"""
    if not t.is_cuda:
        raise NotImplementedError(f'device metrics: tensor on {t.device}; use the numpy functions of this module on the host')
    single = t.dim() == 3
    t = t.detach().float().contiguous()
    return (t[None] if single else t), single


def tensor2img_device(tensor):
    """tensor2img on the GPU: [N,C,H,W] fp32 -> uint8 [N,H,W,C] device tensor, [C,H,W] -> [H,W,C]; one channel is squeezed
    ([N,H,W] / [H,W]) as tensor2img does.  Values equal tensor2img's bit for bit (NaN gives 0)."""
    from . import hip
    x, single = _device_batch(tensor)
    img = hip.tensor2img_u8(x)
    if img.shape[3] == 1:
        img = img[..., 0]
    return img[0] if single else img


def _psnr(sse, count):
    """calculate_psnr's last steps from a sum of squared differences (np.mean = sum / count)"""
    mse = np.float64(sse) / count
    if mse == 0:
        return float('inf')
    return 10. * np.log10(255. * 255. / mse)


def _device_metrics(output, gt, crop_border, sizes, ssim, return_img=False):
    """one set of kernel launches and one device-to-host copy of the per-image result rows.  ssim: None, 'y' or 'rgb'.
    -> (per-image dicts of psnr, psnr_y, finite and, when asked, ssim; the output's uint8 image or None; whether one image)"""
    from . import hip
    out, single = _device_batch(output)
    ref, single_gt = _device_batch(gt)
    if single != single_gt:
        raise ValueError(f'output {tuple(output.shape)} and GT {tuple(gt.shape)}: one image and a batch')
    n, _, h, w = out.shape
    if sizes is not None and single:
        sizes = [sizes]
    flags = {None: 0, 'y': hip.VALM_SSIM_Y, 'rgb': hip.VALM_SSIM_RGB}[ssim]
    res, img = hip.val_metrics(out, ref, crop_border, sizes=sizes, flags=flags, want_img=return_img)
    rows = res.cpu().numpy()
    sums = rows.view(np.float64)
    per = []
    for i in range(n):
        oh, ow = (int(v) for v in tuple(sizes[i])[:2]) if sizes is not None else (h, w)
        hc, wc = oh - 2 * crop_border, ow - 2 * crop_border
        d = dict(psnr=_psnr(int(rows[i, 0]), 3 * hc * wc), psnr_y=_psnr(sums[i, 2], hc * wc), finite=bool(rows[i, 1] == 0))
        m = (hc - 10) * (wc - 10)
        if ssim == 'y':      # calculate_ssim: float(np.mean([map.mean() per channel]))
            d['ssim'] = float(np.mean([sums[i, 3] / m]))
        elif ssim == 'rgb':
            d['ssim'] = float(np.mean([sums[i, 4 + c] / m for c in range(3)]))
        per.append(d)
    return per, img, single


def _msssim_y_device(output, gt, crop_border, sizes):
    """calculate_msssim(..., test_y_channel=True) of each image pair on the forward kernels of csrc/msssim.hip (no coefficient
    maps): the quantised, cropped images go back into [1,3,h,w] fp32 with torch operations (validation is not the hot path)"""
    from . import hip
    imgs = (hip.tensor2img_u8(_device_batch(output)[0]), hip.tensor2img_u8(_device_batch(gt)[0]))
    vals = []
    for i in range(imgs[0].shape[0]):
        oh, ow = (int(v) for v in tuple(sizes[i])[:2]) if sizes is not None else imgs[0].shape[1:3]
        _msssim_size('validation_metrics', oh - 2 * crop_border, ow - 2 * crop_border)
        pair = [(im[i, crop_border:oh - crop_border, crop_border:ow - crop_border].permute(2, 0, 1)[None].float() / 255.0).contiguous()
                for im in imgs]
        _, _, v = hip.msssim_loss_fwd(pair[0], pair[1], MSSSIM_WEIGHTS, rgb=False, want_values=True)
        vals.append(float(v[0]))
    return vals


def validation_metrics(output, gt, crop_border, sizes=None, return_img=False, msssim=False):
    """PSNR, PSNR-Y and SSIM-Y of each image pair, as calculate_psnr and calculate_ssim(test_y_channel=True) give them for
    tensor2img(output[i])[:oh, :ow] and tensor2img(gt[i])[:oh, :ow], computed on the GPU.
    output [N,3,H,W], gt [N,3,Hg,Wg] fp32 device tensors; sizes: None (equal shapes, whole images) or N pairs (oh, ow), the valid
    region of each image (the dataset's zero-padding crop).  Returns dict(psnr=[N], psnr_y=[N], ssim_y=[N], finite=[N]); finite is
    False for an image with NaN or inf in its valid region (its numbers are then those of the quantised values, NaN as 0).
    return_img: also 'img', the uint8 [N,H,W,3] device tensor of tensor2img(output[i]) for every image, uncropped.
    msssim: also 'msssim_y' [N], calculate_msssim(test_y_channel=True) of the same images on the kernels of csrc/msssim.hip."""
    if output.dim() != 4:
        raise ValueError(f'validation_metrics: expected [N,3,H,W] batches, got {tuple(output.shape)}')
    per, img, _ = _device_metrics(output, gt, crop_border, sizes, 'y', return_img)
    out = dict(psnr=[p['psnr'] for p in per], psnr_y=[p['psnr_y'] for p in per], ssim_y=[p['ssim'] for p in per],
               finite=[p['finite'] for p in per])
    if msssim:
        out['msssim_y'] = _msssim_y_device(output, gt, crop_border, sizes)
    if return_img:
        out['img'] = img
    return out


def calculate_psnr_device(output, gt, crop_border, test_y_channel=False, sizes=None):
    """calculate_psnr(tensor2img(output), tensor2img(gt), crop_border, test_y_channel) on the GPU, for fp32 tensors [3,H,W] (-> a
    number) or [N,3,H,W] (-> a list); sizes as in validation_metrics (one pair for a [3,H,W] image)"""
    per, _, single = _device_metrics(output, gt, crop_border, sizes, None)
    vals = [p['psnr_y' if test_y_channel else 'psnr'] for p in per]
    return vals[0] if single else vals


def calculate_ssim_device(output, gt, crop_border, test_y_channel=False, sizes=None):
    """calculate_ssim(tensor2img(output), tensor2img(gt), crop_border, test_y_channel) on the GPU; shapes as calculate_psnr_device"""
    per, _, single = _device_metrics(output, gt, crop_border, sizes, 'y' if test_y_channel else 'rgb')
    vals = [p['ssim'] for p in per]
    return vals[0] if single else vals
