"""Colour correction of test() outputs towards the LQ image (val.color_fix): the ``wavelet`` and ``adain`` "color fix" that StableSR
(Wang et al., IJCV 2024) introduced and DiffBIR, SUPIR and others reuse, on the kernels of csrc/color_fix.hip.

A network trained on targets that are not colour-registered with its input (contextual_opt / CoBi, texture_opt, style_opt, the
discriminators) reproduces the targets' white balance and carries the references' colour cast into its output; the image with the
right colours, the bicubic-upsampled LQ (``match_img_in``), is on the device for every batch anyway.  The fix keeps the output's
detail and takes the colours from that image.

No claim about image quality is made anywhere: only random-init weights were available when this was written.

x is the output, s the colour source, both [B,C,H,W]; every (b, c) plane is handled on its own.  ``sizes``: None, or B pairs
(h_b, w_b) with 1 <= h_b <= H, 1 <= w_b <= W -- the top-left rectangle of sample b is the image (the un-padded image of
MultiRefCUFEDSet): statistics and filters see it alone, with its border as the image border, and every pixel outside it keeps x's
bits.  Nothing is clamped to [0, 1]: tensor2img and the device metrics clamp as before.

    wavelet, levels L in 1..5 (default 5):  high_L(x) + low_L(s) = x + low_L(s - x);  low_0(v) = v,  low_i(v) = low_{i-1}(v)
             filtered with [1,2,1]^T [1,2,1] / 16 at dilation 2^(i-1), replicate padding at every stage;  high_L(v) = v - low_L(v)
    adain:   (x - mu_x) (sigma_s / sigma_x) + mu_s;  mu the mean, sigma = sqrt(var + 1e-5) with the unbiased variance (the
             calc_mean_std of StableSR); a rectangle of one pixel has no such variance: ValueError

The *_torch functions state the operators in plain torch for any floating dtype and device; they are the reference of the tests and
of tools/color_fix_times.py.  The operators have no backward: an inference-side step.
"""
import torch

TYPES = ('wavelet', 'adain')
OPTION_KEYS = ('type', 'levels')
MAX_LEVELS = 5
DEFAULT_LEVELS = 5
EPS = 1e-5


# ------------------------------------------------------------------ the option
def parse_color_fix(val_opt):
    """opt['val'] -> None (color_fix absent, None or False) or the checked configuration: {'type': 'wavelet', 'levels': L} or
    {'type': 'adain'}.  Accepted: 'wavelet' / 'adain' (the defaults) or a dict {type: ..., levels: L}.  Refused by name
    (ValueError): anything else -- unknown keys, a missing or unknown type, levels with adain, a levels that is not an int in 1..5
    (bools included)."""
    v = (val_opt or {}).get('color_fix')
    if v is None or v is False:
        return None
    if isinstance(v, str):
        v = {'type': v}
    if not isinstance(v, dict):
        raise ValueError(f"val.color_fix: {v!r} is not 'wavelet', 'adain' or a dict {{type: wavelet | adain, levels: L}}")
    unknown = sorted(set(v) - set(OPTION_KEYS), key=str)
    if unknown:
        raise ValueError(f'val.color_fix: unknown key(s) {unknown} ({", ".join(OPTION_KEYS)} are the options)')
    kind = v.get('type')
    if not isinstance(kind, str) or kind not in TYPES:
        raise ValueError(f'val.color_fix.type: {kind!r} is not one of {", ".join(TYPES)}')
    if kind == 'adain':
        if 'levels' in v:
            raise ValueError('val.color_fix.levels: adain has no levels (they belong to type: wavelet)')
        return {'type': 'adain'}
    levels = v.get('levels', DEFAULT_LEVELS)
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f'val.color_fix.levels: {levels!r} is not an int in 1..{MAX_LEVELS}')
    return {'type': 'wavelet', 'levels': levels}


# ------------------------------------------------------------------ the reference
def _rects(x, s, sizes):
    if x.dim() != 4 or x.numel() == 0 or s.shape != x.shape:
        raise ValueError(f'color_fix: two non-empty [B,C,H,W] tensors of one shape expected, got {tuple(x.shape)} and {tuple(s.shape)}')
    b, _, h, w = x.shape
    if sizes is None:
        return None
    rects = [tuple(int(v) for v in tuple(r)[:2]) for r in sizes]
    if len(rects) != b or any(len(r) != 2 for r in rects):
        raise ValueError(f'color_fix: sizes: {b} pairs (h_b, w_b) expected for a batch of {b}, got {sizes!r}')
    for hb, wb in rects:
        if not (1 <= hb <= h and 1 <= wb <= w):
            raise ValueError(f'color_fix: sizes: ({hb}, {wb}) is not inside the {h} x {w} planes (1 <= h_b <= H, 1 <= w_b <= W)')
    return rects


def _per_rect(fn, x, s, rects):
    """fn on the whole tensors, or per sample on its rectangle with the rest of the plane left as x"""
    if rects is None:
        return fn(x, s)
    out = x.clone()
    for b, (hb, wb) in enumerate(rects):
        # (contiguous crops: the reductions then run in the order they have on a tensor of that size)
        out[b:b + 1, :, :hb, :wb] = fn(x[b:b + 1, :, :hb, :wb].contiguous(), s[b:b + 1, :, :hb, :wb].contiguous())
    return out


def _blur_axis(v, r, dim):
    """[1,2,1] / 4 along ``dim`` at dilation r, the index clamped into the axis (replicate padding)"""
    n = v.shape[dim]
    i = torch.arange(n, device=v.device)
    a, c = v.index_select(dim, (i - r).clamp(0, n - 1)), v.index_select(dim, (i + r).clamp(0, n - 1))
    return 0.25 * (a + c) + 0.5 * v


def wavelet_low(v, levels):
    """low_L(v) of the last two axes: L stages, each [1,2,1] / 4 along W then along H at dilation 2^(i-1)"""
    for i in range(levels):
        v = _blur_axis(_blur_axis(v, 1 << i, -1), 1 << i, -2)
    return v


def wavelet_color_fix_torch(x, s, sizes=None, levels=DEFAULT_LEVELS):
    """high_L(x) + low_L(s), computed as x + low_L(s - x) (the filter is linear): one subtraction, the filter, one add"""
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f'color_fix: levels {levels!r} is not an int in 1..{MAX_LEVELS}')
    return _per_rect(lambda xr, sr: xr + wavelet_low(sr - xr, levels), x, s, _rects(x, s, sizes))


def _mean_std(v):
    var = v.var(dim=(2, 3), unbiased=True, keepdim=True)
    return v.mean(dim=(2, 3), keepdim=True), (var + EPS).sqrt()


def _adain(xr, sr):
    if xr.shape[2] * xr.shape[3] < 2:
        raise ValueError(f'color_fix: a valid rectangle of {xr.shape[2]} x {xr.shape[3]} = 1 pixel(s) has no unbiased variance '
                         '(at least 2 pixels needed)')
    (mu_x, sig_x), (mu_s, sig_s) = _mean_std(xr), _mean_std(sr)
    return (xr - mu_x) * (sig_s / sig_x) + mu_s


def adain_color_fix_torch(x, s, sizes=None):
    """(x - mu_x) (sigma_s / sigma_x) + mu_s per plane, mean and sqrt(unbiased variance + 1e-5) over the valid rectangle"""
    rects = _rects(x, s, sizes)
    for hb, wb in (rects if rects is not None else [tuple(x.shape[2:])]):   # (refused before anything is computed)
        if hb * wb < 2:
            raise ValueError(f'color_fix: a valid rectangle of {hb} x {wb} = {hb * wb} pixel(s) has no unbiased variance '
                             '(at least 2 pixels needed)')
    return _per_rect(_adain, x, s, rects)


# ------------------------------------------------------------------ the dispatcher
def color_fix(x, s, cfg, sizes=None):
    """x corrected towards s by the configuration ``cfg`` of parse_color_fix (None: x itself).  fp32 tensors on the GPU go to the
    HIP kernels (hip.color_fix_wavelet / hip.color_fix_adain), anything else to the torch forms above"""
    if cfg is None:
        return x
    on_kernels = x.is_cuda and s.is_cuda and x.dtype == torch.float32 and s.dtype == torch.float32
    if cfg['type'] == 'wavelet':
        if on_kernels:
            from . import hip
            return hip.color_fix_wavelet(x.contiguous(), s.contiguous(), sizes, cfg['levels'])
        return wavelet_color_fix_torch(x, s, sizes, cfg['levels'])
    if cfg['type'] == 'adain':
        if on_kernels:
            from . import hip
            return hip.color_fix_adain(x.contiguous(), s.contiguous(), sizes)
        return adain_color_fix_torch(x, s, sizes)
    raise ValueError(f'color_fix: unknown type {cfg["type"]!r}')
