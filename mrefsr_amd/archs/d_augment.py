"""Differentiable discriminator augmentation (train.d_augment): DiffAugment (Zhao et al., NeurIPS 2020) and the pixel / colour part
of ADA's pipeline (Karras et al., NeurIPS 2020) on the kernels of csrc/disc_augment.hip.

The same random transformation T stands in front of every discriminator call -- real and fake images, D's and G's updates -- so
the generator never learns the augmentations.  For fixed parameters T(x) = L x + b with L linear, hence the autograd pair below:
    _Augment      forward = L x + b (hip.disc_augment)      backward = _AugmentAdj
    _AugmentAdj   forward = L^T g  (hip.disc_augment_adj)   backward = _Augment without the bias
each the other's backward, as _Pack / _Unpack in archs/nhwc_disc.py: WGAN-GP and R1 differentiate through it twice.

No claim about image quality is made anywhere: only random-init weights were available when this was written.

Per sample (AugmentParams): fpar = {db, s, c, -} brightness offset, saturation factor, contrast factor; ipar = {flip, ty, tx, y0,
y1, x0, x1, -} horizontal flip, integer translation, cut box [y0,y1) x [x0,x1) clipped to the image.  d_augment_torch states the
formulas; it is the reference of the tests and of tools/d_augment_times.py.
"""
import math

import torch
from torch.autograd import Function

POLICY_OPS = {'color': ('brightness', 'saturation', 'contrast'), 'translation': ('translation', ), 'cutout': ('cutout', ),
              'flip': ('flip', )}
OPTION_KEYS = ('policy', 'p', 'brightness', 'saturation', 'contrast', 'translation', 'cutout', 'adaptive')
ADAPTIVE_KEYS = ('target', 'interval', 'speed_kimg')
ADAPTIVE_GAN_TYPES = ('vanilla', 'wgan_softplus', 'hinge')   # 0 is the real / fake boundary of D's output
DRAWS = 16   # uniforms per sample, see sample_d_augment


class AugmentParams:
    """the parameter tables of one call: ``packed`` is one int32 buffer of 12 B words, fpar = its first 4 B words read as fp32
    [B,4], ipar = the other 8 B [B,8] -- views, so that .to(device) is one copy.  ``contrast``: what the host knows, False when c = 1
    in every sample (the kernels then skip the per-sample sum launch)"""

    def __init__(self, packed, contrast):
        b = packed.numel() // 12
        self.packed, self.contrast = packed, bool(contrast)
        self.fpar = packed[:4 * b].view(torch.float32).view(b, 4)
        self.ipar = packed[4 * b:].view(b, 8)

    @classmethod
    def from_tables(cls, fpar, ipar, contrast=None):
        """fpar [B,3 or 4] {db, s, c}, ipar [B,7 or 8] {flip, ty, tx, y0, y1, x0, x1} (lists or tensors) -> AugmentParams on the CPU;
        contrast None: read from the table"""
        f = torch.as_tensor(fpar, dtype=torch.float32).reshape(-1, len(fpar[0]))
        i = torch.as_tensor(ipar, dtype=torch.int32).reshape(-1, len(ipar[0]))
        b = f.shape[0]
        packed = torch.zeros(12 * b, dtype=torch.int32)
        out = cls(packed, False)
        out.fpar[:, :f.shape[1]] = f
        out.ipar[:, :i.shape[1]] = i
        out.contrast = bool((out.fpar[:, 2] != 1).any()) if contrast is None else bool(contrast)
        return out

    def to(self, device):
        return AugmentParams(self.packed.to(device), self.contrast)


def identity_params(b):
    return AugmentParams.from_tables([[0., 1., 1.]] * b, [[0] * 7] * b, contrast=False)


def cut_box(h, w, ch, cw, cy, cx):
    """DiffAugment's cutout box of ch x cw around centre (cy, cx): rows cy - ch // 2 + [0, ch), clipped to the image (its clamped
    coordinates cover exactly the clipped box) -> (y0, y1, x0, x1)"""
    y0, x0 = cy - ch // 2, cx - cw // 2
    return max(0, min(h, y0)), max(0, min(h, y0 + ch)), max(0, min(w, x0)), max(0, min(w, x0 + cw))


# ------------------------------------------------------------------ the option
def _finite(name, v, lo=None, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (lo is not None and v < lo) or \
            (hi is not None and v > hi):
        rng = '' if lo is None and hi is None else f' in [{lo if lo is not None else "-inf"}, {hi if hi is not None else "inf"}]'
        raise ValueError(f'train.d_augment.{name}: {v!r} is not a finite number{rng}')
    return float(v)


def _range(name, v):
    if not isinstance(v, (list, tuple)) or len(v) != 2:
        raise ValueError(f'train.d_augment.{name}: [lo, hi] expected, got {v!r}')
    lo, hi = _finite(f'{name}[0]', v[0]), _finite(f'{name}[1]', v[1])
    if lo > hi:
        raise ValueError(f'train.d_augment.{name}: [{lo}, {hi}] is not ordered (lo <= hi)')
    return lo, hi


def parse_d_augment(opt, has_net_d=True, gan_type=None):
    """train.d_augment -> the checked configuration dict (every default filled in), or None without the option.  Refused by name
    (ValueError): unknown keys, an empty or unknown policy entry, p outside [0, 1], ranges that are not finite or not ordered, the
    option without network_d, unknown keys of ``adaptive`` and ``adaptive`` with a gan_type whose real / fake boundary is not 0."""
    if opt is None or opt is False:
        return None
    if not isinstance(opt, dict):
        raise ValueError(f'train.d_augment: a dict of options expected, got {opt!r}')
    if not has_net_d:
        raise ValueError('train.d_augment without network_d: the augmentation stands in front of a discriminator; give a network_d or '
                         'drop d_augment')
    unknown = sorted(set(opt) - set(OPTION_KEYS))
    if unknown:
        raise ValueError(f'train.d_augment: unknown key(s) {unknown} ({", ".join(OPTION_KEYS)} are the options)')
    policy = opt.get('policy')
    if isinstance(policy, str):
        policy = [s.strip() for s in policy.split(',')]
    if not isinstance(policy, (list, tuple)) or not policy:
        raise ValueError(f'train.d_augment.policy: a non-empty list (or comma-separated string) of {sorted(POLICY_OPS)} expected, got '
                         f'{opt.get("policy")!r}')
    for entry in policy:
        if entry not in POLICY_OPS:
            raise ValueError(f'train.d_augment.policy: unknown entry {entry!r} ({", ".join(POLICY_OPS)} are the operators)')
    cfg = dict(policy=tuple(dict.fromkeys(policy)),
               ops=tuple(op for entry in POLICY_OPS for op in POLICY_OPS[entry] if entry in policy),
               p=_finite('p', opt.get('p', 1.0), 0.0, 1.0),
               brightness=_finite('brightness', opt.get('brightness', 0.25), 0.0),
               saturation=_range('saturation', opt.get('saturation', [0.0, 2.0])),
               contrast=_range('contrast', opt.get('contrast', [0.5, 1.5])),
               translation=_finite('translation', opt.get('translation', 0.125), 0.0),
               cutout=_finite('cutout', opt.get('cutout', 0.5), 0.0, 1.0), adaptive=None)
    ada = opt.get('adaptive')
    if ada is not None and ada is not False:
        if not isinstance(ada, dict):
            raise ValueError(f'train.d_augment.adaptive: a dict of {list(ADAPTIVE_KEYS)} expected ({{}} for the defaults), got {ada!r}')
        unknown = sorted(set(ada) - set(ADAPTIVE_KEYS))
        if unknown:
            raise ValueError(f'train.d_augment.adaptive: unknown key(s) {unknown} ({", ".join(ADAPTIVE_KEYS)} are the options)')
        if gan_type not in ADAPTIVE_GAN_TYPES:
            raise ValueError(f'train.d_augment.adaptive with gan_type {gan_type!r}: the overfitting statistic is the mean sign of D on the '
                             f'real images, which needs 0 as the real / fake boundary ({", ".join(ADAPTIVE_GAN_TYPES)}); wgan and lsgan '
                             'have none there')
        interval = ada.get('interval', 4)
        if isinstance(interval, bool) or not isinstance(interval, int) or interval < 1:
            raise ValueError(f'train.d_augment.adaptive.interval: {interval!r} is not an int of at least 1')
        speed = _finite('adaptive.speed_kimg', ada.get('speed_kimg', 500), 0.0)
        if speed <= 0:
            raise ValueError(f'train.d_augment.adaptive.speed_kimg: {speed!r} is not above 0')
        cfg['adaptive'] = dict(target=_finite('adaptive.target', ada.get('target', 0.6)), interval=interval, speed_kimg=speed)
    return cfg


# ------------------------------------------------------------------ the sampler
def sample_d_augment(b, h, w, cfg, p, generator):
    """The parameter tables of one discriminator call (host side, pure) -> AugmentParams on the CPU.

    Order of draws, which a seed pins: ONE call ``torch.rand(b, 16, generator=generator, dtype=torch.float64)``; row i belongs to
    sample i, so a larger batch leaves the earlier samples' draws as they are, and every slot is drawn whether or not its operator
    is in the policy or switched on, so the policy and p do not move the other operators' values.  Slots of a row u:
        u[0] < p: brightness on,  db = (2 u[1] - 1) brightness
        u[2] < p: saturation on,  s  = lo + u[3] (hi - lo)            (saturation: [lo, hi])
        u[4] < p: contrast on,    c  = lo + u[5] (hi - lo)            (contrast: [lo, hi])
        u[6] < p: translation on, ty = floor(u[7] (2 ry + 1)) - ry, tx = floor(u[8] (2 rx + 1)) - rx,
                                  ry = round(h translation), rx = round(w translation)
        u[9] < p: cutout on,      box of ch x cw = round(h cutout) x round(w cutout) around (cy, cx), cy = floor(u[10] ny),
                                  cx = floor(u[11] nx), ny = h + 1 if ch is even else h, nx likewise; clipped to the image
        u[12] < p: flip on,       flip = u[13] < 0.5
        u[14], u[15]: not used.
    An operator that is off, or not in the policy, has its identity value.  The values are rounded to fp32 once, here."""
    u = torch.rand(b, DRAWS, generator=generator, dtype=torch.float64).tolist()
    ops = cfg['ops']
    ry, rx = int(round(h * cfg['translation'])), int(round(w * cfg['translation']))
    ch, cw = int(round(h * cfg['cutout'])), int(round(w * cfg['cutout']))
    ny, nx = h + 1 - ch % 2, w + 1 - cw % 2
    fpar, ipar = [], []
    for r in u:
        db, s, c, flip, ty, tx, box = 0.0, 1.0, 1.0, 0, 0, 0, (0, 0, 0, 0)
        if 'brightness' in ops and r[0] < p:
            db = (2.0 * r[1] - 1.0) * cfg['brightness']
        if 'saturation' in ops and r[2] < p:
            s = cfg['saturation'][0] + r[3] * (cfg['saturation'][1] - cfg['saturation'][0])
        if 'contrast' in ops and r[4] < p:
            c = cfg['contrast'][0] + r[5] * (cfg['contrast'][1] - cfg['contrast'][0])
        if 'translation' in ops and r[6] < p:
            ty, tx = int(r[7] * (2 * ry + 1)) - ry, int(r[8] * (2 * rx + 1)) - rx
        if 'cutout' in ops and r[9] < p:
            box = cut_box(h, w, ch, cw, int(r[10] * ny), int(r[11] * nx))
        if 'flip' in ops and r[12] < p:
            flip = int(r[13] < 0.5)
        fpar.append([db, s, c])
        ipar.append([flip, ty, tx, *box])
    return AugmentParams.from_tables(fpar, ipar)


# ------------------------------------------------------------------ the reference
def d_augment_torch(x, params, bias=True):
    """T(x) in plain differentiable torch, any floating dtype and device (the tables are converted exactly): x [B,3,H,W].  For
    output pixel (y, x) of sample b: 0 inside the cut box; sy = y - ty, sx0 = x - tx, 0 if outside the image; sx = W - 1 - sx0 under
    a flip; v = in[b, :, sy, sx] + db; mu = mean_ch v; u = s v + (1 - s) mu; m = mean over (3, H, W) of in[b] + db;
    out = c u + (1 - c) m.  bias=False: db taken as 0 (the linear part)."""
    b, ch, h, w = x.shape
    dev = x.device
    f, i = params.fpar.to(dev).to(x.dtype), params.ipar.to(dev).long()
    db, s, c = (f[:, k].view(b, 1, 1, 1) for k in range(3))
    if not bias:
        db = torch.zeros_like(db)
    flip, ty, tx, y0, y1, x0, x1 = (i[:, k].view(b, 1, 1) for k in range(7))
    ys, xs = torch.arange(h, device=dev).view(1, h, 1), torch.arange(w, device=dev).view(1, 1, w)
    sy, sx0 = ys - ty, xs - tx
    keep = (sy >= 0) & (sy < h) & (sx0 >= 0) & (sx0 < w) & ~((ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1))
    sx = torch.where(flip != 0, w - 1 - sx0, sx0)
    idx = (sy.clamp(0, h - 1) * w + sx.clamp(0, w - 1)).view(b, 1, h * w).expand(b, ch, h * w)
    v = x.reshape(b, ch, h * w).gather(2, idx).view(b, ch, h, w) + db
    mu = v.mean(1, keepdim=True)
    u = s * v + (1 - s) * mu
    m = x.mean((1, 2, 3), keepdim=True) + db
    out = c * u + (1 - c) * m
    return torch.where(keep.unsqueeze(1), out, torch.zeros((), dtype=x.dtype, device=dev))


# ------------------------------------------------------------------ the autograd pair
def _c(t):
    return t if t.is_contiguous() else t.contiguous()


class _Augment(Function):
    """x [B,3,H,W] fp32 on the GPU -> T(x); params: an AugmentParams on x's device (CPU tensors raise NotImplementedError)"""

    @staticmethod
    def forward(ctx, x, params, bias=True):
        from .. import hip
        ctx.params = params
        return hip.disc_augment(_c(x), params, bias)

    @staticmethod
    def backward(ctx, g):
        return _AugmentAdj.apply(g, ctx.params), None, None


class _AugmentAdj(Function):

    @staticmethod
    def forward(ctx, g, params):
        from .. import hip
        ctx.params = params
        return hip.disc_augment_adj(_c(g), params)

    @staticmethod
    def backward(ctx, gg):
        return _Augment.apply(gg, ctx.params, False), None


def d_augment(x, params):
    """T(x) on the HIP kernels, differentiable twice"""
    return _Augment.apply(x, params)


# ------------------------------------------------------------------ adaptive p (ADA's heuristic)
def all_reduce_words(words):
    """the accumulator's words summed over the ranks when torch.distributed is initialised (every rank then holds the same p);
    unchanged otherwise"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(words, op=dist.ReduceOp.SUM)
    return words


class AdaptiveP:
    """p follows the overfitting statistic r_t = E[sign(D(T(real)))] of ADA (Karras et al. 2020, eq. 1 and section 3.1): over
    ``interval`` D steps the device accumulates two words -- the sum over the images of sign(D) (the mean over an image's outputs
    for a discriminator with several per image) and the number of images --, every interval-th step reads them back once (summed
    over the ranks first) and moves p by count / (speed_kimg 1000) towards making r_t meet ``target``."""

    def __init__(self, p, target=0.6, interval=4, speed_kimg=500):
        self.p, self.target, self.interval, self.speed_kimg = float(p), float(target), int(interval), float(speed_kimg)
        self.steps, self.acc, self.rt = 0, None, None

    def update(self, p, sign_sum, count):
        """pure: (p, the two accumulated numbers) -> (the new p, r_t)"""
        if count <= 0:
            return p, None
        rt = sign_sum / count
        sign = (rt > self.target) - (rt < self.target)
        return min(1.0, max(0.0, p + sign * (count / (self.speed_kimg * 1000.0)))), rt

    def accumulate(self, real_pred):
        """real_pred: D(T(real)) of this D step, [B, ...] (detached here); device-side, no readback"""
        pred = real_pred.detach()
        words = torch.stack([torch.sign(pred).reshape(pred.shape[0], -1).double().mean(1).sum(),
                             torch.full((), float(pred.shape[0]), dtype=torch.float64, device=pred.device)])
        self.acc = words if self.acc is None else self.acc + words

    def read(self):
        """the one readback of an interval: (sign sum, count) over all ranks; clears the accumulator"""
        if self.acc is None:
            return 0.0, 0.0
        sign_sum, count = all_reduce_words(self.acc).tolist()
        self.acc = None
        return sign_sum, count

    def step(self):
        """call once per D step, behind accumulate: True when p was updated on this step"""
        self.steps += 1
        if self.steps % self.interval:
            return False
        self.p, rt = self.update(self.p, *self.read())
        self.rt = self.rt if rt is None else rt
        return True

    def state_dict(self):
        return dict(p=self.p, steps=self.steps, rt=self.rt, acc=None if self.acc is None else self.acc.tolist())

    def load_state_dict(self, state, device=None):
        self.p, self.steps, self.rt = float(state['p']), int(state.get('steps', 0)), state.get('rt')
        acc = state.get('acc')
        self.acc = None if acc is None else torch.tensor(acc, dtype=torch.float64, device=device)
