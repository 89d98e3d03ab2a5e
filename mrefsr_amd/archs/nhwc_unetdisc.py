"""Autograd nodes of UNetDiscriminatorSN (archs/discriminator_arch.py) on the kernels of csrc/disc_unet.hip, with the convolution
and LeakyReLU nodes of archs/nhwc_vggdisc.py (_VConv, _BiasGrad) and the image packing of archs/nhwc_disc.py (_Pack) as they are.

As in nhwc_vggdisc.py, every backward is itself built from Functions over the same kernels, so the WGAN-GP penalty
(losses.gradient_penalty_loss: torch.autograd.grad(create_graph=True), then .backward()) differentiates the discriminator twice:
    _SpectralNorm  W_orig -> W = W_orig / sigma for conv1 .. conv8 in one launch; backward (once differentiable: nothing in the
                   penalty differentiates it twice) dW_orig = G / sigma - (<G, W_orig> / sigma^2) u v^T with this forward's u, v, sigma
    _Up            bilinear x2 of y (+ skip): backward = _UpAdj (to y and to skip alike)
    _UpAdj         the adjoint (a gather); backward = _Up.  Both linear: each one's backward is the other
    _Add           x6 + x0; backward passes the gradient to both
    _Conv9         64 -> 1, 3x3, + bias; backward = _Conv9Dgrad (input) + _Conv9Wgrad / _BiasGrad (weight, bias; once differentiable)
    _Conv9Dgrad    backward = conv9's forward (d / d gy) and its weight-gradient kernel (d / d w)
The power iteration runs outside autograd, as torch's spectral_norm runs it under no_grad: once per forward in training mode, updating
weight_u / weight_v in place; each forward keeps its own snapshot of (u, v, sigma) for its backward (a D step runs three forwards
before one backward).  A backward computes only the gradients the running pass uses (nhwc_disc._wanted).
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import hip
from . import nhwc_disc
from .nhwc_disc import _c, _Pack, _wanted
from .nhwc_vggdisc import _BiasGrad, _VConv


class _SpectralNorm(Function):

    @staticmethod
    def forward(ctx, snap_u, snap_v, sigma, *w_origs):
        ctx.save_for_backward(snap_u, snap_v, sigma, *w_origs)
        return tuple(hip.disc_sn_scale(list(w_origs), sigma))

    @staticmethod
    @once_differentiable
    def backward(ctx, *gws):
        snap_u, snap_v, sigma, *w_origs = ctx.saved_tensors
        if not any(_wanted(ctx, 3 + i) for i in range(len(w_origs))):
            return (None, ) * (3 + len(w_origs))
        dws = hip.disc_sn_bwd([_c(g) for g in gws], w_origs, snap_u, snap_v, sigma)
        return (None, None, None, *[dw if ctx.needs_input_grad[3 + i] else None for i, dw in enumerate(dws)])


class _Up(Function):
    """up(y + skip), bilinear x2 with align_corners False (skip may be None)"""

    @staticmethod
    def forward(ctx, y, skip):
        ctx.has_skip = skip is not None
        return hip.disc_up2(y, skip)

    @staticmethod
    def backward(ctx, g):
        a = _UpAdj.apply(_c(g))
        return a, (a if ctx.has_skip else None)


class _UpAdj(Function):

    @staticmethod
    def forward(ctx, g):
        return hip.disc_up2_adj(g)

    @staticmethod
    def backward(ctx, gg):
        return _Up.apply(_c(gg), None)


class _Add(Function):

    @staticmethod
    def forward(ctx, a, b):
        return hip.disc_add(a, b)

    @staticmethod
    def backward(ctx, g):
        return g, g


class _Conv9(Function):
    """nn.Conv2d(C, 1, 3, 1, 1) + bias on [N,H,W,C] -> [N,H,W,1]"""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return hip.disc_conv9(x, w, b)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _c(gy)
        dx = _Conv9Dgrad.apply(gy, w) if _wanted(ctx, 0) else None
        dw = _Conv9Wgrad.apply(gy, x) if _wanted(ctx, 1) else None
        db = _BiasGrad.apply(gy) if _wanted(ctx, 2) else None
        return dx, dw, db


class _Conv9Dgrad(Function):

    @staticmethod
    def forward(ctx, gy, w):
        ctx.save_for_backward(gy, w)
        return hip.disc_conv9_dgrad(gy, w)

    @staticmethod
    @once_differentiable
    def backward(ctx, ggx):
        gy, w = ctx.saved_tensors
        ggx = _c(ggx)
        d_gy = hip.disc_conv9(ggx, w, None) if ctx.needs_input_grad[0] else None
        d_w = hip.disc_conv9_wgrad(ggx, gy) if ctx.needs_input_grad[1] else None
        return d_gy, d_w


class _Conv9Wgrad(Function):

    @staticmethod
    def forward(ctx, gy, x):
        return hip.disc_conv9_wgrad(x, gy)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        raise NotImplementedError('UNetDiscriminatorSN: the weight gradient is differentiated only once (nothing in the WGAN-GP step '
                                  'differentiates it)')


def check_size(net, h, w):
    """H and W multiples of 8 (three halvings, three doublings).  With the skips, the reference fails at the first add whose operands
    differ; without them it runs, but this engine does not"""
    if h % 8 == 0 and w % 8 == 0 and h > 0 and w > 0:
        return
    if not net.skip_connection:
        raise NotImplementedError(f'UNetDiscriminatorSN: input {h} x {w}; the kernels take sizes that are multiples of 8 (skip_connection '
                                  'False runs other sizes in the reference, not here)')
    s0 = (h, w)
    s1 = (s0[0] // 2, s0[1] // 2)
    s2 = (s1[0] // 2, s1[1] // 2)
    s3 = (s2[0] // 2, s2[1] // 2)
    for name, small, big in (('x4 + x2', s3, s2), ('x5 + x1', s2, s1), ('x6 + x0', s1, s0)):
        up = (2 * small[0], 2 * small[1])
        if up != big:
            raise RuntimeError(f'UNetDiscriminatorSN: the skip add {name} cannot run on a {h} x {w} input: the upsampled map is '
                               f'{up[0]} x {up[1]}, the skip {big[0]} x {big[1]} (the reference fails there too)')


def spectral_norm_weights(net, update):
    """one power iteration for conv1 .. conv8 when update (in place), else their stored u, v -> (W list, (snap_u, snap_v, sigma))"""
    convs = net.sn_convs()
    w_origs = [c.weight_orig for c in convs]
    with torch.no_grad():
        snap = hip.disc_sn_power([w.detach() for w in w_origs], [c.weight_u for c in convs], [c.weight_v for c in convs], update,
                                 net.sn_eps())
    return _SpectralNorm.apply(*snap, *w_origs), snap


def discriminator(net, x):
    """UNetDiscriminatorSN.forward on the kernels: x [B,3,H,W] (cuda, fp32) -> [B,1,H,W]"""
    n, _, h, w = x.shape
    check_size(net, h, w)
    ws, _ = spectral_norm_weights(net, net.training and not nhwc_disc.statistics_frozen())
    skip = net.skip_connection
    x0 = _VConv.apply(_Pack.apply(x), net.conv0.weight, net.conv0.bias, 3, True)
    x1 = _VConv.apply(x0, ws[0], None, 4, True)
    x2 = _VConv.apply(x1, ws[1], None, 4, True)
    x3 = _VConv.apply(x2, ws[2], None, 4, True)
    x4 = _VConv.apply(_Up.apply(x3, None), ws[3], None, 3, True)
    x5 = _VConv.apply(_Up.apply(x4, x2 if skip else None), ws[4], None, 3, True)
    x6 = _VConv.apply(_Up.apply(x5, x1 if skip else None), ws[5], None, 3, True)
    if skip:
        x6 = _Add.apply(x6, x0)
    out = _VConv.apply(x6, ws[6], None, 3, True)
    out = _VConv.apply(out, ws[7], None, 3, True)
    out = _Conv9.apply(out, net.conv9.weight, net.conv9.bias)
    return out.view(n, 1, h, w)
