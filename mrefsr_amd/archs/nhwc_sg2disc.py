"""Autograd nodes of StyleGAN2Discriminator (archs/discriminator_arch.py) on the kernels of csrc/disc_sg2.hip, with the 3x3 convolution,
LeakyReLU-mask, bias-gradient and linear-head nodes of archs/nhwc_vggdisc.py (_VConv, _LreluMask, _BiasGrad, _LinearHead) and the image
packing of archs/nhwc_disc.py (_Pack) as they are.

As in nhwc_vggdisc.py, every backward is itself built from Functions over the same kernels, so the WGAN-GP penalty
(losses.gradient_penalty_loss: torch.autograd.grad(create_graph=True), then .backward()) differentiates the discriminator twice:
    _Fir         the FIR in front of a stride-2 convolution (at stride 1 for conv2, at stride 2 for the skip, whose 1x1 / stride-2
                 convolution reads every second sample only); backward = _FirAdj, whose backward is _Fir (both linear)
    _SConv       3x3 / stride 2 or 1x1 / stride 1, pad 0: lrelu(conv(x, w) + b) + res in one launch
                 backward = _LreluMask -> _SConvDgrad (input) + _SConvWgrad / _BiasGrad (weight, bias; once differentiable); res gets gy
    _SConvDgrad  backward = the convolution forward (d / d gy) and the weight-gradient kernel (d / d w)

The exact scalings never get a pass of their own.  LeakyReLU is positively homogeneous, so sqrt(2) lrelu(conv(x, s w) + b) =
lrelu(conv(x, sqrt(2) s w) + sqrt(2) b), and a ResBlock's (sqrt(2) lrelu(v) + skip) / sqrt(2) = lrelu(v) + skip / sqrt(2): every factor
(the equalised-lr scale s = 1 / sqrt(cin k^2) included) is one torch multiplication of a weight or bias tensor, as the reference's own
`self.weight * self.scale` is, and autograd carries it into the stored parameter's gradient, twice differentiable.  The weights are packed
from those products at every use (a few microseconds per layer), as the sibling discriminators do.

The minibatch-stddev statistic works on the B x 4 x 4 x C map after the last ResBlock (32 K floats at B = 4, C = 512) whatever the image
size: it is composed of torch operations under autograd (var, sqrt, mean, cat), as GANLoss is, which also gives its double backward
towards the activations -- the term by which the penalty's gradient reaches every conv_body weight through the statistic.
"""
import math

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import hip
from .nhwc_disc import SLOPE, _c, _Pack, _wanted
from .nhwc_vggdisc import _BiasGrad, _LinearHead, _LreluMask, _VConv

SQRT2 = math.sqrt(2)


class _Fir(Function):
    """upfirdn2d(x, outer(taps, taps), down, pad) on [N,H,W,C]"""

    @staticmethod
    def forward(ctx, x, taps, pad, down):
        ctx.args = (taps, pad, down, tuple(x.shape))
        return hip.disc_sg2_fir(x, taps, pad, down)

    @staticmethod
    def backward(ctx, g):
        return _FirAdj.apply(_c(g), *ctx.args), None, None, None


class _FirAdj(Function):

    @staticmethod
    def forward(ctx, g, taps, pad, down, in_shape):
        ctx.args = (taps, pad, down)
        return hip.disc_sg2_fir(g, taps, pad, down, adjoint_shape=in_shape)

    @staticmethod
    def backward(ctx, gg):
        return _Fir.apply(_c(gg), *ctx.args), None, None, None, None


class _SConv(Function):
    """y = lrelu(conv(x, w, ks, stride 2 if ks == 3 else 1, pad 0) + b) (LeakyReLU when act) + res on [N,H,W,Cin] (Cin = 4 for the packed
    image); an activated layer takes no res (the mask is read from y's sign)"""

    @staticmethod
    def forward(ctx, x, w, b, res, ks, act):
        assert not (act and res is not None)
        ctx.ks, ctx.act = ks, act
        y = hip.disc_sg2_conv(x, hip.disc_sg2_pack_weight(w, x.shape[3], dgrad=False), b, ks, SLOPE if act else None, res)
        ctx.save_for_backward(x, w, y if act else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        g = _LreluMask.apply(_c(gy), y.detach()) if ctx.act else _c(gy)
        dx = _SConvDgrad.apply(g, w, tuple(x.shape), ctx.ks) if _wanted(ctx, 0) else None
        dw = _SConvWgrad.apply(g, x, w.shape[1], ctx.ks) if _wanted(ctx, 1) else None
        db = _BiasGrad.apply(g) if _wanted(ctx, 2) else None
        return dx, dw, db, (gy if ctx.needs_input_grad[3] else None), None, None


class _SConvDgrad(Function):
    """dx = the convolution's input gradient of gy (linear in gy and in w)"""

    @staticmethod
    def forward(ctx, gy, w, in_shape, ks):
        ctx.ks = ks
        ctx.save_for_backward(gy, w)
        return hip.disc_sg2_conv_dgrad(gy, hip.disc_sg2_pack_weight(w, in_shape[3], dgrad=True), in_shape, ks)

    @staticmethod
    @once_differentiable
    def backward(ctx, ggx):
        gy, w = ctx.saved_tensors
        ggx = _c(ggx)
        d_gy = hip.disc_sg2_conv(ggx, hip.disc_sg2_pack_weight(w, ggx.shape[3], dgrad=False), None, ctx.ks) if ctx.needs_input_grad[0] else None
        d_w = hip.disc_sg2_conv_wgrad(ggx, gy, w.shape[1], ctx.ks) if ctx.needs_input_grad[1] else None
        return d_gy, d_w, None, None


class _SConvWgrad(Function):

    @staticmethod
    def forward(ctx, gy, x, cin_real, ks):
        return hip.disc_sg2_conv_wgrad(x, gy, cin_real, ks)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        raise NotImplementedError('StyleGAN2Discriminator: the weight gradient is differentiated only once (nothing in the WGAN-GP step '
                                  'differentiates it)')


def check_input(net, x):
    """the reference runs any input through conv_body and fails in final_linear when the last map is not 4 x 4"""
    b, _, h, w = x.shape
    if (h, w) != (net.out_size, net.out_size):
        n = net.final_linear[0].in_channels
        raise RuntimeError(f'StyleGAN2Discriminator: final_linear expects {n} input features (a 4 x 4 map from a {net.out_size} x '
                           f'{net.out_size} image); the input is {h} x {w} (the reference fails in final_linear too)')
    group = min(b, net.stddev_group)
    if b % group:
        raise RuntimeError(f'StyleGAN2Discriminator: a batch of {b} is not divisible by the minibatch-stddev group of {group} '
                           f'(min(batch, stddev_group={net.stddev_group})); the reference\'s view fails there too')
    return group


def stddev_channel(h, group):
    """h [B,4,4,C] -> [B,4,4,C + 4]: channel C = the group statistic, sqrt(var over the group + 1e-8) averaged over C, H, W and repeated
    over the group (sample b belongs to set b % (B / group)); channels C + 1 .. C + 3 = 0 pad the convolution operand to a multiple of 4"""
    b, hh, ww, c = h.shape
    sd = torch.sqrt(h.view(group, b // group, hh, ww, c).var(0, unbiased=False) + 1e-8).mean([1, 2, 3])
    sd = sd.repeat(group).view(b, 1, 1, 1).expand(b, hh, ww, 1)
    return torch.cat([h, sd, h.new_zeros(b, hh, ww, 3)], 3)


def discriminator(net, x):
    """StyleGAN2Discriminator.forward on the kernels: x [B,3,out_size,out_size] (cuda, fp32) -> [B,1]"""
    group = check_input(net, x)
    taps = net.resample_taps
    conv0, act0 = net.conv_body[0][0], net.conv_body[0][1]
    h = _SConv.apply(_Pack.apply(x), conv0.weight * (conv0.scale * SQRT2), act0.bias * SQRT2, None, 1, True)
    for block in list(net.conv_body)[1:]:
        c1, a1 = block.conv1[0], block.conv1[1]
        fir2, c2, a2 = block.conv2[0], block.conv2[1], block.conv2[2]
        firs, cs = block.skip[0], block.skip[1]
        t = _VConv.apply(h, c1.weight * (c1.scale * SQRT2), a1.bias * SQRT2, 3, True)
        t = _SConv.apply(_Fir.apply(t, taps, fir2.pad, 1), c2.weight * c2.scale, a2.bias, None, 3, True)
        h = _SConv.apply(_Fir.apply(h, taps, firs.pad, 2), cs.weight * (cs.scale / SQRT2), None, t, 1, False)
    h = stddev_channel(h, group)
    cf, af = net.final_conv[0], net.final_conv[1]
    h = _VConv.apply(h, cf.weight * (cf.scale * SQRT2), af.bias * SQRT2, 3, True)
    l1, l2 = net.final_linear
    out = _LinearHead.apply(h, l1.weight * (l1.scale * SQRT2), l1.bias * (l1.lr_mul * SQRT2), (l2.weight * l2.scale).view(-1), l2.bias * l2.lr_mul)
    return out.view(-1, 1)
