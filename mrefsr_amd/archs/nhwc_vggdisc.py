"""Autograd nodes of VGGStyleDiscriminator (archs/discriminator_arch.py) on the kernels of csrc/disc_vgg.hip, with the image packing
and BatchNorm2d + LeakyReLU nodes of archs/nhwc_disc.py (_Pack, _Bn) as they are.

As in nhwc_disc.py, every backward is itself built from Functions over the same kernels, so the WGAN-GP penalty
(losses.gradient_penalty_loss: torch.autograd.grad(create_graph=True), then .backward()) differentiates the discriminator twice:
    _VConv       3x3 / stride 1 or 4x4 / stride 2 convolution (conv0_0: + bias + LeakyReLU in the epilogue)
                 backward = _LreluMask (conv0_0 only) -> _VConvDgrad (input) + _VConvWgrad / _BiasGrad (weight, bias; once differentiable)
    _VConvDgrad  backward = the convolution forward (d / d gy) and the weight-gradient kernel (d / d w)
    _LreluMask   g lrelu'(y): linear in g, so its backward is itself (the mask is piecewise constant: nothing flows to y)
    _LinearHead  NCHW flatten -> linear1 -> LeakyReLU -> linear2; backward = _LinearHeadBwd, whose backward is the head's double
                 backward (d gs, d w1, d w2; the gradients w.r.t. f, b1 and b2 are 0)
A backward computes only the gradients the running backward pass will use (nhwc_disc._wanted), so the penalty's first pass runs no
weight-gradient kernel, and neither does the G step, where D's parameters are frozen.
"""
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import hip
from . import nhwc_disc
from .nhwc_disc import SLOPE, _Bn, _c, _Pack, _wanted


class _VConv(Function):
    """y = conv(x, w, ks, stride ks - 2, pad 1) (+ b) (LeakyReLU when act) on [N,H,W,Cin] (Cin = 4 for the packed image)"""

    @staticmethod
    def forward(ctx, x, w, b, ks, act):
        ctx.ks, ctx.act = ks, act
        y = hip.disc_vconv(x, hip.disc_vconv_pack_weight(w, x.shape[3], dgrad=False), b, ks, SLOPE if act else None)
        ctx.save_for_backward(x, w, y if act else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        g = _LreluMask.apply(_c(gy), y.detach()) if ctx.act else _c(gy)
        dx = _VConvDgrad.apply(g, w, tuple(x.shape), ctx.ks) if _wanted(ctx, 0) else None
        dw = _VConvWgrad.apply(g, x, w.shape[1], ctx.ks) if _wanted(ctx, 1) else None
        db = _BiasGrad.apply(g) if _wanted(ctx, 2) else None
        return dx, dw, db, None, None


class _LreluMask(Function):
    """g lrelu'(y) (y the LeakyReLU's output, not differentiated)"""

    @staticmethod
    def forward(ctx, g, y):
        ctx.save_for_backward(y)
        return hip.disc_lrelu_mask(g, y, SLOPE)

    @staticmethod
    @once_differentiable
    def backward(ctx, gg):
        y, = ctx.saved_tensors
        return hip.disc_lrelu_mask(_c(gg), y, SLOPE) if ctx.needs_input_grad[0] else None, None


class _VConvDgrad(Function):
    """dx = the convolution's input gradient of gy (linear in gy and in w)"""

    @staticmethod
    def forward(ctx, gy, w, in_shape, ks):
        ctx.ks = ks
        ctx.save_for_backward(gy, w)
        return hip.disc_vconv_dgrad(gy, hip.disc_vconv_pack_weight(w, in_shape[3], dgrad=True), in_shape, ks)

    @staticmethod
    @once_differentiable
    def backward(ctx, ggx):
        gy, w = ctx.saved_tensors
        ggx = _c(ggx)
        d_gy = hip.disc_vconv(ggx, hip.disc_vconv_pack_weight(w, ggx.shape[3], dgrad=False), None, ctx.ks) if ctx.needs_input_grad[0] else None
        d_w = hip.disc_vconv_wgrad(ggx, gy, w.shape[1], ctx.ks) if ctx.needs_input_grad[1] else None
        return d_gy, d_w, None, None


class _VConvWgrad(Function):

    @staticmethod
    def forward(ctx, gy, x, cin_real, ks):
        return hip.disc_vconv_wgrad(x, gy, cin_real, ks)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        raise NotImplementedError('VGGStyleDiscriminator: the weight gradient is differentiated only once (nothing in the WGAN-GP step '
                                  'differentiates it)')


class _BiasGrad(Function):

    @staticmethod
    def forward(ctx, gy):
        return hip.disc_bias_grad(gy)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        raise NotImplementedError('VGGStyleDiscriminator: the bias gradient is differentiated only once')


class _LinearHead(Function):
    """f [N,H,W,C] -> linear2(lrelu(linear1(f.permute(0, 3, 1, 2).reshape(N, -1)))) [N]; w1 [J, C*H*W], w2 [J]"""

    @staticmethod
    def forward(ctx, f, w1, b1, w2, b2):
        out, hidden = hip.disc_linear_head(f, w1, b1, w2, b2, SLOPE)
        ctx.save_for_backward(f, w1, w2, hidden)
        return out

    @staticmethod
    def backward(ctx, gs):
        f, w1, w2, hidden = ctx.saved_tensors
        gf, gw1, gb1, gw2, gb2 = _LinearHeadBwd.apply(_c(gs), f, w1, w2, hidden, _wanted(ctx, 0), any(_wanted(ctx, i) for i in range(1, 5)))
        return gf, gw1, gb1, gw2, gb2


class _LinearHeadBwd(Function):

    @staticmethod
    def forward(ctx, gs, f, w1, w2, hidden, want_f, want_params):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(gs, w1, w2, hidden)
        return hip.disc_linear_head_bwd(gs, hidden, f, w1, w2, SLOPE, want_f=want_f, want_params=want_params)

    @staticmethod
    @once_differentiable
    def backward(ctx, ggf, ggw1, ggb1, ggw2, ggb2):
        if any(g is not None for g in (ggw1, ggb1, ggw2, ggb2)):
            raise NotImplementedError('VGGStyleDiscriminator: only the input gradient of the head is differentiated twice')
        if ggf is None:
            return (None, ) * 7
        gs, w1, w2, hidden = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_gs, d_w1, d_w2 = hip.disc_linear_head_dbl(_c(ggf), gs, hidden, w1, w2, SLOPE, want_gs=need[0], want_params=need[2] or need[3])
        return d_gs, None, d_w1, d_w2, None, None, None


def check_width(net, w):
    """the reference's linear1 takes num_feat * 8 * 5 * 5 features: the map after five floor halvings must be 5 wide"""
    wo = w
    for _ in range(5):
        wo //= 2
    if wo != 5:
        c = net.linear1.in_features // 25
        raise RuntimeError(f'VGGStyleDiscriminator: linear1 expects {net.linear1.in_features} input features (num_feat * 8 * 5 * 5); '
                           f'an image {w} wide is {wo} wide after five halvings, {c * 5 * wo} features')


def discriminator(net, x):
    """VGGStyleDiscriminator.forward on the kernels: x [B,3,H,W] (cuda, fp32) -> [B,1]"""
    check_width(net, x.shape[3])
    h = _Pack.apply(x)
    h = _VConv.apply(h, net.conv0_0.weight, net.conv0_0.bias, 3, True)
    for conv, bn in net.conv_bn_layers():
        h = _VConv.apply(h, conv.weight, None, conv.kernel_size[0], False)
        stats = (None, None, None) if nhwc_disc.statistics_frozen() else (bn.running_mean, bn.running_var, bn.num_batches_tracked)
        h = _Bn.apply(h, bn.weight, bn.bias, *stats, bn.eps, bn.momentum)
    out = _LinearHead.apply(h, net.linear1.weight, net.linear1.bias, net.linear2.weight.view(-1), net.linear2.bias)
    return out.view(-1, 1)
