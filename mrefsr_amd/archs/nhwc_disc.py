"""Autograd nodes of ImageDiscriminator (archs/discriminator_arch.py) on the kernels of csrc/disc.hip.

One Function per fused launch: image packing, 3x3 convolution, BatchNorm2d + LeakyReLU, and the head (pool -> 1x1 -> LeakyReLU
-> 1x1 -> sigmoid).  Each backward is itself built from Functions over the same kernels, so the gradient penalty of WGAN-GP
(losses.gradient_penalty_loss: torch.autograd.grad(create_graph=True), then .backward()) differentiates the discriminator twice:
    _Pack        backward = _Unpack                 (both linear: each one's backward is the other)
    _Conv        backward = _ConvDgrad (input) + _ConvWgrad (weight, bias; once differentiable)
    _ConvDgrad   backward = the convolution forward (d / d gy) and the weight-gradient kernel (d / d w)
    _Bn          backward = _BnBwd, whose backward is the double-backward kernel
    _Head        backward = _HeadBwd, whose backward is the head's double-backward kernel
Nothing needs a third derivative: the second-order nodes are once_differentiable.  A backward computes only the gradients the
running backward pass will use (torch._C._will_engine_execute_node on the node behind each input), so the penalty's first
pass, which wants the image gradient alone, runs no weight-gradient kernel.

Maps are channels-last fp32 [N,H,W,C]; the image enters as [B,3,H,W] and is packed to 4 channels.
"""
import contextlib

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import hip

SLOPE = 0.2
_frozen = [False]


@contextlib.contextmanager
def frozen_statistics():
    """inside: the BatchNorm layers normalise with batch statistics as in training, but leave running_mean / running_var /
    num_batches_tracked unchanged (a forward re-run on the range-free kernels must not count twice)"""
    prev = _frozen[0]
    _frozen[0] = True
    try:
        yield
    finally:
        _frozen[0] = prev


def statistics_frozen():
    return _frozen[0]


def _c(t):
    return t if t is None or t.is_contiguous() else t.contiguous()


def _wanted(ctx, i):
    """is the gradient of input i used by the backward pass being run?"""
    if not ctx.needs_input_grad[i]:
        return False
    node = ctx.next_functions[i][0]
    return node is None or torch._C._will_engine_execute_node(node)


class _Pack(Function):

    @staticmethod
    def forward(ctx, img):
        return hip.disc_pack_image(_c(img))

    @staticmethod
    def backward(ctx, g4):
        return _Unpack.apply(_c(g4))


class _Unpack(Function):

    @staticmethod
    def forward(ctx, g4):
        return hip.disc_unpack_image(_c(g4))

    @staticmethod
    def backward(ctx, g):
        return _Pack.apply(_c(g))


class _Conv(Function):
    """y = conv3x3(x, w, stride, pad 1) + b on [N,H,W,Cin] (Cin = 4 for the packed image, whose w has 3 input channels)"""

    @staticmethod
    def forward(ctx, x, w, b, stride):
        ctx.stride = stride
        ctx.save_for_backward(x, w)
        return hip.disc_conv3x3(x, hip.disc_conv_pack_weight(w, x.shape[3], dgrad=False), b, stride)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _c(gy)
        dx = _ConvDgrad.apply(gy, w, tuple(x.shape), ctx.stride) if _wanted(ctx, 0) else None
        dw = db = None
        if _wanted(ctx, 1) or _wanted(ctx, 2):
            dw, db = _ConvWgrad.apply(gy, x, w.shape[1], ctx.stride)
        return dx, dw, db, None


class _ConvDgrad(Function):
    """dx = conv3x3 input gradient of gy (linear in gy and in w)"""

    @staticmethod
    def forward(ctx, gy, w, in_shape, stride):
        ctx.stride, ctx.in_shape = stride, in_shape
        ctx.save_for_backward(gy, w)
        return hip.disc_conv3x3_dgrad(gy, hip.disc_conv_pack_weight(w, in_shape[3], dgrad=True), in_shape, stride)

    @staticmethod
    @once_differentiable
    def backward(ctx, ggx):
        gy, w = ctx.saved_tensors
        ggx = _c(ggx)
        d_gy = hip.disc_conv3x3(ggx, hip.disc_conv_pack_weight(w, ggx.shape[3], dgrad=False), None, ctx.stride) \
            if ctx.needs_input_grad[0] else None
        d_w = hip.disc_conv3x3_wgrad(ggx, gy, w.shape[1], ctx.stride) if ctx.needs_input_grad[1] else None
        return d_gy, d_w, None, None


class _ConvWgrad(Function):

    @staticmethod
    def forward(ctx, gy, x, cin_real, stride):
        return hip.disc_conv3x3_wgrad(x, gy, cin_real, stride), hip.disc_bias_grad(gy)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        raise NotImplementedError('ImageDiscriminator: the weight gradient is differentiated only once (nothing in the WGAN-GP step '
                                  'differentiates it)')


class _Bn(Function):
    """BatchNorm2d (training mode) + LeakyReLU(0.2); the running statistics are updated in place"""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum):
        y, mean, invstd = hip.disc_bn_lrelu(x, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, SLOPE)
        ctx.save_for_backward(x, gamma, y, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, y, mean, invstd = ctx.saved_tensors
        gx, gg, gb = _BnBwd.apply(_c(gy), x, gamma, y, mean, invstd)
        return gx, gg, gb, None, None, None, None, None


class _BnBwd(Function):
    """(gy, x, gamma) -> (gx, dgamma, dbeta); y (the LeakyReLU mask), mean and invstd are the forward's, not differentiated"""

    @staticmethod
    def forward(ctx, gy, x, gamma, y, mean, invstd):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(gy, x, gamma, y, mean, invstd)
        return hip.disc_bn_lrelu_bwd(gy, y, x, mean, invstd, gamma, SLOPE)

    @staticmethod
    @once_differentiable
    def backward(ctx, ggx, ggamma, gbeta):
        gy, x, gamma, y, mean, invstd = ctx.saved_tensors
        if ggx is None and ggamma is None and gbeta is None:
            return None, None, None, None, None, None
        if ggx is None:
            ggx = torch.zeros_like(x)
        want = tuple(ctx.needs_input_grad[:3])
        d_gy, d_x, d_g = hip.disc_bn_lrelu_dbl(_c(ggx), _c(ggamma), _c(gbeta), gy, y, x, mean, invstd, gamma, SLOPE, want)
        return d_gy, d_x, d_g, None, None, None


class _Head(Function):
    """f [N,H,W,C] -> sigmoid(w2 lrelu(w1 mean_hw(f) + b1) + b2) [N]; w1 [J,C], w2 [J] (views of the 1x1 weights)"""

    @staticmethod
    def forward(ctx, f, w1, b1, w2, b2):
        out, pooled, hidden = hip.disc_head(f, w1, b1, w2, b2, SLOPE)
        ctx.save_for_backward(f, w1, b1, w2, b2, out, pooled, hidden)
        return out

    @staticmethod
    def backward(ctx, gs):
        f, w1, b1, w2, b2, out, pooled, hidden = ctx.saved_tensors
        return _HeadBwd.apply(_c(gs), f, w1, b1, w2, b2, out, pooled, hidden)


class _HeadBwd(Function):

    @staticmethod
    def forward(ctx, gs, f, w1, b1, w2, b2, s, pooled, hidden):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(gs, w1, w2, s, pooled, hidden)
        gf, gw1, gb1, gw2, gb2 = hip.disc_head_bwd(gs, s, pooled, hidden, w1, w2, tuple(f.shape), SLOPE)
        return gf, gw1, gb1, gw2, gb2

    @staticmethod
    @once_differentiable
    def backward(ctx, ggf, ggw1, ggb1, ggw2, ggb2):
        if any(g is not None for g in (ggw1, ggb1, ggw2, ggb2)):
            raise NotImplementedError('ImageDiscriminator: only the input gradient of the head is differentiated twice')
        if ggf is None:
            return (None, ) * 9
        gs, w1, w2, s, pooled, hidden = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_gs, d_f, dw1, db1, dw2, db2 = hip.disc_head_dbl(_c(ggf), gs, s, pooled, hidden, w1, w2, SLOPE, want_gs=need[0], want_f=need[1],
                                                          want_params=any(need[2:6]))
        return d_gs, d_f, dw1, db1, dw2, db2, None, None, None


def discriminator(net, x):
    """ImageDiscriminator.forward on the kernels: x [B,3,H,W] (cuda, fp32) -> [B,1,1,1]"""
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d) and not (m.training and m.track_running_stats and m.momentum is not None):
            raise NotImplementedError('ImageDiscriminator: BatchNorm2d runs in training mode with running statistics and a momentum only '
                                      '(the model trains net_d; eval-mode statistics have no kernel here)')
    h = _Pack.apply(x)
    for blk in net.blocks():
        conv1, bn1, _, conv2, bn2, _ = blk
        for conv, bn, stride in ((conv1, bn1, 1), (conv2, bn2, 2)):
            h = _Conv.apply(h, conv.weight, conv.bias, stride)
            stats = (None, None, None) if statistics_frozen() else (bn.running_mean, bn.running_var, bn.num_batches_tracked)
            h = _Bn.apply(h, bn.weight, bn.bias, *stats, bn.eps, bn.momentum)
    head = net.out_block
    c1, c2 = head[1], head[3]
    out = _Head.apply(h, c1.weight.view(c1.out_channels, c1.in_channels), c1.bias, c2.weight.view(c2.in_channels), c2.bias)
    return out.view(-1, 1, 1, 1)
