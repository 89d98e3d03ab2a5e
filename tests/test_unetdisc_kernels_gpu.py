"""GPU: the kernels of csrc/disc_unet.hip (UNetDiscriminatorSN) and disc_vgg.hip's convolutions at the U-Net's layer shapes, against
fp64 torch on the CPU.

Gate: max abs error <= 2e-5 * max |reference| (the csrc/disc.hip gate) for every map; u, v and sigma of the spectral norm to 1e-5.
Shapes: every layer of UNetDiscriminatorSN(3, 64) at 160 x 160 (B = 4) and at 16 x 24 (B = 2), where the upsampled maps start
from 2 x 3 and every border case of the bilinear weights is hit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth_unetdisc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SIZES = [(4, 160, 160), (2, 16, 24)]


def _close(got, want, rel=2e-5):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    assert err <= rel * scale + 1e-30, (err, scale)


def _net(nf=64):
    from mrefsr_amd.archs.discriminator_arch import UNetDiscriminatorSN
    net = UNetDiscriminatorSN(3, nf)
    spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth_unetdisc.state_dict(spec).items()}, strict=True)
    return net


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _sn64(w, u, v):
    """torch's spectral_norm power iteration (one step, eps 1e-12) in fp64 -> (u, v, sigma)"""
    m = w.double().reshape(w.shape[0], -1)
    v = F.normalize(m.t() @ u.double(), dim=0, eps=1e-12)
    u = F.normalize(m @ v, dim=0, eps=1e-12)
    return u, v, torch.dot(u, m @ v)


def test_spectral_norm_power_iteration_and_buffers():
    """u, v, sigma of all eight layers against fp64; the buffers updated in place in training mode, left alone in eval mode"""
    from mrefsr_amd import hip
    net = _net().to(DEV)
    convs = net.sn_convs()
    u0 = [c.weight_u.clone() for c in convs]
    v0 = [c.weight_v.clone() for c in convs]
    ptrs = [(c.weight_u.data_ptr(), c.weight_v.data_ptr()) for c in convs]
    w = [c.weight_orig.detach() for c in convs]
    su, sv, sigma = hip.disc_sn_power(w, [c.weight_u for c in convs], [c.weight_v for c in convs], True)
    ou = ov = 0
    for i, c in enumerate(convs):
        wu, wv, ws = _sn64(w[i].cpu(), u0[i].cpu(), v0[i].cpu())
        r, k = wu.numel(), wv.numel()
        _close(su[ou:ou + r], wu, 1e-5)
        _close(sv[ov:ov + k], wv, 1e-5)
        assert abs(sigma[i].item() - ws.item()) <= 1e-5 * ws.item(), (i, sigma[i].item(), ws.item())
        assert torch.equal(c.weight_u, su[ou:ou + r]) and torch.equal(c.weight_v, sv[ov:ov + k])   # in place, the same bits
        assert (c.weight_u.data_ptr(), c.weight_v.data_ptr()) == ptrs[i]
        ou, ov = ou + r, ov + k
    assert ou == su.numel() and ov == sv.numel()
    # eval: sigma from the stored vectors, nothing written
    u1 = [c.weight_u.clone() for c in convs]
    v1 = [c.weight_v.clone() for c in convs]
    su2, sv2, sigma2 = hip.disc_sn_power(w, [c.weight_u for c in convs], [c.weight_v for c in convs], False)
    for i, c in enumerate(convs):
        assert torch.equal(c.weight_u, u1[i]) and torch.equal(c.weight_v, v1[i])
        m = w[i].cpu().double().reshape(w[i].shape[0], -1)
        want = torch.dot(u1[i].cpu().double(), m @ v1[i].cpu().double())
        assert abs(sigma2[i].item() - want.item()) <= 1e-5 * want.item()
    assert torch.equal(su2, torch.cat(u1)) and torch.equal(sv2, torch.cat(v1))


def test_spectral_norm_scale_and_backward():
    """W = W_orig / sigma, and dW_orig = G / sigma - (<G, W_orig> / sigma^2) u v^T against fp64 autograd with u, v held constant"""
    from mrefsr_amd import hip
    net = _net().to(DEV)
    convs = net.sn_convs()
    w = [c.weight_orig.detach() for c in convs]
    su, sv, sigma = hip.disc_sn_power(w, [c.weight_u for c in convs], [c.weight_v for c in convs], True)
    ws = hip.disc_sn_scale(w, sigma)
    g = torch.Generator().manual_seed(3)
    gs = [torch.randn(x.shape, generator=g) for x in w]
    dws = hip.disc_sn_bwd([t.to(DEV) for t in gs], w, su, sv, sigma)
    ou = ov = 0
    for i in range(8):
        r, k = w[i].shape[0], w[i][0].numel()
        u, v = su[ou:ou + r].cpu().double(), sv[ov:ov + k].cpu().double()
        ou, ov = ou + r, ov + k
        wo = w[i].cpu().double().requires_grad_(True)
        s = torch.dot(u, wo.reshape(r, -1) @ v)
        out = wo / s
        _close(ws[i], out)
        out.backward(gs[i].double())
        _close(dws[i], wo.grad)


def _up_cases():
    """(N, h, w, C, skip) of the three upsamplings of UNetDiscriminatorSN(3, 64) at each size"""
    out = []
    for n, hh, ww in SIZES:
        out += [(n, hh // 8, ww // 8, 512, False), (n, hh // 4, ww // 4, 256, True), (n, hh // 2, ww // 2, 128, True),
                (n, hh // 4, ww // 4, 256, False), (n, hh // 2, ww // 2, 128, False)]
    return out


@pytest.mark.parametrize('n,h,w,c,skip', _up_cases())
def test_upsample_adjoint_and_double_backward(n, h, w, c, skip):
    """up(y (+ skip)) against F.interpolate in fp64; the adjoint against its autograd; _UpAdj's backward (= _Up) likewise"""
    from mrefsr_amd import hip
    from mrefsr_amd.archs.nhwc_unetdisc import _Up
    g = torch.Generator().manual_seed(n * 100 + h + c)
    y = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    sk = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) if skip else None
    gout = torch.randn(n, c, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    yy = y.clone().requires_grad_(True)
    want = F.interpolate(yy + sk if skip else yy, scale_factor=2, mode='bilinear', align_corners=False)
    want.backward(gout)
    yd = _nhwc(y.float()).to(DEV).requires_grad_(True)
    skd = _nhwc(sk.float()).to(DEV).requires_grad_(True) if skip else None
    got = _Up.apply(yd, skd)
    _close(_nchw(got), want)
    _close(_nchw(hip.disc_up2_adj(_nhwc(gout.float()).to(DEV))), yy.grad)
    # d/d y through autograd (the adjoint node), then the adjoint node's own backward
    gy, = torch.autograd.grad(got, yd, _nhwc(gout.float()).to(DEV), create_graph=True)
    _close(_nchw(gy), yy.grad)
    if skip:
        gs, = torch.autograd.grad(got, skd, _nhwc(gout.float()).to(DEV))
        _close(_nchw(gs), yy.grad)
    r = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    go = _nhwc(gout.float()).to(DEV).requires_grad_(True)
    gy2, = torch.autograd.grad(_Up.apply(yd, skd), yd, go, create_graph=True)
    d_go, = torch.autograd.grad(gy2, go, _nhwc(r.float()).to(DEV))
    _close(_nchw(d_go), F.interpolate(r, scale_factor=2, mode='bilinear', align_corners=False))


def _conv9_cases():
    return [(n, hh, ww, 64) for n, hh, ww in SIZES] + [(1, 5, 7, 16), (2, 9, 3, 80)]


@pytest.mark.parametrize('n,h,w,c', _conv9_cases())
def test_conv9_forward_dgrad_wgrad_and_double_backward(n, h, w, c):
    """conv9 (C -> 1, 3x3, bias) forward, input gradient, weight and bias gradients against fp64; _Conv9Dgrad's backward (d gy, d w)"""
    from mrefsr_amd.archs.nhwc_unetdisc import _Conv9
    g = torch.Generator().manual_seed(n * 10 + h + c)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(1, c, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * c))**0.5
    b = torch.randn(1, generator=g, dtype=torch.float64)
    gout = torch.randn(n, 1, h, w, generator=g, dtype=torch.float64)
    r = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    xx, ww, bb = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    want = F.conv2d(xx, ww, bb, padding=1)
    gx64, gw64, gb64 = torch.autograd.grad(want, (xx, ww, bb), gout, create_graph=True)
    go64 = gout.clone().requires_grad_(True)
    gxx, = torch.autograd.grad(F.conv2d(xx, ww, bb, padding=1), xx, go64, create_graph=True)
    d_go64, d_w64 = torch.autograd.grad(gxx, (go64, ww), r)
    # (non-leaf inputs: torch cannot tell a backward run by autograd.grad whether it will use a leaf's gradient, nhwc_disc._wanted)
    xd = _nhwc(x.float()).to(DEV).requires_grad_(True).clone()
    wd = wt.float().to(DEV).requires_grad_(True).clone()
    bd = b.float().to(DEV).requires_grad_(True).clone()
    got = _Conv9.apply(xd, wd, bd)
    _close(_nchw(got), want)
    god = _nhwc(gout.float()).to(DEV).requires_grad_(True)
    gx, gw, gb = torch.autograd.grad(got, (xd, wd, bd), god, create_graph=True)
    _close(_nchw(gx), gx64)
    _close(gw, gw64)
    _close(gb, gb64)
    d_go, d_w = torch.autograd.grad(gx, (god, wd), _nhwc(r.float()).to(DEV))
    _close(_nchw(d_go), d_go64)
    _close(d_w, d_w64)


def _vconv_cases():
    """(N, ks, Cin, Cout, H, W) of conv1 .. conv8 of UNetDiscriminatorSN(3, 64) at each size"""
    out = []
    for n, h, w in SIZES:
        out += [(n, 4, 64, 128, h, w), (n, 4, 128, 256, h // 2, w // 2), (n, 4, 256, 512, h // 4, w // 4), (n, 3, 512, 256, h // 4, w // 4),
                (n, 3, 256, 128, h // 2, w // 2), (n, 3, 128, 64, h, w), (n, 3, 64, 64, h, w)]
    return out


@pytest.mark.parametrize('n,ks,cin,cout,h,w', _vconv_cases())
def test_sn_layer_convolutions(n, ks, cin, cout, h, w):
    """disc_vgg.hip's convolution (+ LeakyReLU) at the U-Net's layer shapes: forward, input gradient and weight gradient"""
    from mrefsr_amd.archs.nhwc_vggdisc import _VConv
    g = torch.Generator().manual_seed(n + ks + cin + h)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) * (2.0 / (cin * ks * ks))**0.5
    stride = 2 if ks == 4 else 1
    xd = _nhwc(x.float()).to(DEV).requires_grad_(True).clone()
    wd = wt.float().to(DEV).requires_grad_(True).clone()
    y = _VConv.apply(xd, wd, None, ks, True)
    mask = _nchw(y > 0).cpu()
    z64 = F.conv2d(x, wt, None, stride, 1)
    _close(_nchw(y), torch.where(mask, z64, 0.2 * z64))
    gout = torch.randn(z64.shape, generator=g, dtype=torch.float64)
    xx, ww = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    zz = F.conv2d(xx, ww, None, stride, 1)
    gx64, gw64 = torch.autograd.grad(torch.where(mask, zz, 0.2 * zz), (xx, ww), gout)
    gx, gw = torch.autograd.grad(y, (xd, wd), _nhwc(gout.float()).to(DEV))
    _close(_nchw(gx), gx64)
    _close(gw, gw64)
