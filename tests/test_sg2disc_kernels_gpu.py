"""GPU: the kernels of csrc/disc_sg2.hip (StyleGAN2Discriminator) against fp64 torch on the CPU.

Gate: max abs error <= 2e-5 * max |reference| for every output (the csrc/disc.hip and disc_vgg.hip gate).  The FIR is compared with
F.conv2d of the zero-padded map with the flipped outer-product kernel (what upfirdn2d computes), the convolutions behind it with
F.conv2d of that blurred map."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SLOPE = 0.2


def _close(got, want, rel=2e-5):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    assert err <= rel * scale + 1e-30, (err, scale)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).float().to(DEV).contiguous()


def _taps(k):
    k = torch.tensor(k, dtype=torch.float64)
    return k / k.sum()


def fir64(x, k, pad, down):
    """upfirdn2d(x, outer(k, k), down=down, pad=pad) in fp64 on [N,C,H,W]: pad with zeros, correlate with the flipped kernel, decimate"""
    c = x.shape[1]
    k2 = torch.outer(k, k).flip(0, 1)[None, None].repeat(c, 1, 1, 1)
    return F.conv2d(F.pad(x, (pad[0], pad[1], pad[0], pad[1])), k2, groups=c)[:, :, ::down, ::down]


def _pads(taps, ks):
    p = (len(taps) - 2) + (ks - 1)
    return ((p + 1) // 2, p // 2)


@pytest.mark.parametrize('k', [(1, 3, 3, 1), (1, 2, 1), (1, 1), (1, 2, 4, 3)])
@pytest.mark.parametrize('n,c,h,w,ks', [(2, 16, 8, 8, 3), (2, 16, 8, 8, 1), (1, 32, 64, 64, 3), (1, 32, 64, 64, 1), (2, 4, 11, 14, 3), (1, 8, 10, 6, 1)])
def test_fir_and_adjoint(k, n, c, h, w, ks):
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(h * 100 + c + ks + len(k))
    taps, down = _taps(k), (1 if ks == 3 else 2)
    pad = _pads(k, ks)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    y = fir64(x, taps, pad, down)
    if h % 2 == 0 and w % 2 == 0:
        assert y.shape[2:] == ((h + 1, w + 1) if ks == 3 else (h // 2, w // 2))   # what the stride-2 convolution behind it needs
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    got = hip.disc_sg2_fir(_nhwc(x.detach()), taps.tolist(), pad, down)
    _close(got, y.permute(0, 2, 3, 1))
    adj = hip.disc_sg2_fir(_nhwc(gy), taps.tolist(), pad, down, adjoint_shape=(n, h, w, c))
    _close(adj, x.grad.permute(0, 2, 3, 1))


def test_fir_matches_the_package_upfirdn2d():
    """the product's own basicsr.ops.upfirdn2d (csrc/upfirdn2d.hip) gives the same map"""
    from mrefsr_amd import hip
    from mrefsr_amd.archs.stylegan2_ops import make_resample_kernel
    from mrefsr_amd.ops.upfirdn2d import upfirdn2d
    x = torch.randn(2, 32, 16, 16, device=DEV)
    want = upfirdn2d(x, make_resample_kernel((1, 3, 3, 1)).to(DEV), pad=(2, 2))
    got = hip.disc_sg2_fir(x.permute(0, 2, 3, 1).contiguous(), _taps((1, 3, 3, 1)).tolist(), (2, 2), 1)
    _close(got, want.permute(0, 2, 3, 1), rel=1e-6)


# (n, cin, cout, h): the smallest map (8 -> 4), a 3 -> 4 padded input, split reductions (512 channels on 8 x 8), the largest map (128)
PAIR_CASES = [(2, 32, 48, 8), (4, 512, 512, 8), (4, 128, 256, 32), (3, 16, 16, 18), (2, 64, 64, 128)]


@pytest.mark.parametrize('ks', [3, 1])
@pytest.mark.parametrize('n,cin,cout,h', PAIR_CASES)
def test_fir_strided_conv_forward_dgrad_wgrad(n, cin, cout, h, ks):
    """FIR + 3x3 / stride 2 / pad 0 (+ bias + LeakyReLU) and FIR + 1x1 / stride 2 (+ residual): forward, input gradient and weight
    gradient against F.conv2d of the blurred input in fp64"""
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(cin * 1000 + cout + ks + h)
    taps = _taps((1, 3, 3, 1))
    pad = _pads(taps, ks)
    x = torch.randn(n, cin, h, h, generator=g, dtype=torch.float64)
    wt = (torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) / (ks * cin**0.5)).requires_grad_(True)
    b = torch.randn(cout, generator=g, dtype=torch.float64) if ks == 3 else None
    res = torch.randn(n, cout, h // 2, h // 2, generator=g, dtype=torch.float64) if ks == 1 else None
    xb = fir64(x, taps, pad, 1).requires_grad_(True)
    pre = F.conv2d(xb, wt, b, stride=2)
    assert pre.shape[2:] == (h // 2, h // 2)
    y = F.leaky_relu(pre, SLOPE) if ks == 3 else pre + res
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    pre.backward(dy)   # the gradient at the convolution's output (the mask is _LreluMask's business)
    # the device side: conv2 reads the stride-1 FIR output, the skip the stride-2 one with a stride-1 1x1 convolution
    xd = hip.disc_sg2_fir(_nhwc(x), taps.tolist(), pad, 1 if ks == 3 else 2)
    wd = wt.detach().float().to(DEV)
    got = hip.disc_sg2_conv(xd, hip.disc_sg2_pack_weight(wd, cin, False), None if b is None else b.float().to(DEV), ks,
                            SLOPE if ks == 3 else None, None if res is None else _nhwc(res))
    _close(got, y.permute(0, 2, 3, 1))
    dyd = _nhwc(dy)
    dx = hip.disc_sg2_conv_dgrad(dyd, hip.disc_sg2_pack_weight(wd, cin, True), tuple(xd.shape), ks)
    want_dx = xb.grad if ks == 3 else xb.grad[:, :, ::2, ::2]
    _close(dx, want_dx.permute(0, 2, 3, 1))   # (every element: torch.empty is not zeroed)
    dw = hip.disc_sg2_conv_wgrad(xd, dyd, cin, ks)
    _close(dw, wt.grad)
    assert torch.equal(dw, hip.disc_sg2_conv_wgrad(xd, dyd, cin, ks))
    assert torch.equal(dx, hip.disc_sg2_conv_dgrad(dyd, hip.disc_sg2_pack_weight(wd, cin, True), tuple(xd.shape), ks))


@pytest.mark.parametrize('n,cout,h', [(4, 64, 128), (2, 256, 32), (1, 16, 8)])
def test_input_stage(n, cout, h):
    """the 1x1 convolution from the packed RGB image (3 -> 4 channels) + bias + LeakyReLU, its input and weight gradients"""
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(cout + h)
    img = torch.rand(n, 3, h, h, generator=g, dtype=torch.float64).requires_grad_(True)
    wt = torch.randn(cout, 3, 1, 1, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    pre = F.conv2d(img, wt, b)
    dy = torch.randn(pre.shape, generator=g, dtype=torch.float64)
    pre.backward(dy)
    x4 = hip.disc_pack_image(img.detach().float().to(DEV))
    wd = wt.detach().float().to(DEV)
    got = hip.disc_sg2_conv(x4, hip.disc_sg2_pack_weight(wd, 4, False), b.float().to(DEV), 1, SLOPE)
    _close(got, F.leaky_relu(pre, SLOPE).permute(0, 2, 3, 1))
    dx = hip.disc_sg2_conv_dgrad(_nhwc(dy), hip.disc_sg2_pack_weight(wd, 4, True), tuple(x4.shape), 1)
    _close(dx[..., :3], img.grad.permute(0, 2, 3, 1))
    assert torch.count_nonzero(dx[..., 3]).item() == 0
    _close(hip.disc_sg2_conv_wgrad(x4, _nhwc(dy), 3, 1), wt.grad)


def test_final_conv_operand_513_channels():
    """final_conv's 513 inputs run on disc_vgg.hip's 3x3 convolution with the operand padded to 516 channels"""
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(513)
    x = torch.randn(4, 513, 4, 4, generator=g, dtype=torch.float64).requires_grad_(True)
    wt = (torch.randn(512, 513, 3, 3, generator=g, dtype=torch.float64) / 68).requires_grad_(True)
    b = torch.randn(512, generator=g, dtype=torch.float64)
    y = F.conv2d(x, wt, b, padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    xd = torch.zeros(4, 4, 4, 516, device=DEV)
    xd[..., :513] = _nhwc(x.detach())
    wd = wt.detach().float().to(DEV)
    _close(hip.disc_vconv(xd, hip.disc_vconv_pack_weight(wd, 516, False), b.float().to(DEV), 3), y.permute(0, 2, 3, 1))
    dx = hip.disc_vconv_dgrad(_nhwc(dy), hip.disc_vconv_pack_weight(wd, 516, True), tuple(xd.shape), 3)
    _close(dx[..., :513], x.grad.permute(0, 2, 3, 1))
    assert torch.count_nonzero(dx[..., 513:]).item() == 0
    _close(hip.disc_vconv_wgrad(xd, _nhwc(dy), 513, 3), wt.grad)


def test_refuses_unsupported_shapes():
    from mrefsr_amd import _lib, hip
    with pytest.raises(_lib.MrefsrHipError, match='Cout'):
        hip.disc_sg2_conv(torch.zeros(1, 9, 9, 16, device=DEV), torch.zeros(24, 9, 16, device=DEV), None, 3)
    with pytest.raises(_lib.MrefsrHipError, match='Cin'):
        hip.disc_sg2_conv(torch.zeros(1, 9, 9, 6, device=DEV), torch.zeros(16, 9, 6, device=DEV), None, 3)
    with pytest.raises(_lib.MrefsrHipError, match='kernel size'):
        hip.disc_sg2_conv(torch.zeros(1, 9, 9, 16, device=DEV), torch.zeros(16, 4, 16, device=DEV), None, 2)
    with pytest.raises(_lib.MrefsrHipError, match='taps'):
        hip.disc_sg2_fir(torch.zeros(1, 8, 8, 16, device=DEV), [0.2] * 5, (2, 2), 1)
    with pytest.raises(_lib.MrefsrHipError, match='multiple of 4'):
        hip.disc_sg2_fir(torch.zeros(1, 8, 8, 6, device=DEV), [0.5, 0.5], (1, 1), 1)
    with pytest.raises(NotImplementedError, match='CPU'):
        hip.disc_sg2_fir(torch.zeros(1, 8, 8, 16), [0.5, 0.5], (1, 1), 1)
