"""GPU: the kernels of csrc/disc.hip (ImageDiscriminator) against fp64 torch on the CPU.

Gate: max abs error <= 2e-5 * max |reference| for every output.  Shapes: every convolution of ImageDiscriminator(3, 32) at 160 x 160
(B = 4), and an odd 75 x 53 image, where the stride-2 parity phases and ceil(H / 2) are exercised."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _close(got, want, rel=2e-5):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    assert err <= rel * scale + 1e-30, (err, scale)


def _layers(h, w, ndf=32):
    """(Cin, Cout, stride, H, W) of every convolution of ImageDiscriminator(3, ndf) at an h x w image"""
    out, cin = [], 3
    for k in range(5):
        c = ndf * 2**k
        out.append((cin, c, 1, h, w))
        out.append((c, c, 2, h, w))
        h, w, cin = (h + 1) // 2, (w + 1) // 2, c
    return out


CASES = [(4, ) + l for l in _layers(160, 160)] + [(2, ) + l for l in _layers(75, 53)]


@pytest.mark.parametrize('n,cin,cout,stride,h,w', CASES)
def test_conv3x3_forward_dgrad_wgrad(n, cin, cout, stride, h, w):
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(cin * 1000 + cout + stride + h)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) / (3 * cin**0.5)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    y = F.conv2d(x, wt, b, stride=stride, padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    wr = wt.clone().requires_grad_(True)
    F.conv2d(xr, wr, None, stride=stride, padding=1).backward(dy)
    cp = 4 if cin == 3 else cin
    x4 = torch.zeros(n, h, w, cp, dtype=torch.float64)
    x4[..., :cin] = x.permute(0, 2, 3, 1)
    xd = x4.float().to(DEV).contiguous()
    wd = wt.float().to(DEV)
    got = hip.disc_conv3x3(xd, hip.disc_conv_pack_weight(wd, cp, False), b.float().to(DEV), stride)
    _close(got, y.permute(0, 2, 3, 1))
    dyd = dy.permute(0, 2, 3, 1).float().to(DEV).contiguous()
    dx = hip.disc_conv3x3_dgrad(dyd, hip.disc_conv_pack_weight(wd, cp, True), tuple(xd.shape), stride)
    _close(dx[..., :cin], xr.grad.permute(0, 2, 3, 1))
    if cp != cin:
        assert torch.count_nonzero(dx[..., cin:]).item() == 0
    dw = hip.disc_conv3x3_wgrad(xd, dyd, cin, stride)
    _close(dw, wr.grad)
    _close(hip.disc_bias_grad(dyd), dy.sum((0, 2, 3)))
    # two runs, the same bits
    assert torch.equal(dw, hip.disc_conv3x3_wgrad(xd, dyd, cin, stride))


def test_conv3x3_refuses_unsupported_shapes():
    from mrefsr_amd import _lib, hip
    x = torch.zeros(1, 8, 8, 8, device=DEV)
    with pytest.raises(_lib.MrefsrHipError, match='Cin'):
        hip.disc_conv3x3(x, torch.zeros(9, 8, 16, device=DEV), None, 2)
    with pytest.raises(_lib.MrefsrHipError, match='Cout'):
        hip.disc_conv3x3(torch.zeros(1, 8, 8, 16, device=DEV), torch.zeros(9, 16, 24, device=DEV), None, 1)
    with pytest.raises(_lib.MrefsrHipError, match='stride'):
        hip.disc_conv3x3(torch.zeros(1, 8, 8, 16, device=DEV), torch.zeros(9, 16, 16, device=DEV), None, 3)


def _bn_ref(x, gamma, beta, gy, a, b, c):
    """fp64 torch: BatchNorm2d (training) + LeakyReLU(0.2), its backward and double backward"""
    x = x.clone().requires_grad_(True)
    gamma = gamma.clone().requires_grad_(True)
    beta = beta.clone().requires_grad_(True)
    gy = gy.clone().requires_grad_(True)
    rm, rv = torch.zeros(x.shape[1], dtype=torch.float64), torch.ones(x.shape[1], dtype=torch.float64)
    y = F.leaky_relu(F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5), 0.2)
    gx, gg, gb = torch.autograd.grad(y, (x, gamma, beta), gy, create_graph=True)
    L = (a * gx).sum() + (b * gg).sum() + (c * gb).sum()
    dgy, dx, dgam = torch.autograd.grad(L, (gy, x, gamma))
    return y, rm, rv, gx, gg, gb, dgy, dx, dgam


@pytest.mark.parametrize('n,c,h,w', [(4, 32, 160, 160), (4, 64, 40, 40), (4, 512, 5, 5), (2, 256, 5, 4), (2, 16, 75, 53)])
def test_bn_lrelu_forward_backward_double_backward(n, c, h, w):
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 3 + 2
    gamma = 1 + 0.3 * torch.randn(c, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(c, generator=g, dtype=torch.float64)
    gy, a = torch.randn(x.shape, generator=g, dtype=torch.float64), torch.randn(x.shape, generator=g, dtype=torch.float64)
    b, cc = torch.randn(c, generator=g, dtype=torch.float64), torch.randn(c, generator=g, dtype=torch.float64)
    y, rm, rv, gx, gg, gb, dgy, dx, dgam = _bn_ref(x, gamma, beta, gy, a, b, cc)

    def d(t):
        return (t.permute(0, 2, 3, 1) if t.dim() == 4 else t).float().to(DEV).contiguous()

    def nhwc(t):
        return t.permute(0, 2, 3, 1)
    rmd, rvd = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    xd = d(x)
    yd, mean, invstd = hip.disc_bn_lrelu(xd, d(gamma), d(beta), rmd, rvd, nbt)
    _close(yd, nhwc(y))
    _close(rmd, rm, 1e-5)
    _close(rvd, rv, 1e-5)
    assert int(nbt) == 1
    gxd, ggd, gbd = hip.disc_bn_lrelu_bwd(d(gy), yd, xd, mean, invstd, d(gamma))
    _close(gxd, nhwc(gx))
    _close(ggd, gg)
    _close(gbd, gb)
    dgyd, dxd, dgd = hip.disc_bn_lrelu_dbl(d(a), d(b), d(cc), d(gy), yd, xd, mean, invstd, d(gamma))
    _close(dgyd, nhwc(dgy))
    _close(dxd, nhwc(dx), 5e-5 if h * w * n > 50000 else 2e-5)
    _close(dgd, dgam)


def _head_ref(f, w1, b1, w2, b2):
    p = f.mean((1, 2))
    return torch.sigmoid(F.leaky_relu(p @ w1.t() + b1, 0.2) @ w2 + b2)


@pytest.mark.parametrize('n,h,w', [(4, 5, 5), (2, 3, 2), (7, 1, 1)])
def test_head_forward_backward_double_backward(n, h, w):
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(n + h)
    C, J = 512, 1024
    f = torch.randn(n, h, w, C, generator=g, dtype=torch.float64)
    w1 = torch.randn(J, C, generator=g, dtype=torch.float64) * 0.05
    b1 = torch.randn(J, generator=g, dtype=torch.float64) * 0.1
    w2 = torch.randn(J, generator=g, dtype=torch.float64) * 0.05
    b2 = torch.randn(1, generator=g, dtype=torch.float64) * 0.1
    gs = torch.randn(n, generator=g, dtype=torch.float64)
    ggf = torch.randn(f.shape, generator=g, dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in (f, w1, b1, w2, b2)]
    gsr = gs.clone().requires_grad_(True)
    s = _head_ref(*leaves)
    grads = torch.autograd.grad(s, leaves, gsr, create_graph=True)
    second = torch.autograd.grad((grads[0] * ggf).sum(), [gsr] + leaves)
    dv = [t.float().to(DEV).contiguous() for t in (f, w1, b1, w2, b2)]
    out, pooled, hidden = hip.disc_head(*dv)
    _close(out, s)
    gd = hip.disc_head_bwd(gs.float().to(DEV), out, pooled, hidden, dv[1], dv[3], tuple(f.shape))
    for got, want in zip(gd, grads):
        _close(got, want)
    dd = hip.disc_head_dbl(ggf.float().to(DEV), gs.float().to(DEV), out, pooled, hidden, dv[1], dv[3])
    for got, want in zip(dd, second):
        _close(got, want)


def test_pack_and_unpack_image():
    from mrefsr_amd import hip
    img = torch.randn(3, 3, 75, 53)
    x4 = hip.disc_pack_image(img.to(DEV))
    want = torch.cat([img.permute(0, 2, 3, 1), torch.zeros(3, 75, 53, 1)], 3)
    assert torch.equal(x4.cpu(), want)
    g4 = torch.randn(3, 75, 53, 4)
    assert torch.equal(hip.disc_unpack_image(g4.to(DEV)).cpu(), g4[..., :3].permute(0, 3, 1, 2))
