"""GPU: the kernels of csrc/disc_vgg.hip (VGGStyleDiscriminator) against fp64 torch on the CPU.

Gate: max abs error <= 2e-5 * max |reference| for every output (the csrc/disc.hip gate).  Shapes: every convolution of
VGGStyleDiscriminator(3, 64) at 160 x 160 (B = 4), and at an odd 75 x 53 image (B = 2), where floor(H / 2), the parity phases of the
4x4 input gradient and its last row and column are exercised."""
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


def _layers(h, w, nf=64):
    """(ks, Cin, Cout, H, W) of every convolution of VGGStyleDiscriminator(3, nf) at an h x w image"""
    chans = [nf, nf, 2 * nf, 2 * nf, 4 * nf, 4 * nf, 8 * nf, 8 * nf, 8 * nf, 8 * nf]
    out, cin = [], 3
    for i, c in enumerate(chans):
        ks = 3 if i % 2 == 0 else 4
        out.append((ks, cin, c, h, w))
        if ks == 4:
            h, w = h // 2, w // 2
        cin = c
    return out


CASES = [(4, ) + l for l in _layers(160, 160)] + [(2, ) + l for l in _layers(75, 53)]


@pytest.mark.parametrize('n,ks,cin,cout,h,w', CASES)
def test_vconv_forward_dgrad_wgrad(n, ks, cin, cout, h, w):
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(cin * 1000 + cout + ks + h)
    stride = 2 if ks == 4 else 1
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) / (ks * cin**0.5)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    y = F.conv2d(x, wt, b, stride=stride, padding=1)
    assert y.shape[2:] == ((h // 2, w // 2) if ks == 4 else (h, w))
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    wr = wt.clone().requires_grad_(True)
    F.conv2d(xr, wr, None, stride=stride, padding=1).backward(dy)
    cp = 4 if cin == 3 else cin
    x4 = torch.zeros(n, h, w, cp, dtype=torch.float64)
    x4[..., :cin] = x.permute(0, 2, 3, 1)
    xd = x4.float().to(DEV).contiguous()
    wd = wt.float().to(DEV)
    got = hip.disc_vconv(xd, hip.disc_vconv_pack_weight(wd, cp, False), b.float().to(DEV), ks)
    _close(got, y.permute(0, 2, 3, 1))
    dyd = dy.permute(0, 2, 3, 1).float().to(DEV).contiguous()
    dx = hip.disc_vconv_dgrad(dyd, hip.disc_vconv_pack_weight(wd, cp, True), tuple(xd.shape), ks)
    _close(dx[..., :cin], xr.grad.permute(0, 2, 3, 1))   # (every element: torch.empty is not zeroed)
    if cp != cin:
        assert torch.count_nonzero(dx[..., cin:]).item() == 0
    dw = hip.disc_vconv_wgrad(xd, dyd, cin, ks)
    _close(dw, wr.grad)
    # two runs, the same bits
    assert torch.equal(dw, hip.disc_vconv_wgrad(xd, dyd, cin, ks))
    assert torch.equal(dx, hip.disc_vconv_dgrad(dyd, hip.disc_vconv_pack_weight(wd, cp, True), tuple(xd.shape), ks))


def test_vconv_refuses_unsupported_shapes():
    from mrefsr_amd import _lib, hip
    with pytest.raises(_lib.MrefsrHipError, match='Cout'):
        hip.disc_vconv(torch.zeros(1, 8, 8, 16, device=DEV), torch.zeros(24, 16, 16, device=DEV), None, 4)
    with pytest.raises(_lib.MrefsrHipError, match='Cin'):
        hip.disc_vconv(torch.zeros(1, 8, 8, 6, device=DEV), torch.zeros(16, 9, 6, device=DEV), None, 3)


def test_conv0_bias_lrelu_forward_backward_double_backward():
    """conv0_0: conv + bias + LeakyReLU(0.2) in the epilogue, its backward (the mask from the output's sign) and double backward
    (d / d gy: the same mask; d / d x: 0), through the autograd nodes, against fp64"""
    from mrefsr_amd.archs import nhwc_vggdisc as V
    g = torch.Generator().manual_seed(11)
    n, h, w, cout = 2, 40, 36, 64
    x = torch.randn(n, 3, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, 3, 3, 3, generator=g, dtype=torch.float64) * 0.3
    b = torch.randn(cout, generator=g, dtype=torch.float64) * 0.1
    gy = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    ggx = torch.randn(n, 3, h, w, generator=g, dtype=torch.float64)
    # the kernels (nodes): y, then dx / dw / db of <gy, y>, then the gradients of <ggx, dx> w.r.t. gy and w
    xd = x.float().to(DEV).requires_grad_(True)
    wd, bd = wt.float().to(DEV).requires_grad_(True), b.float().to(DEV).requires_grad_(True)
    gyd = gy.permute(0, 2, 3, 1).float().to(DEV).contiguous().requires_grad_(True)
    # (through a view: the nodes ask the engine whether a gradient is used, which autograd.grad cannot tell for its own leaf inputs)
    y = V._VConv.apply(V._Pack.apply(xd), wd.view_as(wd), bd.view_as(bd), 3, True)
    dx, dw, db = torch.autograd.grad(y, (xd, wd, bd), gyd, create_graph=True)
    d_gy, d_w = torch.autograd.grad((dx * ggx.float().to(DEV)).sum(), (gyd, wd))
    # fp64 with the kernels' mask (pre-activations within rounding of 0 would otherwise flip it)
    mask = (y.detach() > 0).permute(0, 3, 1, 2).cpu()
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    gyr = gy.clone().requires_grad_(True)
    z = F.conv2d(xr, wr, br, padding=1)
    yr = torch.where(mask, z, 0.2 * z)
    _close(y.permute(0, 3, 1, 2), yr)
    rdx, rdw, rdb = torch.autograd.grad(yr, (xr, wr, br), gyr, create_graph=True)
    for got, want in ((dx, rdx), (dw, rdw), (db, rdb)):
        _close(got, want)
    r_gy, r_w = torch.autograd.grad((rdx * ggx).sum(), (gyr, wr))
    _close(d_gy.permute(0, 3, 1, 2), r_gy)
    _close(d_w, r_w)
    # the mask kernel by itself
    from mrefsr_amd import hip
    t = torch.randn(3, 5, 7, 64, generator=g).to(DEV)
    yy = torch.randn(3, 5, 7, 64, generator=g).to(DEV)
    assert torch.equal(hip.disc_lrelu_mask(t, yy), torch.where(yy > 0, t, t * 0.2))


@pytest.mark.parametrize('n,h,w,c', [(4, 5, 5, 512), (2, 5, 5, 64), (3, 2, 3, 16)])
def test_linear_head_forward_backward_double_backward(n, h, w, c):
    """NCHW flatten -> linear1 -> LeakyReLU -> linear2 against F.linear in fp64 (the map's channels-last layout permuted by the kernel)"""
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(n + h + c)
    J = 100
    K = c * h * w
    f = torch.randn(n, h, w, c, generator=g, dtype=torch.float64)
    w1 = torch.randn(J, K, generator=g, dtype=torch.float64) / K**0.5
    b1 = torch.randn(J, generator=g, dtype=torch.float64) * 0.1
    w2 = torch.randn(1, J, generator=g, dtype=torch.float64) * 0.1
    b2 = torch.randn(1, generator=g, dtype=torch.float64) * 0.1
    gs = torch.randn(n, generator=g, dtype=torch.float64)
    ggf = torch.randn(f.shape, generator=g, dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in (f, w1, b1, w2, b2)]
    gsr = gs.clone().requires_grad_(True)
    hid = F.linear(leaves[0].permute(0, 3, 1, 2).reshape(n, -1), leaves[1], leaves[2])
    s = F.linear(F.leaky_relu(hid, 0.2), leaves[3], leaves[4]).view(-1)
    grads = torch.autograd.grad(s, leaves, gsr, create_graph=True)
    second = torch.autograd.grad((grads[0] * ggf).sum(), [gsr, leaves[1], leaves[3]])
    dv = [t.float().to(DEV).contiguous() for t in (f, w1, b1, w2.view(-1), b2)]
    out, hidden = hip.disc_linear_head(*dv)
    _close(hidden, hid)
    _close(out, s)
    gd = hip.disc_linear_head_bwd(gs.float().to(DEV), hidden, dv[0], dv[1], dv[3])
    for got, want in zip(gd, grads):
        _close(got, want.view(got.shape))
    dd = hip.disc_linear_head_dbl(ggf.float().to(DEV), gs.float().to(DEV), hidden, dv[1], dv[3])
    for got, want in zip(dd, second):
        _close(got, want.view(got.shape))
    with pytest.raises(RuntimeError, match='linear1 expects'):
        hip.disc_linear_head(dv[0][:, :, :-1].contiguous(), *dv[1:])
