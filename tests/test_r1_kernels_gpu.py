"""GPU: the kernels of csrc/gan_reg.hip -- the per-sample sum of squares of r1_penalty and its backward.

Forward tolerance: relative to the float64 sum of the same fp32 elements, ((L + 1) / 2 + 2) 2^-24 with L =
hip.r1_lane_squares(n) the squares one lane adds at that n; computed from n here, not chosen by trial."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = [(1, 1), (1, 3), (3, 255), (2, 1025), (4, 12288), (5, 49159)]
U = 2.0 ** -24


def _bound(n):
    from mrefsr_amd import hip
    return ((hip.r1_lane_squares(n) + 1) / 2 + 2) * U


def _rows(batch, n, offset, seed=0):
    """[batch, n] normal data on the GPU whose first row starts ``offset`` elements behind an allocation (0: at it; 1: 4-byte
    aligned only), and the allocation"""
    g = torch.Generator().manual_seed(1000 * batch + n + seed)
    data = torch.randn(batch, n, generator=g)
    buf = torch.zeros(batch * n + offset + 4, device=DEV)
    view = buf[offset:offset + batch * n].view(batch, n)
    view.copy_(data)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * offset
    return view, buf, data


@pytest.fixture(scope='module')
def cases():
    """every (shape, offset) case once: the rows, the float64 sums and two runs of the forward"""
    from mrefsr_amd import hip
    out = {}
    for batch, n in SHAPES:
        for offset in (0, 1):
            view, buf, data = _rows(batch, n, offset)
            out[batch, n, offset] = dict(g=view, buf=buf, want=data.double().pow(2).sum(1), got=hip.r1_sqnorm(view), again=hip.r1_sqnorm(view))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('batch,n', SHAPES)
def test_forward_vs_float64_and_its_bits(cases, batch, n, offset):
    c = cases[batch, n, offset]
    got, want = c['got'].cpu().double(), c['want']
    assert c['got'].shape == (batch, ) and c['got'].dtype == torch.float32
    err = float(((got - want).abs() / want).max())
    print(f'\n[r1_sqnorm {batch} x {n} offset {offset}] |rel err| / bound = {err / _bound(n):.3f} (bound {_bound(n):.3e})')
    assert err <= _bound(n), (err, _bound(n))
    assert torch.equal(c['got'], c['again'])   # the same bits from run to run


def test_special_values():
    from mrefsr_amd import hip
    for batch, n in SHAPES:
        for offset in (0, 1):
            view, _, _ = _rows(batch, n, offset)
            view.zero_()
            assert torch.equal(hip.r1_sqnorm(view), torch.zeros(batch, device=DEV))   # all-zero rows: exactly 0
    for n in (3, 1025, 49159):
        for offset in (0, 1):
            view, _, data = _rows(4, n, offset, seed=1)
            clean = hip.r1_sqnorm(view).cpu()
            view[1, n // 2] = float('inf')
            view[2, n - 1] = float('nan')
            view[3, 0] = 2e19   # finite, but its square overflows fp32
            out = hip.r1_sqnorm(view).cpu()
            assert out[0] == clean[0] and np.isfinite(float(out[0]))   # the other row keeps its bits
            assert out[1] == float('inf') and bool(torch.isnan(out[2])) and out[3] == float('inf'), (n, offset, out)


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('batch,n', SHAPES)
def test_backward_bits_and_guards(cases, batch, n, offset):
    """gg = fl32(fl32(2 gs) g): bit-equal to torch's fp32 expression, for g and gg at the same offset (16-byte path) and at different
    ones (4-byte path); the elements on both sides of gg keep their guard value"""
    from mrefsr_amd import hip
    g = cases[batch, n, offset]['g']
    gs = torch.randn(batch, generator=torch.Generator().manual_seed(n)).to(DEV)
    want = g * (2 * gs).view(batch, 1)
    assert torch.equal(hip.r1_sqnorm_bwd(g, gs), want)
    for out_offset in (offset, offset + 1, offset + 2):
        buf = torch.full((batch * n + out_offset + 5, ), -7.0, device=DEV)
        out = buf[out_offset:out_offset + batch * n].view(batch, n)
        assert hip.r1_sqnorm_bwd(g, gs, out=out) is out
        assert torch.equal(out, want), (batch, n, offset, out_offset)
        assert bool((buf[:out_offset] == -7.0).all()) and bool((buf[out_offset + batch * n:] == -7.0).all())
    special = g.clone()
    special[0, 0] = float('inf')
    gs0 = gs.clone()
    gs0[0] = 0.0
    got, want = hip.r1_sqnorm_bwd(special, gs0), special * (2 * gs0).view(batch, 1)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0))


@pytest.mark.parametrize('batch,n', [(3, 255), (4, 12288)])
def test_function_gradient_vs_torch(batch, n):
    """the autograd node of r1_penalty: its value within the forward bound of the torch expression's, its autograd.grad bit-equal to the
    torch expression's (2 / B exact for these B is not assumed: compared with the bound)"""
    from mrefsr_amd.losses.losses import _R1SqNorm
    x = torch.randn(batch, 3, n // 3, generator=torch.Generator().manual_seed(n)).to(DEV).requires_grad_(True)
    w = torch.rand(batch, generator=torch.Generator().manual_seed(batch)).to(DEV) + 0.5
    got = (_R1SqNorm.apply(x * 1.0) * w).sum()
    ggot, = torch.autograd.grad(got, x)
    x64 = x.detach().double().requires_grad_(True)
    want = (x64.pow(2).view(batch, -1).sum(1) * w.double()).sum()
    gwant, = torch.autograd.grad(want, x64)
    bound = _bound(n) + batch * U   # the weighted sum of B values adds its own fp32 roundings: a product and B - 1 additions
    assert abs(got.item() - want.item()) <= bound * abs(want.item())
    assert float(((ggot.double() - gwant).abs() / gwant.abs().clamp_min(1e-30)).max()) <= 2 * U   # one rounding per element (and w's)
    xt = x.detach().clone().requires_grad_(True)
    gt, = torch.autograd.grad(((xt * 1.0).pow(2).view(batch, -1).sum(1) * w).sum(), xt)
    assert torch.equal(ggot, gt)   # the bits of torch's own backward of the expression


def test_refusals():
    from mrefsr_amd import hip
    with pytest.raises(NotImplementedError, match='no CPU path'):
        hip.r1_sqnorm(torch.zeros(2, 8))
    with pytest.raises(TypeError):
        hip.r1_sqnorm(torch.zeros(2, 8, device=DEV, dtype=torch.float16))
    with pytest.raises(ValueError, match='contiguous'):
        hip.r1_sqnorm(torch.zeros(2, 8, device=DEV)[:, ::2])
    with pytest.raises(ValueError):
        hip.r1_sqnorm(torch.zeros(0, 8, device=DEV))
    with pytest.raises(ValueError, match='gs'):
        hip.r1_sqnorm_bwd(torch.zeros(2, 8, device=DEV), torch.zeros(3, device=DEV))
