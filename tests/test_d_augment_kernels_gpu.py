"""GPU: the kernels of csrc/disc_augment.hip (hip.disc_augment, hip.disc_augment_adj and the autograd pair of archs/d_augment.py)
against d_augment_torch in float64.

The bound of every comparison is counted from the source, not chosen by trial.  With A = max |in| + |db| over the
sample (max |g| for the adjoint), sigma = |s| + |1 - s|, U = sigma A and Mag = max(U, |c| U + |1 - c| A), no intermediate of a pixel
exceeds Mag and each fp32 rounding that feeds an output moves it by at most 2^-24 Mag: 16 roundings in the forward (three
brightness adds, two adds and the division of the channel mean, 1 - s, two products and the add of the saturation line, the
double -> fp32 of the sample mean and its brightness add, 1 - c, two products and the add of the contrast line), 13 in the adjoint."""
import pytest
import torch

from mrefsr_amd.archs import d_augment as da

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U24 = 2.0 ** -24
ROUNDINGS = dict(fwd=16, lin=16, adj=13)
SHAPES = [(1, 3, 8, 8), (2, 3, 11, 13), (5, 3, 37, 53)]


def _tables(b, rows):
    """rows: per-sample (db, s, c, flip, ty, tx, y0, y1, x0, x1), cycled over the batch"""
    rows = [rows[i % len(rows)] for i in range(b)]
    return da.AugmentParams.from_tables([list(r[:3]) for r in rows], [list(r[3:]) for r in rows])


def _cases(b, h, w):
    ident = (0.0, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 0)
    ry, rx = round(h / 8), round(w / 8)
    every = [(0.2, 2.0, 1.5, 1, ry, -rx, 0, h // 2, 0, w // 2), (-0.25, 0.0, 0.5, 0, -ry, rx, h // 3, h, w // 4, w),
             (0.1, 1.3, 0.7, 1, 1, 2, 2, h - 1, 1, w - 2), (-0.05, 0.4, 1.2, 1, -1, 0, 0, 0, 0, 0)]
    return {
        'identity': _tables(b, [ident]),
        'shift +-round(side / 8)': _tables(b, [(0.0, 1.0, 1.0, 0, ry, rx, 0, 0, 0, 0), (0.0, 1.0, 1.0, 0, -ry, -rx, 0, 0, 0, 0),
                                              (0.0, 1.0, 1.0, 1, ry, -rx, 0, 0, 0, 0)]),
        'shift of the full width': _tables(b, [(0.1, 1.0, 1.0, 0, 0, w, 0, 0, 0, 0), (0.1, 0.5, 1.5, 1, 0, -w, 0, 0, 0, 0)]),
        'box at two borders': _tables(b, [(0.0, 1.0, 1.0, 0, 0, 0, 0, h // 2, 0, w // 2), (0.0, 1.0, 1.0, 1, 0, 0, h // 2, h, w // 2, w)]),
        'box over the whole image': _tables(b, [(0.2, 0.5, 1.5, 0, 0, 0, 0, h, 0, w)]),
        'empty box': _tables(b, [(0.0, 1.0, 1.0, 0, 0, 0, 3, 3, 0, w), (0.0, 1.0, 1.0, 0, 0, 0, 0, h, 2, 2)]),
        'saturation 0 / 2': _tables(b, [(0.0, 0.0, 1.0, 0, 0, 0, 0, 0, 0, 0), (0.0, 2.0, 1.0, 1, 0, 0, 0, 0, 0, 0)]),
        'contrast 0.5 / 1.5': _tables(b, [(0.0, 1.0, 0.5, 0, 0, 0, 0, 0, 0, 0), (0.0, 1.0, 1.5, 1, 0, 0, 0, 0, 0, 0)]),
        'brightness and flip': _tables(b, [(0.25, 1.0, 1.0, 1, 0, 0, 0, 0, 0, 0), (-0.25, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 0)]),
        'mixed: sample 0 identity, the others everything': _tables(b, [ident] + every if b > 1 else every[:1]),
    }


def _mag(par, amax, bias):
    """[B] float64: the magnitude bound of each sample's intermediates from max |x|, db, s, c"""
    f = par.fpar.double().cpu()
    a = amax.double().cpu() + (f[:, 0].abs() if bias else 0.0)
    sigma = f[:, 1].abs() + (1 - f[:, 1]).abs()
    u = sigma * a
    return torch.maximum(u, f[:, 2].abs() * u + (1 - f[:, 2]).abs() * a)


def _amax(t):
    return t.detach().abs().reshape(t.shape[0], -1).max(1).values


def _ratio(got, want, bound):
    """max over the samples of max |got - want| / the sample's bound"""
    err = (got.detach().double().cpu() - want.detach().double().cpu()).abs().reshape(got.shape[0], -1).max(1).values
    return float((err / bound).max())


def _inputs(shape, seed=0):
    g = torch.Generator().manual_seed(seed + shape[0] * 1000 + shape[2])
    return torch.rand(shape, generator=g), torch.randn(shape, generator=g)


def _check(shape, name, par):
    from mrefsr_amd import hip
    x, g = _inputs(shape)
    pd = par.to(DEV)
    xd, gd = x.to(DEV), g.to(DEV)
    x64 = x.double().requires_grad_(True)
    want = da.d_augment_torch(x64, par)
    want_adj, = torch.autograd.grad(want, x64, g.double())
    want_lin = da.d_augment_torch(x.double(), par, bias=False)
    got, got_adj, got_lin = hip.disc_augment(xd, pd), hip.disc_augment_adj(gd, pd), hip.disc_augment(xd, pd, bias=False)
    r = dict(fwd=_ratio(got, want, ROUNDINGS['fwd'] * U24 * _mag(par, _amax(x), True)),
             adj=_ratio(got_adj, want_adj, ROUNDINGS['adj'] * U24 * _mag(par, _amax(g), False)),
             lin=_ratio(got_lin, want_lin, ROUNDINGS['lin'] * U24 * _mag(par, _amax(x), False)))
    print(f'[disc_augment {"x".join(map(str, shape))} {name}] err / bound: forward {r["fwd"]:.3f}  adjoint {r["adj"]:.3f}  '
          f'bias-free forward {r["lin"]:.3f}')
    assert max(r.values()) <= 1.0, (name, r)
    # the zeros are selected: exact, and the same pixels as the reference's
    assert torch.equal(got.cpu() == 0, want.detach() == 0)
    # the same bits from call to call
    assert torch.equal(hip.disc_augment(xd, pd), got) and torch.equal(hip.disc_augment_adj(gd, pd), got_adj)
    return got, got_adj, xd, gd


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_forward_adjoint_and_linear_part_vs_float64(shape):
    b, _, h, w = shape
    print()
    for name, par in _cases(b, h, w).items():
        got, got_adj, xd, gd = _check(shape, name, par)
        if name == 'identity':
            assert torch.equal(got, xd) and torch.equal(got_adj, gd) and not par.contrast
        if name in ('shift of the full width', 'box over the whole image'):
            assert float(got.abs().max()) == 0.0
            # nothing is kept: only the (1 - c) / N S_b term could be left, and S_b is a sum over no pixel
            assert float(got_adj.abs().max()) == 0.0


def test_flagship_shape_once():
    shape = (4, 3, 160, 160)
    print()
    _check(shape, 'mixed', _cases(4, 160, 160)['mixed: sample 0 identity, the others everything'])


def test_bound_catches_a_brightness_off_by_1e_5():
    """the bound means something: the float64 reference with every brightness offset moved by 1e-5 is outside it"""
    shape = (2, 3, 11, 13)
    x, _ = _inputs(shape)
    par = _cases(2, 11, 13)['mixed: sample 0 identity, the others everything']
    want = da.d_augment_torch(x.double(), par)
    bound = ROUNDINGS['fwd'] * U24 * _mag(par, _amax(x), True)
    wrong = da.AugmentParams.from_tables((par.fpar[:, :3] + torch.tensor([1e-5, 0.0, 0.0])).tolist(), par.ipar.tolist())
    assert _ratio(da.d_augment_torch(x.double(), wrong), want, bound) > 1.0


def test_nan_under_the_cut_box_and_in_the_margin():
    """zeros are written by selection: a NaN that only cut or shifted-out pixels would read does not reach the output.  The limit:
    contrast reads the whole sample's mean, so with c != 1 a NaN anywhere in the sample is in every kept pixel of that sample."""
    from mrefsr_amd import hip
    b, h, w = 2, 11, 13
    x, g = _inputs((b, 3, h, w))
    for c in (1.0, 1.5):
        par = _tables(b, [(0.1, 0.5, c, 1, 2, -3, 1, 6, 4, 9), (0.0, 2.0, c, 0, -1, 2, 0, 4, 0, w)])
        geometry = da.AugmentParams.from_tables([[0.0, 1.0, 1.0]] * b, par.ipar.tolist())   # the same flip, shift and box, no colour
        ones = torch.ones(b, 3, h, w, dtype=torch.float64, requires_grad=True)
        moved = da.d_augment_torch(ones, geometry)
        keep = moved.detach() != 0                                               # output pixels that are neither cut nor shifted in
        read = torch.autograd.grad(moved.sum(), ones)[0] != 0                    # source pixels that some output pixel reads
        assert 0 < int(keep.sum()) < keep.numel() and 0 < int(read.sum()) < read.numel()
        bad = torch.where(read, x, torch.full_like(x, float('nan')))             # NaN at every source pixel that no output reads
        clean, dirty = hip.disc_augment(x.to(DEV), par.to(DEV)).cpu(), hip.disc_augment(bad.to(DEV), par.to(DEV)).cpu()
        assert bool(torch.isfinite(clean).all()) and float(dirty[~keep].abs().max()) == 0.0
        if c == 1.0:
            assert torch.equal(dirty, clean)
        else:
            assert bool(torch.isnan(dirty[keep]).all())
        # the adjoint: a NaN of g at a cut or shifted-in output pixel is dropped, in the pixel term and in S_b alike
        gbad = torch.where(keep, g, torch.full_like(g, float('nan')))
        gc, gd = hip.disc_augment_adj(g.to(DEV), par.to(DEV)), hip.disc_augment_adj(gbad.to(DEV), par.to(DEV))
        assert bool(torch.isfinite(gc).all()) and torch.equal(gc, gd)


def test_double_backward_through_autograd():
    """f(x) = sum T(x)^3, gx = df/dx with create_graph, then d sum(gx^2) / dx: the only path through _AugmentAdj.backward.  Bound, to
    first order: with Lambda = max_b max(sigma, |c| sigma + |1 - c|) (the gain of L and of L^T in the max norm) and X = max |T(x)| <=
    Mag, |gx| <= 3 Lambda X^2 and the result <= 36 Lambda^3 X^3; the roundings on the way are 2 x 16 (T(x) enters squared) + 3 (the
    power's backward) + 13 (adjoint) for gx, then 16 (L on 2 gx, the 2 exact) + 16 + 3 (6 T(x) times it) + 13 (adjoint): 96 in all,
    each at most 2^-24 of the magnitude bound."""
    print()
    for shape in SHAPES[:2]:
        b, _, h, w = shape
        par = _cases(b, h, w)['mixed: sample 0 identity, the others everything']
        x, _ = _inputs(shape, seed=1)

        def lines(x, T):
            gx, = torch.autograd.grad((T(x) ** 3).sum(), x, create_graph=True)
            (gx ** 2).sum().backward()
            return gx.detach(), x.grad
        pd = par.to(DEV)
        gx, gxx = lines(x.to(DEV).requires_grad_(True), lambda t: da.d_augment(t, pd))
        wgx, wgxx = lines(x.double().requires_grad_(True), lambda t: da.d_augment_torch(t, par))
        f = par.fpar.double()
        sigma = f[:, 1].abs() + (1 - f[:, 1]).abs()
        lam = float(torch.maximum(sigma, f[:, 2].abs() * sigma + (1 - f[:, 2]).abs()).max())
        xmax = float(_mag(par, _amax(x), True).max())
        r1 = float((gx.double().cpu() - wgx).abs().max()) / (48 * U24 * 3 * lam * xmax ** 2)
        r2 = float((gxx.double().cpu() - wgxx).abs().max()) / (96 * U24 * 36 * lam ** 3 * xmax ** 3)
        print(f'[disc_augment double backward {"x".join(map(str, shape))}] err / bound: gx {r1:.3f}  d sum(gx^2) / dx {r2:.3f}')
        assert r1 <= 1.0 and r2 <= 1.0 and float(wgxx.abs().max()) > 0


def test_non_contiguous_inputs_and_refusals():
    from mrefsr_amd import hip
    par = _cases(2, 11, 13)['mixed: sample 0 identity, the others everything'].to(DEV)
    x = torch.rand(2, 3, 13, 11, device=DEV).transpose(2, 3)
    assert not x.is_contiguous() and torch.equal(da.d_augment(x, par), hip.disc_augment(x.contiguous(), par))
    with pytest.raises(NotImplementedError):
        da.d_augment(torch.rand(2, 3, 11, 13), par)
    with pytest.raises(NotImplementedError):
        hip.disc_augment(torch.rand(2, 4, 11, 13, device=DEV), par)
    with pytest.raises(ValueError):
        hip.disc_augment(torch.rand(3, 3, 11, 13, device=DEV), par)


def _launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()                       # (the scratch and the ticket word exist)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_launch_counts():
    from mrefsr_amd import hip
    x = torch.rand(5, 3, 37, 53, device=DEV)
    cases = _cases(5, 37, 53)
    full, plain = cases['mixed: sample 0 identity, the others everything'].to(DEV), cases['shift +-round(side / 8)'].to(DEV)
    assert full.contrast and not plain.contrast
    for fn, apply_kernel in ((hip.disc_augment, 'disc_augment_fwd_kernel'), (hip.disc_augment_adj, 'disc_augment_adj_kernel')):
        two, one = _launches(lambda: fn(x, full)), _launches(lambda: fn(x, plain))
        assert len(two) == 2 and 'disc_augment_sum_kernel' in two[0] and apply_kernel in two[1], two
        assert len(one) == 1 and apply_kernel in one[0], one
