"""The reference side of the DCN edge tests (no GPU): what the hostile offset fields of tests/golden/dcn_edge_cases.py cover, and
the two oracles (oracle/mrefsr_oracle.c through oracle/c_api.py, oracle/dcn_torch.py) against closed forms, against each other and
against a hand evaluation of deform_conv_cuda_kernel.cu:526-568 -- on the window boundary, on integer positions, in the border bands
and outside.  tests/test_dcn_edges_gpu.py holds every DCN kernel to these oracles on the same fields."""
import functools

import numpy as np
import pytest
import torch

import dcn_edge_cases as E
from oracle import c_api as orc
from oracle import dcn_torch

CASES = E.cases()
# the oracles are one code path for every channel count: the wide geometries (whose fp64 autograd takes seconds) are left to the GPU tests
ORACLE_CASES = [(g, m) for g, m in CASES if E.GEOMETRIES[g][0] <= 64]
SHIFTS = ((-2, 3), (1, -1))


def _ids(cases):
    return [f'{g}-{m[0]}x{m[1]}x{m[2]}' for g, m in cases]


@pytest.mark.parametrize('geometry,bhw', CASES, ids=_ids(CASES))
def test_lattice_covers_every_pair_under_every_tap_group_and_ragged_tile(geometry, bhw):
    """conditions on the INPUTS of the GPU tests: every (y-class, x-class) pair of the 16 x 16 edge set under each of the 9 taps, in
    each deformable group, in the last (ragged) 64-pixel tile and in the last (ragged) 32-pixel tile (the backward's tile), and at
    least once with a nonzero mask; every target exactly representable and reached exactly by the fp32 sum base + tap + offset"""
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    _, h, w = bhw
    b = E.lattice_batch(geometry, bhw)
    f = E.field('lattice', b, dg, h, w, stride, pad, dil, with_mask)
    ho, wo = E.out_size(h, w, stride, pad, dil)
    assert f.offset.shape == (b, dg * 18, ho, wo) and f.offset.dtype == np.float32
    assert (f.mask is None) == (not with_mask)
    missing = E.missing_pairs(f)
    assert not missing, f'{geometry} {b}x{h}x{w}: pairs that never occur -- {missing[:3]}'
    if with_mask:
        m = np.unique(f.mask)
        assert 0.0 in m and 1.0 in m and ((m > 0) & (m < 1)).any()
    # exactness: targets are multiples of 1/8, and the sum the kernels form lands on them
    for t in (f.ty, f.tx):
        assert t.dtype == np.float32 and (t * 8 == np.round(t * 8)).all()
    py, px = E.positions_fp32(f, h, w, stride, pad, dil)
    assert py.dtype == np.float32 and (py == f.ty).all() and (px == f.tx).all()
    # each class index means the value it is named after, on this map
    for cls, t, length in ((f.cy, f.ty, h), (f.cx, f.tx, w)):
        assert (E.edge_values(length)[cls] == t).all()
        assert set(np.unique(cls).tolist()) == set(range(E.N_CLASSES))
    ev = E.edge_values(h)
    assert ev[1] == -1 and ev[14] == h and ev[5] == 0 and ev[10] == h - 1 and 0 <= ev[7] <= h - 1


@pytest.mark.parametrize('geometry,bhw', CASES, ids=_ids(CASES))
def test_position_exact_fields_land_where_they_say(geometry, bhw):
    """zero / shift / outside / mostly_outside: fp32 positions equal the targets; `outside` is at least 1.5 pixels beyond the map on
    some axis for EVERY sample, with both signs and magnitudes up to 1e4; `mostly_outside` puts exactly every 37th sample back"""
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    b, h, w = bhw
    for name, kw in (('zero', {}), ('shift', dict(shift=SHIFTS[0])), ('shift', dict(shift=SHIFTS[1])), ('outside', {}), ('mostly_outside', {})):
        f = E.field(name, b, dg, h, w, stride, pad, dil, with_mask, **kw)
        py, px = E.positions_fp32(f, h, w, stride, pad, dil)
        assert (py == f.ty).all() and (px == f.tx).all(), name
        far = (f.ty <= -1.5) | (f.ty >= h + 0.5) | (f.tx <= -1.5) | (f.tx >= w + 0.5)
        if name == 'outside':
            assert far.all()
            assert (f.ty < -1e3).any() and (f.ty > 1e3).any() and (f.tx < -1e3).any() and (f.tx > 1e3).any()
            assert np.abs(f.offset).max() <= 1.0e4 + max(h, w) + 4
        if name == 'mostly_outside':
            n = np.arange(far.size).reshape(far.shape)
            assert (far == (n % E.MOSTLY_OUTSIDE_EVERY != 0)).all()
            assert not E.outside_window(f.ty, f.tx, h, w)[~far].any()


@functools.lru_cache(maxsize=None)
def _inputs(geometry, b, h, w):
    return E.inputs(geometry, b, h, w)


def _t64(a):
    return torch.from_numpy(a).double()


@pytest.mark.parametrize('geometry,bhw', ORACLE_CASES, ids=_ids(ORACLE_CASES))
def test_oracle_forward_equals_the_closed_forms(geometry, bhw):
    """orc.dcnv2_fwd: zero offsets = the plain convolution, whole-pixel shifts = the convolution of the translated map (fp64 torch;
    integer positions sample exact values and the oracle accumulates in double, so the two differ by the final rounding to fp32: one
    ulp at a tie, 2.4e-7 relative, plus 1e-10 for sums that cancel); every sample outside or every mask 0 = the bias, exactly"""
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    b, h, w = bhw
    x, wgt, bias = _inputs(geometry, b, h, w)
    for shift in ((0, 0),) + SHIFTS:
        f = E.field('shift', b, dg, h, w, stride, pad, dil, with_mask, shift=shift)
        want = E.shifted_conv2d(_t64(x), _t64(wgt), _t64(bias), stride, pad, dil, groups, shift).numpy()
        got = orc.dcnv2_fwd(x, f.offset, f.mask, wgt, bias, stride, pad, dil, groups, dg)
        np.testing.assert_allclose(got, want, rtol=2.4e-7, atol=1e-10, err_msg=f'{geometry} {bhw} shift {shift}')
    f0 = E.field('zero', b, dg, h, w, stride, pad, dil, with_mask)
    assert not f0.offset.any()
    want0 = torch.nn.functional.conv2d(_t64(x), _t64(wgt), _t64(bias), stride, pad, dil, groups).numpy()
    np.testing.assert_allclose(orc.dcnv2_fwd(x, f0.offset, f0.mask, wgt, bias, stride, pad, dil, groups, dg), want0, rtol=2.4e-7, atol=1e-10)
    for name in ('outside', 'mask_zero'):
        if name == 'mask_zero' and not with_mask:
            continue
        f = E.field(name, b, dg, h, w, stride, pad, dil, with_mask)
        got = orc.dcnv2_fwd(x, f.offset, f.mask, wgt, bias, stride, pad, dil, groups, dg)
        assert (got == bias.reshape(1, -1, 1, 1)).all(), f'{geometry} {bhw} {name}: the oracle does not return the bias exactly'
        col = orc.dcnv2_im2col(x, f.offset, f.mask, 3, 3, stride, pad, dil, dg)
        assert not col.any(), f'{geometry} {bhw} {name}: nonzero columns'
        assert not orc.dcnv2_fwd(x, f.offset, f.mask, wgt, None, stride, pad, dil, groups, dg).any()


def _torch_backward(x, off, mask, wgt, gout, stride, pad, dil, groups, dg):
    xs = [None if a is None else _t64(a).requires_grad_(True) for a in (x, off, mask, wgt)]
    out = dcn_torch.modulated_deform_conv2d(xs[0], xs[1], xs[2], xs[3], None, stride, pad, dil, groups, dg)
    out.backward(_t64(gout))
    return [None if t is None else t.grad.numpy() for t in xs]


@pytest.mark.parametrize('geometry,bhw', ORACLE_CASES, ids=_ids(ORACLE_CASES))
def test_oracle_backward_c_and_torch_agree_on_the_lattice_and_are_zero_outside_the_window(geometry, bhw):
    """orc.dcnv2_bwd against the fp64 autograd of oracle/dcn_torch.py on the lattice field: every gradient, incl. grad_offset and
    grad_mask EXACTLY 0 where the target is -1 or below, or L or above, on either axis (deform_conv_cuda_kernel.cu:531-535, :747) --
    in both oracles.  The C oracle samples in fp32 as the reference does and accumulates in double: 1e-6 of the largest gradient
    (16 fp32 roundings' worth) + 1e-6 relative."""
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    _, h, w = bhw
    b = E.lattice_batch(geometry, bhw)
    x, wgt, _ = _inputs(geometry, b, h, w)
    f = E.field('lattice', b, dg, h, w, stride, pad, dil, with_mask)
    ho, wo = E.out_size(h, w, stride, pad, dil)
    gout = np.random.default_rng(5).standard_normal((b, co, ho, wo)).astype(np.float32)
    gx, goff, gm, gw, _ = orc.dcnv2_bwd(x, f.offset, f.mask, wgt, gout, stride, pad, dil, groups, dg)
    tx, toff, tm, tw = _torch_backward(x, f.offset, f.mask, wgt, gout, stride, pad, dil, groups, dg)
    out5 = E.outside_window(f.ty, f.tx, h, w)
    out_off = np.broadcast_to(out5[:, :, :, None], (b, dg, 9, 2, ho, wo)).reshape(goff.shape)
    assert out5.any() and (f.ty == -1).any() and (f.ty == h).any() and (f.tx == -1).any() and (f.tx == w).any()
    for who, go, gmk in (('mrefsr_oracle.c', goff, gm), ('dcn_torch.py', toff, tm)):
        assert not go[out_off].any(), f'{who}: nonzero grad_offset at a sample on or outside the window boundary'
        if with_mask:
            assert not gmk[out5.reshape(gmk.shape)].any(), f'{who}: nonzero grad_mask at a sample on or outside the window boundary'
    for name, got, want in (('grad_x', gx, tx), ('grad_offset', goff, toff), ('grad_mask', gm, tm), ('grad_weight', gw, tw)):
        if want is None:
            continue
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6 * float(np.abs(want).max()), err_msg=f'{geometry} {bhw} {name}')
    assert np.abs(toff).max() > 0 and np.abs(tx).max() > 0


def _coordinate_weight(im, y, x, bp_dir):
    """deform_conv_cuda_kernel.cu:526-568 (dmcn_get_coordinate_weight) in fp64, line for line: the derivative of the bilinear sample with
    respect to y (bp_dir 0) or x (bp_dir 1), one-sided at an integer position -- floor() takes the cell to the right / below"""
    height, width = im.shape
    if y <= -1 or y >= height or x <= -1 or x >= width:
        return 0.0
    y_low, x_low = int(np.floor(y)), int(np.floor(x))
    y_high, x_high = y_low + 1, x_low + 1
    weight = 0.0
    if bp_dir == 0:
        if y_low >= 0 and x_low >= 0:
            weight += -1 * (x_low + 1 - x) * im[y_low, x_low]
        if y_low >= 0 and x_high <= width - 1:
            weight += -1 * (x - x_low) * im[y_low, x_high]
        if y_high <= height - 1 and x_low >= 0:
            weight += (x_low + 1 - x) * im[y_high, x_low]
        if y_high <= height - 1 and x_high <= width - 1:
            weight += (x - x_low) * im[y_high, x_high]
    else:
        if y_low >= 0 and x_low >= 0:
            weight += -1 * (y_low + 1 - y) * im[y_low, x_low]
        if y_low >= 0 and x_high <= width - 1:
            weight += (y_low + 1 - y) * im[y_low, x_high]
        if y_high <= height - 1 and x_low >= 0:
            weight += -1 * (y - y_low) * im[y_high, x_low]
        if y_high <= height - 1 and x_high <= width - 1:
            weight += (y - y_low) * im[y_high, x_high]
    return weight


@pytest.mark.parametrize('bhw', E.GEOMETRY_MAPS['g8_dg4'], ids=lambda m: f'{m[0]}x{m[1]}x{m[2]}')
def test_offset_gradient_is_the_one_sided_form_of_the_reference_at_integer_positions(bhw):
    """grad_offset of both oracles on the lattice field against  sum_c grad_col[c] * mask * coordinate_weight(c)  with the hand-written
    fp64 coordinate weight above -- at every sample whose target is an integer on at least one axis (0, the interior integer, L-1,
    and -1 / L where the weight is 0), and at every other sample as well"""
    geometry = 'g8_dg4'
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    _, h, w = bhw
    b = E.lattice_batch(geometry, bhw)
    x, wgt, _ = _inputs(geometry, b, h, w)
    f = E.field('lattice', b, dg, h, w, stride, pad, dil, with_mask)
    ho, wo = E.out_size(h, w, stride, pad, dil)
    gout = np.random.default_rng(6).standard_normal((b, co, ho, wo)).astype(np.float32)
    gcol = np.einsum('ock,bop->bckp', wgt.reshape(co, c, 9).astype(np.float64), gout.reshape(b, co, ho * wo).astype(np.float64))
    ty, tx = f.ty.reshape(b, dg, 9, -1).astype(np.float64), f.tx.reshape(b, dg, 9, -1).astype(np.float64)
    mask = f.mask.reshape(b, dg, 9, -1).astype(np.float64)
    cpg = c // dg
    want = np.zeros((b, dg, 9, 2, ho * wo))
    xd = x.astype(np.float64)
    for bi in range(b):
        for g in range(dg):
            for t in range(9):
                for p in range(ho * wo):
                    for d in (0, 1):
                        want[bi, g, t, d, p] = sum(gcol[bi, g * cpg + cc, t, p] * mask[bi, g, t, p]
                                                   * _coordinate_weight(xd[bi, g * cpg + cc], ty[bi, g, t, p], tx[bi, g, t, p], d) for cc in range(cpg))
    integer = ((ty == np.floor(ty)) | (tx == np.floor(tx)))[:, :, :, None].repeat(2, 3)
    assert integer.mean() > 0.5 and np.abs(want[integer]).max() > 0
    _, goff, _, _, _ = orc.dcnv2_bwd(x, f.offset, f.mask, wgt, gout, stride, pad, dil, groups, dg)
    _, toff, _, _ = _torch_backward(x, f.offset, f.mask, wgt, gout, stride, pad, dil, groups, dg)
    scale = float(np.abs(want).max())
    for who, got, tol in (('mrefsr_oracle.c', goff, 1e-6), ('dcn_torch.py', toff, 1e-12)):
        got = got.reshape(want.shape)
        err = np.abs(got - want)
        assert err[integer].max() <= tol * scale, f'{who}: offset gradient at integer positions off by {err[integer].max():.3e} (scale {scale:.3e})'
        assert err.max() <= tol * scale, f'{who}: offset gradient off by {err.max():.3e}'
