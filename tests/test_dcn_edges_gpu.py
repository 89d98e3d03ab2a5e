"""Every DCN kernel path, forward and backward, on the hostile offset fields of tests/golden/dcn_edge_cases.py: samples exactly on
the window boundary (-1 and L), on integers, in the two border bands, far outside, and the closed forms (zero offsets = the plain
convolution, whole-pixel shifts = the convolution of the translated map, all outside / mask 0 = the bias).  The one bilinear
set-up of csrc/dcn_sample.h, as the kernels of csrc/dcn.hip, csrc/dcn_bwd.hip and csrc/dcn_any.hip use it, is held to one rule here:
deform_conv_cuda_kernel.cu:467-497, :526-568 as oracle/mrefsr_oracle.c and oracle/dcn_torch.py restate it
(tests/test_dcn_edges_cpu.py checks those two against closed forms, each other and a hand evaluation).

Bars are the ones the project already holds these kernels to: fp32-equivalent forward rtol = atol = 1e-4 (test_dcn_forward_vs_oracle),
col2im rtol = atol = 2e-4 (test_dcn_backward_pieces_vs_oracle), fused backward 2e-4 relative + 2e-4 x max |g| (test_dcn_fused_backward_vs_oracle),
f64 / f16 1e-11 / 3e-2 of the largest value, gradients four times that (test_dcn_other_dtypes_of_the_reference_dispatch), bf16
arithmetic one bf16 ulp + noise against the bf16 restatement (test_config4_every_dcn_and_attention_launch_within_one_bf16_ulp_of_the_restatement)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dcn_edge_cases as E
from oracle import c_api as orc
from oracle import dcn_torch

pytestmark = pytest.mark.gpu

SLOPE = 0.1
SLOPE32 = float(np.float32(SLOPE))     # the kernels take the slope as a C float
SHIFTS = ((-2, 3), (1, -1))
ORACLE_FIELDS = ('lattice', 'mostly_outside', 'heavy_tail')
CLOSED_FIELDS = ('zero', 'shift0', 'shift1')
BIAS_FIELDS = ('outside', 'mask_zero')
ALL_FIELDS = ORACLE_FIELDS + CLOSED_FIELDS + BIAS_FIELDS


@pytest.fixture(scope='module')
def hip():
    from mrefsr_amd import hip as h
    return h


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _nhwc(a):
    return dev(a).permute(0, 2, 3, 1).contiguous()


def _lrelu(a):
    """LeakyReLU as the epilogues form it, in a's own precision (numpy)"""
    return np.where(a > 0, a, a * a.dtype.type(SLOPE32))


def _ids(cases):
    return [f'{g}-{m[0]}x{m[1]}x{m[2]}' for g, m in cases]


def _batch(geometry, bhw, name):
    return E.lattice_batch(geometry, bhw) if name == 'lattice' else bhw[0]


@functools.lru_cache(maxsize=None)
def _field(geometry, bhw, name):
    """(Field, x, weight, bias) of one geometry / map / field name (shift0 / shift1: the two whole-pixel shifts); None where a field
    needs a mask and the geometry has none"""
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    _, h, w = bhw
    b = _batch(geometry, bhw, name)
    if name == 'mask_zero' and not with_mask:
        return None
    if name.startswith('shift'):
        f = E.field('shift', b, dg, h, w, stride, pad, dil, with_mask, shift=SHIFTS[int(name[5:])])
    else:
        f = E.field(name, b, dg, h, w, stride, pad, dil, with_mask)
    return (f,) + E.inputs(geometry, b, h, w)


def _shift_of(name):
    return (0, 0) if name == 'zero' else SHIFTS[int(name[5:])]


@functools.lru_cache(maxsize=None)
def _want_fwd(geometry, bhw, name):
    """the fp32 paths' reference output BEFORE the activation, with bias (computed once per geometry / map / field, read-only)"""
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    f, x, wgt, bias = _field(geometry, bhw, name)
    if name in CLOSED_FIELDS:
        t = lambda a: torch.from_numpy(a).double()      # noqa: E731
        out = E.shifted_conv2d(t(x), t(wgt), t(bias), stride, pad, dil, groups, _shift_of(name)).numpy()
    elif name in BIAS_FIELDS:
        ho, wo = f.offset.shape[2:]
        out = np.broadcast_to(bias.reshape(1, -1, 1, 1), (x.shape[0], co, ho, wo)).copy()
    else:
        out = orc.dcnv2_fwd(x, f.offset, f.mask, wgt, bias, stride, pad, dil, groups, dg)
    out.setflags(write=False)
    return out


def _blame_forward(run, geometry, bhw, rtol, atol):
    """which edge classes a forward path gets wrong on the lattice field: the field again with every sample pushed far outside
    (offset -1e4) except those of ONE class on one axis whose other axis is interior (k or k + 0.5), kernel against oracle"""
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    f, x, wgt, bias = _field(geometry, bhw, 'lattice')
    b, _, ho, wo = f.offset.shape
    bad = []
    for axis, cls, other in (('y', f.cy, f.cx), ('x', f.cx, f.cy)):
        for k in range(E.N_CLASSES):
            keep = (cls == k) & ((other == 7) | (other == 8))
            keep = np.broadcast_to(keep[:, :, :, None], (b, dg, 9, 2, ho, wo)).reshape(f.offset.shape)
            off = np.where(keep, f.offset, np.float32(-1.0e4)).astype(np.float32)
            want = _lrelu(orc.dcnv2_fwd(x, off, f.mask, wgt, bias, stride, pad, dil, groups, dg))
            got = run(x, off, f.mask, wgt, bias)
            if not np.allclose(got, want, rtol=rtol, atol=atol):
                bad.append(f'{axis} = {E.EDGE_NAMES[k]}')
    return ', '.join(bad) if bad else 'no single class alone (an interaction)'


# ------------------------------------------------------------------------------------------------ forward, fp32-equivalent paths
# (path, geometry, keyword arguments of hip.dcn_fwd, MREFSR_DCN_PT, MREFSR_DCN_T)
FWD_PATHS = [
    ('pt_cpg8_T2', 'c64', dict(channels_last=True), '1', '2'),                 # dcn_fwd_pt_kernel, paired 4-channel gather
    ('pt_cpg8_T4', 'c64', dict(channels_last=True), '1', '4'),
    ('pt_cpg16_NB2', 'c128', dict(channels_last=True), '1', '2'),
    ('pt_map8', 'c128_64', dict(channels_last=True), '1', '2'),                # 8-channel mapping
    ('one_tile_c256', 'c256', dict(channels_last=True), '1', '2'),             # dcn_fwd_bf16_kernel (Co = 256 stays on it)
    ('one_tile_c64', 'c64', dict(channels_last=True), '0', '2'),
    ('three_term_split', 'c64', dict(channels_last=True, range_free=True), '1', '2'),
    ('mfma_nchw_gather', 'c64_dg1_v1', dict(nhwc_gather=False), '1', '2'),     # dcn_fwd_mfma_kernel, DCNv1
    ('generic', 'g8_dg4', {}, '1', '2'),
    ('generic_groups2_stride2', 'g8_4_dg2_groups2_stride2', {}, '1', '2'),
    ('generic_dil2', 'g12_20_dg3_dil2', {}, '1', '2'),
]
FWD_CASES = [(p, m) for p in FWD_PATHS for m in E.GEOMETRY_MAPS[p[1]]]


def _runner(hip, monkeypatch, path, act_slope=SLOPE):
    name, geometry, kw, pt, t = path
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]

    def run(x, off, mask, wgt, bias):
        monkeypatch.setenv('MREFSR_DCN_PT', pt)
        monkeypatch.setenv('MREFSR_DCN_T', t)
        cl = kw.get('channels_last', False)
        out = hip.dcn_fwd(_nhwc(x) if cl else dev(x), dev(off), dev(mask), dev(wgt), dev(bias), stride, pad, dil, groups, dg, act_slope, **kw)
        return (out.permute(0, 3, 1, 2) if cl else out).cpu().numpy()
    return run


@pytest.mark.parametrize('path,bhw', FWD_CASES, ids=[f'{p[0]}-{m[0]}x{m[1]}x{m[2]}' for p, m in FWD_CASES])
def test_forward_paths_on_every_field(hip, monkeypatch, path, bhw):
    """one fp32-equivalent forward path on all fields, fused LeakyReLU(0.1): the bias BIT FOR BIT where every sample is outside or
    every mask is 0 (with and without a bias), the fp64 closed-form convolution on zero / whole-pixel offsets, the oracle on the
    lattice, mostly-outside and heavy-tailed fields; range flag clean"""
    pname, geometry = path[0], path[1]
    run = _runner(hip, monkeypatch, path)
    for name in ALL_FIELDS:
        fx = _field(geometry, bhw, name)
        if fx is None:
            continue
        f, x, wgt, bias = fx
        got = run(x, f.offset, f.mask, wgt, bias)
        want = _lrelu(_want_fwd(geometry, bhw, name))
        where = f'path {pname} ({geometry}, map {x.shape[0]}x{bhw[1]}x{bhw[2]}), field {f.name}'
        if name in BIAS_FIELDS:
            bad = got != want.astype(np.float32)
            assert not bad.any(), f'{where}: {int(bad.sum())} outputs are not lrelu(bias) bit for bit, worst |d| {np.abs(got - want).max():.3e}'
            got0 = run(x, f.offset, f.mask, wgt, None)
            assert not got0.any(), f'{where}, no bias: nonzero output {np.abs(got0).max():.3e} (columns / accumulators not exactly 0)'
            continue
        ok = np.isclose(got, want, rtol=1e-4, atol=1e-4)
        if not ok.all():
            err = np.abs(got - want)
            i = tuple(int(v) for v in np.unravel_index(np.argmax(err), err.shape))
            blame = _blame_forward(run, geometry, bhw, 1e-4, 1e-4) if name == 'lattice' else 'n/a'
            pytest.fail(f'{where}: {int((~ok).sum())} of {ok.size} outputs differ, worst {err[i]:.3e} at (b, o, ho, wo) = {i} '
                        f'(got {got[i]:.6g}, want {want[i]:.6g}); edge classes that fail on their own: {blame}')
    hip.check_conv_range()


TILE_CASES = [(g, m) for g in ('c64', 'c128', 'c128_64') for m in E.GEOMETRY_MAPS[g]]


@pytest.mark.parametrize('geometry,bhw', TILE_CASES, ids=_ids(TILE_CASES))
def test_tile_counts_return_the_same_bits_on_every_field(hip, monkeypatch, geometry, bhw):
    """T = 2, T = 4 (Co = 64) and the one-tile kernel: the SAME BITS on every field, with a mask and without one"""
    c, co, dg = E.GEOMETRIES[geometry][:3]
    for name in ALL_FIELDS:
        f, x, wgt, bias = _field(geometry, bhw, name)
        dx, doff, dw, db = _nhwc(x), dev(f.offset), dev(wgt), dev(bias)
        for mask in (dev(f.mask), None):
            monkeypatch.setenv('MREFSR_DCN_PT', '0')
            ref = hip.dcn_fwd(dx, doff, mask, dw, db, 1, 1, 1, 1, dg, SLOPE, channels_last=True)
            for t in ('2', '4'):
                monkeypatch.setenv('MREFSR_DCN_PT', '1')
                monkeypatch.setenv('MREFSR_DCN_T', t)
                got = hip.dcn_fwd(dx, doff, mask, dw, db, 1, 1, 1, 1, dg, SLOPE, channels_last=True)
                assert torch.equal(got, ref), (f'{geometry} map {tuple(x.shape)}, field {f.name}, mask {mask is not None}: T = {t} differs from '
                                               f'the one-tile kernel in {int((got != ref).sum())} outputs')
    hip.check_conv_range()


# ------------------------------------------------------------------------------------------------ forward, bf16 arithmetic
def _r16(t):
    return t.bfloat16().float()


BF16_CASES = [(g, m, io16) for g in ('c64', 'c256') for m in E.GEOMETRY_MAPS[g][:2] for io16 in (False, True)]


@pytest.mark.parametrize('geometry,bhw,io16', BF16_CASES, ids=[f'{g}-{m[0]}x{m[1]}x{m[2]}-{"bf16" if s else "fp32"}_storage' for g, m, s in BF16_CASES])
def test_bf16_arithmetic_on_every_field(hip, geometry, bhw, io16):
    """bf16_arith=True with fp32 and bf16 tensors: lrelu(bias) rounded to bf16, bit for bit, where nothing is sampled; elsewhere at
    most one bf16 ulp + the fp32 noise of the sum + two products' worth of a column rounding flip from the bf16 restatement (the
    oracle's im2col, columns and weights rounded to bf16, one fp32 GEMM, + bias, LeakyReLU, ONE rounding)"""
    c, co, dg = E.GEOMETRIES[geometry][:3]
    for name in ALL_FIELDS:
        f, x, wgt, bias = _field(geometry, bhw, name)
        xr = _r16(torch.from_numpy(x))                                            # bf16-valued input for both storages
        xin = xr.permute(0, 2, 3, 1).contiguous().cuda()
        y = hip.dcn_fwd(xin.bfloat16() if io16 else xin, dev(f.offset), dev(f.mask), dev(wgt), dev(bias), 1, 1, 1, 1, dg, SLOPE,
                        channels_last=True, bf16_arith=True)
        assert y.dtype == (torch.bfloat16 if io16 else torch.float32)
        got = y.float().permute(0, 3, 1, 2).cpu()
        where = f'bf16 arithmetic, {"bf16" if io16 else "fp32"} storage ({geometry}, map {tuple(x.shape)}), field {f.name}'
        assert torch.equal(got, _r16(got)), f'{where}: the launch returned values that are not bf16'
        if name in BIAS_FIELDS:
            want = _r16(torch.from_numpy(_lrelu(bias))).view(1, -1, 1, 1).expand_as(got)
            assert torch.equal(got, want), f'{where}: {int((got != want).sum())} outputs are not bf16(lrelu(bias)) bit for bit'
            continue
        col = torch.from_numpy(orc.dcnv2_im2col(xr.numpy(), f.offset, f.mask, 3, 3, 1, 1, 1, dg))
        w2 = _r16(torch.from_numpy(wgt)).flatten(1)
        tb = torch.from_numpy(bias)
        out = (torch.matmul(w2, _r16(col)) + tb.view(1, -1, 1)).view_as(got)
        mag = (torch.matmul(w2.abs(), _r16(col).abs()) + tb.abs().view(1, -1, 1)).view_as(got)
        flip = 2.0 * 2.0 ** -8 * (w2.abs().amax(1).view(1, -1, 1) * _r16(col).abs().amax(1, keepdim=True)).view_as(got)
        ref = _r16(F.leaky_relu(out, SLOPE))
        big = torch.maximum(got.abs(), ref.abs()).clamp_min(2.0 ** -126)
        ulp = torch.exp2(torch.floor(torch.log2(big)) - 7)
        excess = ((got - ref).abs() - ulp - 4e-6 * mag - flip).max().item()
        print(f'{where}: {int((got != ref).sum())} of {got.numel()} differ from the restatement, worst excess {excess:.2e}')
        assert excess <= 0, f'{where}: {excess:.3e} beyond one bf16 ulp + noise of the restatement'
    hip.check_conv_range()


# ------------------------------------------------------------------------------------------------ the other dtypes (dcn_any.hip)
def _torch_ref(x, off, mask, wgt, bias, geometry, gcol=None):
    """fp64 oracle/dcn_torch.py on the values the kernel sees -> (out before the activation, columns, (gx, goff, gmask) of the columns)"""
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    xs = [None if a is None else a.detach().double().cpu().clone().requires_grad_(gcol is not None) for a in (x, off, mask)]
    cols, ho, wo = dcn_torch.deform_columns(xs[0], xs[1], xs[2], 3, 3, stride, pad, dil, dg)
    grads = None
    if gcol is not None:
        cols.backward(gcol.double().cpu())
        grads = [None if t is None else t.grad for t in xs]
    with torch.no_grad():
        out = dcn_torch.modulated_deform_conv2d(xs[0], xs[1], xs[2], wgt.double().cpu(), None if bias is None else bias.double().cpu(),
                                                stride, pad, dil, groups, dg)
    return out, cols.detach(), grads


ANY_CASES = [(m, dt) for m in E.GEOMETRY_MAPS['g8_dg4'] for dt in (torch.float64, torch.float16)]


@pytest.mark.parametrize('bhw,dtype', ANY_CASES, ids=[f'{m[0]}x{m[1]}x{m[2]}-{str(d)[6:]}' for m, d in ANY_CASES])
def test_other_dtypes_forward_im2col_and_col2im_on_every_field(hip, bhw, dtype):
    """mrefsr_dcn_fwd / _im2col / _col2im (csrc/dcn_any.hip) in float64 and float16 against oracle/dcn_torch.py in fp64 on the
    values the kernel sees: 1e-11 / 3e-2 of the largest value, gradients four times that; the bias bit for bit and zero columns where
    nothing is sampled; grad_offset / grad_mask exactly 0 on and outside the window boundary"""
    geometry = 'g8_dg4'
    tol = 1e-11 if dtype == torch.float64 else 3e-2
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    _, h, w = bhw
    for name in ALL_FIELDS:
        f, x, wgt, bias = _field(geometry, bhw, name)
        dx, doff, dm, dw, db = (dev(a, dtype) for a in (x, f.offset, f.mask, wgt, bias))
        where = f'dcn_any {str(dtype)[6:]} (map {tuple(x.shape)}), field {f.name}'
        got = hip.dcn_fwd(dx, doff, dm, dw, db, stride, pad, dil, groups, dg, SLOPE)
        col = hip.dcn_im2col(dx, doff, dm, wgt.shape, stride, pad, dil, groups, dg)
        assert got.dtype == dtype and col.dtype == dtype
        if name in BIAS_FIELDS:
            acc = db.double() if dtype == torch.float64 else db.float()
            want = torch.where(acc > 0, acc, acc * SLOPE32).to(dtype).view(1, -1, 1, 1).expand_as(got)
            assert torch.equal(got, want), f'{where}: {int((got != want).sum())} outputs are not lrelu(bias) bit for bit'
            assert not col.any().item(), f'{where}: nonzero columns'
            continue
        out, cols, _ = _torch_ref(dx, doff, dm, dw, db, geometry)
        want = torch.where(out > 0, out, out * SLOPE32)
        err = (got.double().cpu() - want).abs().max().item()
        assert err <= tol * float(want.abs().max()), f'{where}: forward off by {err:.3e}'
        err = (col.double().cpu() - cols).abs().max().item()
        assert err <= tol * float(cols.abs().max()), f'{where}: im2col off by {err:.3e}'
    for name in ('lattice', 'outside', 'heavy_tail'):
        f, x, wgt, bias = _field(geometry, bhw, name)
        dx, doff, dm = (dev(a, dtype) for a in (x, f.offset, f.mask))
        where = f'dcn_any col2im {str(dtype)[6:]} (map {tuple(x.shape)}), field {f.name}'
        gcol = torch.randn(x.shape[0], c * 9, f.offset.shape[2] * f.offset.shape[3], generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dtype)
        gx, goff, gm = hip.dcn_col2im(gcol.cuda(), dx, doff, dm, wgt.shape, stride, pad, dil, groups, dg)
        _, _, (rx, roff, rm) = _torch_ref(dx, doff, dm, dev(wgt, dtype), None, geometry, gcol)
        if name == 'lattice':
            _assert_zero_outside_window(f, h, w, goff.cpu().numpy(), gm.cpu().numpy(), where)
        for gname, a, r in (('grad_x', gx, rx), ('grad_offset', goff, roff), ('grad_mask', gm, rm)):
            assert a.dtype == dtype
            err = (a.double().cpu() - r).abs().max().item()
            assert err <= 4 * tol * max(float(r.abs().max()), 1.0), f'{where}: {gname} off by {err:.3e}'
        if name == 'outside':
            assert not gx.any().item() and not goff.any().item() and not gm.any().item(), f'{where}: nonzero gradient with every sample outside'


# ------------------------------------------------------------------------------------------------ backward
def _assert_zero_outside_window(f, h, w, goff, gmask, where):
    """grad_offset (both components) and grad_mask exactly 0 at every lattice entry whose target is <= -1 or >= L on either axis; the
    message names the edge classes of the first offender"""
    b, dg, _, ho, wo = f.ty.shape
    out5 = E.outside_window(f.ty, f.tx, h, w)
    go = goff.reshape(b, dg, 9, 2, ho, wo)
    bad = out5[:, :, :, None] & (go != 0)
    if gmask is not None:
        bad = bad | (out5 & (gmask.reshape(b, dg, 9, ho, wo) != 0))[:, :, :, None]
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        j = i[:3] + i[4:]
        classes = sorted({(E.EDGE_NAMES[f.cy[k[:3] + k[4:]]], E.EDGE_NAMES[f.cx[k[:3] + k[4:]]]) for k in zip(*np.nonzero(bad))})
        pytest.fail(f'{where}: {int(bad.sum())} gradient entries are nonzero at samples on or outside the window boundary, first at '
                    f'(b, group, tap, y|x, ho, wo) = {i}: target (y {f.ty[j]}, x {f.tx[j]}), grad_offset {go[i]:.3e}; (y, x) edge classes hit: {classes[:8]}')


def _assert_grad(where, gname, got, want, rtol, atol, f=None):
    ok = np.isclose(got, want, rtol=rtol, atol=atol)
    if ok.all():
        return
    err = np.abs(got - want)
    i = tuple(int(v) for v in np.unravel_index(np.argmax(err), err.shape))
    extra = ''
    if f is not None and f.cy is not None and gname in ('grad_offset', 'grad_mask'):
        b, dg, _, ho, wo = f.cy.shape
        bad5 = (~ok).reshape((b, dg, 9, -1, ho, wo)).any(3)
        classes = sorted({(E.EDGE_NAMES[y], E.EDGE_NAMES[x]) for y, x in zip(f.cy[bad5].tolist(), f.cx[bad5].tolist())})
        extra = f'; (y, x) edge classes of the failing samples: {classes[:10]}{" ..." if len(classes) > 10 else ""}'
    pytest.fail(f'{where}: {gname} differs in {int((~ok).sum())} of {ok.size} entries, worst {err[i]:.3e} at {i} (got {got[i]:.6g}, want {want[i]:.6g}){extra}')


@functools.lru_cache(maxsize=None)
def _want_bwd(geometry, bhw, name, gscale):
    """(gout, (gx, goff, gmask, gw)) of the oracle -- of the fp64 autograd of the closed-form convolution on zero / shift fields (gx, gw)"""
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    f, x, wgt, bias = _field(geometry, bhw, name)
    ho, wo = f.offset.shape[2:]
    gout = (np.random.default_rng(11).standard_normal((x.shape[0], co, ho, wo)) * gscale).astype(np.float32)
    gx, goff, gm, gw, _ = orc.dcnv2_bwd(x, f.offset, f.mask, wgt, gout, stride, pad, dil, groups, dg)
    closed = None
    if name in CLOSED_FIELDS:
        xt, wt = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, wgt))
        E.shifted_conv2d(xt, wt, None, stride, pad, dil, groups, _shift_of(name)).backward(torch.from_numpy(gout).double())
        closed = (xt.grad.numpy(), wt.grad.numpy())
    return gout, (gx, goff, gm, gw), closed


COL2IM_CASES = [(g, m) for g in ('g8_dg4', 'g8_4_dg2_groups2_stride2', 'g12_20_dg3_dil2', 'c64') for m in E.GEOMETRY_MAPS[g]]
BWD_FIELDS = ('lattice', 'mostly_outside', 'heavy_tail', 'zero', 'shift0', 'shift1', 'outside')


@pytest.mark.parametrize('geometry,bhw', COL2IM_CASES, ids=_ids(COL2IM_CASES))
def test_col2im_on_every_field(hip, geometry, bhw):
    """hip.dcn_im2col / hip.dcn_col2im in fp32 (csrc/dcn_any.hip) around the two library GEMMs, against the oracle on every field; exactly 0
    on and outside the window boundary; everything exactly 0 when every sample is outside; grad_x / grad_weight of the closed-form
    convolution on zero / whole-pixel offsets"""
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    _, h, w = bhw
    cig, cog = c // groups, co // groups
    for name in BWD_FIELDS:
        f, x, wgt, bias = _field(geometry, bhw, name)
        gout, (gx, goff, gm, gw), closed = _want_bwd(geometry, bhw, name, 1.0)
        b, _, ho, wo = f.offset.shape
        where = f'col2im fp32 ({geometry}, map {tuple(x.shape)}), field {f.name}'
        dx, doff, dm, dw, dgo = dev(x), dev(f.offset), dev(f.mask), dev(wgt), dev(gout)
        col = hip.dcn_im2col(dx, doff, dm, wgt.shape, stride, pad, dil, groups, dg)
        go_g = dgo.view(b, groups, cog, ho * wo)
        gw_h = torch.einsum('bgop,bgkp->gok', go_g, col.view(b, groups, cig * 9, ho * wo)).reshape(co, cig, 3, 3).cpu().numpy()
        gcol = torch.einsum('gok,bgop->bgkp', dw.view(groups, cog, cig * 9), go_g).reshape(b, c * 9, ho * wo).contiguous()
        gx_h, goff_h, gm_h = hip.dcn_col2im(gcol, dx, doff, dm, wgt.shape, stride, pad, dil, groups, dg)
        gx_h, goff_h, gm_h = gx_h.cpu().numpy(), goff_h.cpu().numpy(), None if gm_h is None else gm_h.cpu().numpy()
        if name == 'outside':
            assert not col.any().item(), f'{where}: nonzero columns'
            for gname, a in (('grad_x', gx_h), ('grad_offset', goff_h), ('grad_mask', gm_h), ('grad_weight', gw_h)):
                assert a is None or not a.any(), f'{where}: {gname} is not exactly 0 (largest {np.abs(a).max():.3e})'
            continue
        if name == 'lattice':
            _assert_zero_outside_window(f, h, w, goff_h, gm_h, where)
        _assert_grad(where, 'grad_offset', goff_h, goff, 2e-4, 2e-4, f)
        if with_mask:
            _assert_grad(where, 'grad_mask', gm_h, gm, 2e-4, 2e-4, f)
        _assert_grad(where, 'grad_x', gx_h, gx, 2e-4, 2e-4)
        _assert_grad(where, 'grad_weight', gw_h, gw, 2e-4, 2e-4)
        if closed is not None:
            _assert_grad(where + ' (closed form)', 'grad_x', gx_h, closed[0], 2e-4, 2e-4)
            _assert_grad(where + ' (closed form)', 'grad_weight', gw_h, closed[1], 2e-4, 2e-4)
    f, x, wgt, bias = _field(geometry, bhw, 'mask_zero')
    col = hip.dcn_im2col(dev(x), dev(f.offset), dev(f.mask), wgt.shape, stride, pad, dil, groups, dg)
    assert not col.any().item(), f'im2col fp32 ({geometry}, map {tuple(x.shape)}), field mask_zero: nonzero columns'


FUSED_CASES = [(g, m) for g in ('c64', 'c128', 'c256', 'c64_dg2_v1') for m in E.GEOMETRY_MAPS[g]]
GSCALE = 1e-6     # the magnitude of an L1 loss's gradients, as in test_dcn_fused_backward_vs_oracle


@pytest.mark.parametrize('geometry,bhw', FUSED_CASES, ids=_ids(FUSED_CASES))
def test_fused_backward_on_every_field(hip, geometry, bhw):
    """hip.dcn_bwd_data / hip.dcn_bwd_weight (csrc/dcn_bwd.hip) at 8, 16 and 32 channels per deformable group, with a mask and without one,
    against the oracle on every field: 2e-4 relative + 2e-4 x max |g|; exactly 0 on and outside the window boundary; everything,
    grad_weight included, exactly 0 when every sample is outside; the closed-form convolution's grad_x / grad_weight"""
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    _, h, w = bhw
    for name in BWD_FIELDS:
        f, x, wgt, bias = _field(geometry, bhw, name)
        gout, (gx, goff, gm, gw), closed = _want_bwd(geometry, bhw, name, GSCALE)
        where = f'fused backward, {c // dg} channels per group ({geometry}, map {tuple(x.shape)}), field {f.name}'
        gmax = float(np.abs(gout).max())
        amax = dev(np.array([gmax], np.float32))
        dw = dev(wgt)
        ws = 2.0 ** (13 - int(np.floor(np.log2(np.abs(wgt).max()))))
        pk = hip.conv_pack_view(dw, None, 16, dgrad='T', wscale=ws)
        gx_h, goff_h, gm_h = hip.dcn_bwd_data(_nhwc(gout), _nhwc(x), dev(f.offset), dev(f.mask), pk, dg, g_amax=amax)
        gw_h = hip.dcn_bwd_weight(_nhwc(gout), _nhwc(x), dev(f.offset), dev(f.mask), co, dg, g_amax=amax).cpu().numpy()
        gx_h, goff_h, gm_h = gx_h.cpu().numpy(), goff_h.cpu().numpy(), None if gm_h is None else gm_h.cpu().numpy()
        if name == 'outside':
            for gname, a in (('grad_x', gx_h), ('grad_offset', goff_h), ('grad_mask', gm_h), ('grad_weight', gw_h)):
                assert a is None or not a.any(), f'{where}: {gname} is not exactly 0 (largest {np.abs(a).max():.3e})'
            continue
        if name == 'lattice':
            _assert_zero_outside_window(f, h, w, goff_h, gm_h, where)
        _assert_grad(where, 'grad_offset', goff_h, goff, 2e-4, 2e-4 * gmax, f)
        if with_mask:
            _assert_grad(where, 'grad_mask', gm_h, gm, 2e-4, 2e-4 * gmax, f)
        _assert_grad(where, 'grad_x', gx_h, gx, 2e-4, 2e-4 * gmax)
        _assert_grad(where, 'grad_weight', gw_h, gw, 2e-4, 2e-4 * float(np.abs(gw).max()))
        if closed is not None:
            _assert_grad(where + ' (closed form)', 'grad_x', gx_h, closed[0], 2e-4, 2e-4 * gmax)
            _assert_grad(where + ' (closed form)', 'grad_weight', gw_h, closed[1], 2e-4, 2e-4 * float(np.abs(closed[1]).max()))
    hip.check_conv_range()


@pytest.mark.parametrize('bhw', E.GEOMETRY_MAPS['c64'], ids=lambda m: f'{m[0]}x{m[1]}x{m[2]}')
def test_training_node_routes_the_same_fields_to_the_same_gradients(hip, bhw):
    """nhwc_train._Dcn at 64 -> 64 (channels-last forward, the routing of its backward) on the lattice, outside and shift fields:
    forward against the oracle, every gradient against the oracle at the fused kernels' bars, exactly 0 where they must be"""
    from mrefsr_amd.archs import nhwc_train
    geometry = 'c64'
    c, co, dg, groups, stride, pad, dil, with_mask = E.GEOMETRIES[geometry]
    _, h, w = bhw
    for name in ('lattice', 'outside', 'shift0'):
        f, x, wgt, bias = _field(geometry, bhw, name)
        gout, (gx, goff, gm, gw), closed = _want_bwd(geometry, bhw, name, GSCALE)
        gmax = float(np.abs(gout).max())
        where = f'nhwc_train._Dcn ({geometry}, map {tuple(x.shape)}), field {f.name}'
        xs = [t.requires_grad_(True) for t in (_nhwc(x), dev(f.offset), dev(f.mask), dev(wgt), dev(bias))]
        out = nhwc_train.dcn(xs[0], xs[1], xs[2], xs[3], xs[4], dg, 1.0)
        np.testing.assert_allclose(out.detach().permute(0, 3, 1, 2).cpu().numpy(), _want_fwd(geometry, bhw, name), rtol=1e-4, atol=1e-4,
                                   err_msg=where + ': forward')
        out.backward(_nhwc(gout))
        gx_h = xs[0].grad.permute(0, 3, 1, 2).cpu().numpy()
        goff_h, gm_h, gw_h = (t.grad.cpu().numpy() for t in xs[1:4])
        np.testing.assert_allclose(xs[4].grad.cpu().numpy(), gout.astype(np.float64).sum((0, 2, 3)), rtol=2e-4, atol=2e-4 * gmax, err_msg=where + ': grad_bias')
        if name == 'outside':
            for gname, a in (('grad_x', gx_h), ('grad_offset', goff_h), ('grad_mask', gm_h), ('grad_weight', gw_h)):
                assert not a.any(), f'{where}: {gname} is not exactly 0 (largest {np.abs(a).max():.3e})'
            continue
        if name == 'lattice':
            _assert_zero_outside_window(f, h, w, goff_h, gm_h, where)
        _assert_grad(where, 'grad_offset', goff_h, goff, 2e-4, 2e-4 * gmax, f)
        _assert_grad(where, 'grad_mask', gm_h, gm, 2e-4, 2e-4 * gmax, f)
        _assert_grad(where, 'grad_x', gx_h, gx, 2e-4, 2e-4 * gmax)
        _assert_grad(where, 'grad_weight', gw_h, gw, 2e-4, 2e-4 * float(np.abs(gw).max()))
    hip.check_conv_range()
