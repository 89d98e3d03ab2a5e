"""GPU: the kernels of csrc/ldl_loss.hip (through losses.LDLLoss) against the float64 torch expression of the definition
(losses.ldl_loss_torch, which tests/test_ldl_loss_cpu.py ties to the reference's own function) evaluated on the CPU.

Shapes: a block owns TILE = 16 x 32 pixels (rows x columns), forward and backward alike.  4 x 4, 5 x 6 and 6 x 5 (the reflections
from both ends land on the same pixels), 7 x 9; rows of tile - 1, tile, tile + 1 and 2 tile + 1 against 9 columns, columns alike
against 8 rows; B = 3 at 27 x 43 with per-sample noise scales 0.02, 0.1 and 0.3; 2 x 64 x 48, the GT size of the step test.

Inputs: the classes "generic" and "plateau" of tests/golden/ldl_cases.py, whose masks no rounding can flip (|r - r_e| >= 1e-3 or an
exact tie): no pixel is left out of any comparison, and the kernels' mask must be the float64 mask on every pixel.

Error bar: not fixed in advance.  The yardstick is the same expression evaluated by torch in fp32 on the CPU, against float64, on
the same fp32 inputs; per class the kernels' |loss - loss64| / loss64, max |grad - grad64| / max |grad64| and max |w - w64| /
max |w64| must stay within 4 x the largest value the yardstick reaches in that class over all shapes (an equally valid fp32
order of operations; a wrong tap, reflection multiplicity or tile seam shows at 1e-2 and above).  Both columns are printed."""
import functools
import os

import numpy as np
import pytest
import torch

import ldl_cases

pytestmark = pytest.mark.gpu

TILE = (16, 32)
_TH, _TW = TILE
SHAPES = ([(1, 4, 4), (1, 5, 6), (1, 6, 5), (1, 7, 9)]
          + [(1, m, 9) for m in (_TH - 1, _TH, _TH + 1, 2 * _TH + 1)]      # rows 15, 16, 17, 33
          + [(1, 8, m) for m in (_TW - 1, _TW, _TW + 1, 2 * _TW + 1)]      # columns 31, 32, 33, 65
          + [(3, 27, 43), (2, 64, 48)])
SCALES = {(3, 27, 43): [0.02, 0.1, 0.3]}
FACTOR = 4.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ldl.npz')


def expression(out, gt, ema, dtype):
    """(loss, grad, w) of the torch expression in ``dtype`` on the CPU, as float64"""
    from mrefsr_amd.losses import ldl_artifact_map_torch, ldl_loss_torch
    o = out.detach().to(dtype, copy=True).requires_grad_(True)
    loss = ldl_loss_torch(o, gt.to(dtype), ema.to(dtype))
    loss.backward()
    with torch.no_grad():
        w = ldl_artifact_map_torch(gt.to(dtype), out.to(dtype), ema.to(dtype))
    return float(loss.detach()), o.grad.double(), w.double()


def rel_err(x, x64):
    return float((x.double() - x64).abs().max() / x64.abs().max())


@functools.lru_cache(maxsize=None)
def reference():
    """every case once: {(class, shape): (out, gt, ema, loss64, grad64, w64, yardstick errors (loss, grad, w))} and
    {class: (loss bar, gradient bar, map bar)} = FACTOR x the largest yardstick error of the class"""
    cases, bars = {}, {}
    for ci, cls in enumerate(ldl_cases.CLASSES):
        worst = [0.0, 0.0, 0.0]
        for si, shape in enumerate(SHAPES):
            out, gt, ema = ldl_cases.make_inputs(cls, shape, 1000 * ci + si, scales=SCALES.get(shape))
            loss64, grad64, w64 = expression(out, gt, ema, torch.float64)
            loss32, grad32, w32 = expression(out, gt, ema, torch.float32)
            assert torch.equal(w32 == 0, w64 == 0), (cls, shape)          # the construction: fp32 and float64 agree on every mask bit
            y = (abs(loss32 - loss64) / loss64, rel_err(grad32, grad64), rel_err(w32, w64))
            cases[cls, shape] = (out, gt, ema, loss64, grad64, w64, y)
            worst = [max(a, b) for a, b in zip(worst, y)]
        bars[cls] = tuple(FACTOR * v for v in worst)
    return cases, bars


def run_hip(out, gt, ema, weight=1.0, upstream=None):
    from mrefsr_amd.losses import LDLLoss
    p = out.detach().cuda().requires_grad_(True)
    loss = LDLLoss(loss_weight=weight)(p, gt.cuda(), ema.cuda())
    (loss if upstream is None else upstream * loss).backward()
    return loss.detach(), p.grad


def hip_map(out, gt, ema):
    from mrefsr_amd.losses import LDLLoss
    return LDLLoss().artifact_map(out.cuda(), gt.cuda(), ema.cuda())


@pytest.mark.parametrize('cls', ldl_cases.CLASSES)
def test_loss_gradient_and_map_within_the_fp32_yardstick(cls):
    cases, bars = reference()
    loss_bar, grad_bar, map_bar = bars[cls]
    print(f'class {cls}: bars loss {loss_bar:.2e}, gradient {grad_bar:.2e}, map {map_bar:.2e} ({FACTOR:g} x the fp32 torch expression)')
    bad = []
    for shape in SHAPES:
        out, gt, ema, loss64, grad64, w64, (yl, yg, yw) = cases[cls, shape]
        loss, grad = run_hip(out, gt, ema)
        w = hip_map(out, gt, ema)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and grad.shape == out.shape and w.shape == w64.shape and not w.requires_grad
        el, eg, ew = abs(float(loss) - loss64) / loss64, rel_err(grad.cpu(), grad64), rel_err(w.cpu(), w64)
        mask_ok = torch.equal(w.cpu() == 0, w64 == 0)
        print(f'  {cls:8s} {str(shape):12s} loss64 {loss64:.6e}  loss rel err hip {el:.2e} torch-fp32 {yl:.2e}   grad hip {eg:.2e} '
              f'torch-fp32 {yg:.2e}   map hip {ew:.2e} torch-fp32 {yw:.2e}   masked {float((w64 == 0).double().mean()):.2f} mask equal {mask_ok}')
        if not (el <= loss_bar and eg <= grad_bar and ew <= map_bar and mask_ok and bool(torch.isfinite(grad).all())):
            bad.append((shape, el, eg, ew, mask_ok))
    assert not bad, bad


@pytest.mark.parametrize('cls', ldl_cases.CLASSES)
def test_map_against_the_reference_fixture(cls):
    """w, the loss and the gradient on the shapes of tests/golden/ldl.npz (the reference's own function in float64), same bars"""
    _, bars = reference()
    loss_bar, grad_bar, map_bar = bars[cls]
    z = np.load(GOLDEN)
    for shape in ldl_cases.GOLDEN_SHAPES:
        key = ldl_cases.golden_key(cls, shape)
        out, gt, ema = (torch.from_numpy(z[f'{key}_{n}']) for n in ('out', 'gt', 'ema'))
        w64, grad64, loss64 = torch.from_numpy(z[f'{key}_w']), torch.from_numpy(z[f'{key}_grad']), float(z[f'{key}_loss'])
        w = hip_map(out, gt, ema).cpu()
        loss, grad = run_hip(out, gt, ema, weight=float(z['loss_weight']))
        el, eg, ew = abs(float(loss) - loss64) / loss64, rel_err(grad.cpu(), grad64), rel_err(w, w64)
        print(f'  {key:22s} loss {el:.2e} (bar {loss_bar:.2e})  gradient {eg:.2e} (bar {grad_bar:.2e})  map {ew:.2e} (bar {map_bar:.2e})')
        assert torch.equal(w == 0, w64 == 0)
        assert el <= loss_bar and eg <= grad_bar and ew <= map_bar


def test_two_calls_give_identical_bits_and_inputs_are_not_written():
    from mrefsr_amd.losses import LDLLoss
    cases, _ = reference()
    for cls, shape in (('generic', (3, 27, 43)), ('plateau', (2, 64, 48))):
        out, gt, ema = cases[cls, shape][:3]
        pc, tc, ec = out.cuda().requires_grad_(True), gt.cuda().requires_grad_(True), ema.cuda().requires_grad_(True)
        keep = [t.detach().clone() for t in (pc, tc, ec)]
        runs = []
        for _ in range(2):
            pc.grad = None
            loss = LDLLoss()(pc, tc, ec)
            loss.backward()
            runs.append((loss.detach().clone(), pc.grad.clone(), LDLLoss().artifact_map(pc, tc, ec).clone()))
        assert all(torch.equal(a, b) for a, b in zip(*runs))
        assert all(torch.equal(t.detach(), k) for t, k in zip((pc, tc, ec), keep))
        assert tc.grad is None and ec.grad is None                     # target and pred_ema are constants


def test_upstream_gradient_and_loss_weight_scale_the_result():
    """(3 loss).backward(): the kernel reads the 3 from the device and multiplies its scale by it before the bracket, torch multiplies
    the finished gradient -- two roundings on either path (the scale, the product), so the two agree to 8 x 2^-24 per element.
    loss_weight 0.25, a power of two, scales loss and gradient exactly"""
    cases, _ = reference()
    out, gt, ema = cases['generic', (3, 27, 43)][:3]
    loss1, grad1 = run_hip(out, gt, ema)
    loss3, grad3 = run_hip(out, gt, ema, upstream=3.0)
    assert torch.equal(loss3, loss1)
    assert float(grad1.abs().max()) > 0 and torch.allclose(grad3, 3.0 * grad1, rtol=8 * 2.0 ** -24, atol=1e-30)
    lossw, gradw = run_hip(out, gt, ema, weight=0.25)
    assert torch.equal(lossw, 0.25 * loss1) and torch.equal(gradw, 0.25 * grad1)


def test_a_pred_without_grad_runs_the_forward_only():
    from mrefsr_amd import hip
    from mrefsr_amd.losses import LDLLoss
    cases, _ = reference()
    out, gt, ema = cases['generic', (2, 64, 48)][:3]
    with_grad, _ = run_hip(out, gt, ema)
    loss = LDLLoss()(out.cuda(), gt.cuda(), ema.cuda())
    assert not loss.requires_grad and loss.grad_fn is None and torch.equal(loss, with_grad)
    value, saved, w = hip.ldl_loss_fwd(out.cuda(), gt.cuda(), ema.cuda())
    assert saved is None and w is None and torch.equal(value, with_grad)
    with pytest.raises(NotImplementedError, match='fp32'):
        LDLLoss()(out.cuda().double(), gt.cuda().double(), ema.cuda().double())


def test_zero_variance_sample_in_a_batch_of_two():
    """out == gt in sample 0: no loss from it, a finite gradient that is exactly 0 there, a map of 0; sample 1 is what it is alone
    with loss_weight 1 / 2 -- the same kernel arithmetic on the same tiles, so bit for bit"""
    cases, bars = reference()
    out, gt, ema = (t.clone() for t in cases['generic', (2, 64, 48)][:3])
    out[0] = gt[0]
    loss, grad = run_hip(out, gt, ema)
    alone, grad_alone = run_hip(out[1:].contiguous(), gt[1:].contiguous(), ema[1:].contiguous(), weight=0.5)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and float(grad[0].abs().max()) == 0.0
    assert float(hip_map(out, gt, ema)[0].abs().max()) == 0.0
    assert float(loss) > 0 and torch.equal(loss, alone) and torch.equal(grad[1:], grad_alone)
    loss64, grad64, _ = expression(out, gt, ema, torch.float64)
    assert abs(float(loss) - loss64) / loss64 <= bars['generic'][0] and rel_err(grad.cpu(), grad64) <= bars['generic'][1]
