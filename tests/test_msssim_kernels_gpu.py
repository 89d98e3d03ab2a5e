"""GPU: the kernels of csrc/msssim.hip (through losses.MSSSIMLoss) against the float64 torch expression of the definition
(losses.msssim_loss_torch) evaluated on the CPU, in both channel modes.  Pattern, input generators and the factor 4 are those of
tests/test_ssim_loss_kernels_gpu.py.

Shapes (B, H, W; M levels): 22 x 22 with 2 (one map position at the last level); 23 x 45 with 2 (odd sides: a dropped row and
column); 54 x 91 with 3 (levels 54 x 91, 27 x 45, 13 x 22: odd at two levels, maps straddle the 16 x 32 tile); 63 x 107 with 3;
64 x 48 with 3 (the step test's GT); 160 x 160 with 4 (the shipped GT crop); 176 x 176 with 5 (the smallest five-level shape);
177 x 190 with 5 (last level 11 x 11).  Weights: the first M of the default five, used as given.

Error bar: not fixed in advance.  The yardstick is msssim_loss_torch in fp32 on the CPU against the same in float64 on the same
inputs; per input class ("generic": the smooth image plus 0.05 noise, and target uniform with pred = 0.5 target + 0.5 uniform;
"flat": a constant 0.5 target with 0.01 noise on pred, and a constant 0.98 with 1e-3 noise) the kernels' |loss - loss64| and
max |grad - grad64| / max |grad64| must stay within 4 x the largest value the yardstick reaches in that class over all shapes and
both modes (a wrong tap, halo, seam, pooling parity or level multiplier shows at 1e-2).  Condition, asserted on the float64
reference before anything is compared: every per-level mean F_{p,j} >= 0.05."""
import functools

import pytest
import torch

from test_msssim_cpu import anti_correlated, level_means
from test_ssim_loss_kernels_gpu import FACTOR, make_inputs, rel_grad_err

pytestmark = pytest.mark.gpu

DEFAULT = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SHAPES = (((1, 22, 22), 2), ((1, 23, 45), 2), ((2, 54, 91), 3), ((1, 63, 107), 3), ((2, 64, 48), 3), ((1, 160, 160), 4),
          ((1, 176, 176), 5), ((2, 177, 190), 5))
KINDS = {'generic': ('smooth', 'mixed'), 'flat': ('flat50', 'flat98')}
CHANNELS = ('y', 'rgb')


def inputs(kind, shape, seed):
    """(pred, target) fp32 on the CPU: the generators of the SSIM test; 'mixed': target uniform, pred = 0.5 target + 0.5 uniform"""
    if kind != 'mixed':
        return make_inputs(kind, shape, seed)
    other, target = make_inputs('uniform', shape, seed)
    return (0.5 * target + 0.5 * other).contiguous(), target


def expression(pred, target, channel, weights, dtype):
    """(loss, grad) of the torch expression in ``dtype`` on the CPU, as float64"""
    from mrefsr_amd.losses import msssim_loss_torch
    p = pred.detach().to(dtype, copy=True).requires_grad_(True)
    loss = msssim_loss_torch(p, target.to(dtype), channel, weights)
    loss.backward()
    return float(loss.detach()), p.grad.double()


@functools.lru_cache(maxsize=None)
def reference():
    """every case once: {(kind, channel, shape): (pred, target, weights, loss64, grad64, yardstick loss err, yardstick grad err)}
    and {class: (loss bar, gradient bar)} = FACTOR x the largest yardstick error of the class"""
    cases, bars = {}, {}
    for cls, kinds in KINDS.items():
        worst_l = worst_g = 0.0
        for kind in kinds:
            for ci, channel in enumerate(CHANNELS):
                for si, (shape, m) in enumerate(SHAPES):
                    weights = DEFAULT[:m]
                    pred, target = inputs(kind, shape, 1000 * ci + si)
                    fmin = float(level_means(pred.double(), target.double(), channel, weights).min())
                    assert fmin >= 0.05, (kind, channel, shape, fmin)
                    loss64, grad64 = expression(pred, target, channel, weights, torch.float64)
                    loss32, grad32 = expression(pred, target, channel, weights, torch.float32)
                    yl, yg = abs(loss32 - loss64), rel_grad_err(grad32, grad64)
                    cases[kind, channel, shape] = (pred, target, weights, loss64, grad64, yl, yg)
                    worst_l, worst_g = max(worst_l, yl), max(worst_g, yg)
        bars[cls] = (FACTOR * worst_l, FACTOR * worst_g)
    return cases, bars


def run_hip(pred, target, channel, weights, weight=1.0, upstream=None):
    from mrefsr_amd.losses import MSSSIMLoss
    p = pred.detach().float().cuda().requires_grad_(True)
    loss = MSSSIMLoss(loss_weight=weight, channel=channel, weights=weights)(p, target.float().cuda())
    (loss if upstream is None else upstream * loss).backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize('channel', CHANNELS)
@pytest.mark.parametrize('cls', list(KINDS))
def test_loss_and_gradient_within_the_fp32_yardstick(cls, channel):
    cases, bars = reference()
    loss_bar, grad_bar = bars[cls]
    print(f'class {cls}: loss bar {loss_bar:.2e}, gradient bar {grad_bar:.2e} ({FACTOR:g} x the fp32 torch expression)')
    bad = []
    for kind in KINDS[cls]:
        for shape, m in SHAPES:
            pred, target, weights, loss64, grad64, yl, yg = cases[kind, channel, shape]
            loss, grad = run_hip(pred, target, channel, weights)
            assert loss.dim() == 0 and loss.dtype == torch.float32 and grad.shape == pred.shape
            el, eg = abs(float(loss) - loss64), rel_grad_err(grad.cpu(), grad64)
            print(f'  {kind:8s} {channel:3s} {str(shape):14s} M={m} loss64 {loss64:.6e}  |loss err| hip {el:.2e} torch-fp32 {yl:.2e}   '
                  f'grad rel err hip {eg:.2e} torch-fp32 {yg:.2e}')
            if not (el <= loss_bar and eg <= grad_bar and bool(torch.isfinite(grad).all())):
                bad.append((kind, shape, el, eg))
    assert not bad, bad


@pytest.mark.parametrize('channel', CHANNELS)
def test_two_calls_give_identical_bits_and_inputs_are_not_written(channel):
    from mrefsr_amd.losses import MSSSIMLoss
    cases, _ = reference()
    for shape in ((2, 54, 91), (2, 177, 190)):
        pred, target, weights = cases['smooth', channel, shape][:3]
        pc, tc = pred.detach().cuda().requires_grad_(True), target.cuda()
        keep_p, keep_t = pc.detach().clone(), tc.clone()
        out = []
        for _ in range(2):
            pc.grad = None
            loss = MSSSIMLoss(channel=channel, weights=weights)(pc, tc)
            loss.backward()
            out.append((loss.detach().clone(), pc.grad.clone()))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        assert torch.equal(pc.detach(), keep_p) and torch.equal(tc, keep_t) and not tc.requires_grad


@pytest.mark.parametrize('channel', CHANNELS)
def test_upstream_gradient_and_loss_weight_scale_the_result(channel):
    """(3 loss).backward(): the last kernel reads the 3 from the device and multiplies its scale by it before the sum of the levels,
    torch multiplies afterwards: the two agree to 8 x 2^-24 per element.  loss_weight 0.25, a power of two, scales both exactly"""
    cases, _ = reference()
    pred, target, weights = cases['smooth', channel, (2, 54, 91)][:3]
    loss1, grad1 = run_hip(pred, target, channel, weights)
    loss3, grad3 = run_hip(pred, target, channel, weights, upstream=3.0)
    assert torch.equal(loss3, loss1)
    assert float(grad1.abs().max()) > 0 and torch.allclose(grad3, 3.0 * grad1, rtol=8 * 2.0 ** -24, atol=1e-30)
    lossw, gradw = run_hip(pred, target, channel, weights, weight=0.25)
    assert torch.equal(lossw, 0.25 * loss1) and torch.equal(gradw, 0.25 * grad1)


@pytest.mark.parametrize('shape,weights', [((2, 23, 45), (0.4, 0.6)), ((2, 54, 91), (0.3, 0.3, 0.4))])
def test_zero_rule_on_the_gpu(shape, weights):
    """pred = 1 - target: every plane's F_1 is negative (asserted in float64), so the loss is loss_weight exactly and the gradient
    is exactly zero, with nothing non-finite"""
    pred, target = anti_correlated(shape, 3)
    assert bool((level_means(pred, target, 'rgb', weights)[:, 0] < 0).all())
    loss, grad = run_hip(pred, target, 'rgb', weights, weight=0.7)
    assert float(loss) == float(torch.tensor(0.7)) and bool(torch.isfinite(grad).all()) and not bool(grad.any())


@pytest.mark.parametrize('channel', CHANNELS)
def test_mixed_batch_zero_for_the_anti_correlated_sample_half_for_the_other(channel):
    """sample 0 anti-correlated, sample 1 ordinary: sample 0's gradient is exactly zero, sample 1's is half of what it gets alone
    (the planes' sums do not depend on the batch; the scale 1 / planes halves exactly)"""
    weights = (0.4, 0.6)
    bad_p, bad_t = anti_correlated((1, 23, 45), 4)
    good_p, good_t = make_inputs('smooth', (1, 23, 45), 5)
    loss1, grad1 = run_hip(good_p, good_t, channel, weights)
    loss, grad = run_hip(torch.cat([bad_p.float(), good_p]), torch.cat([bad_t.float(), good_t]), channel, weights)
    assert bool(torch.isfinite(grad).all()) and not bool(grad[0].any()) and float(grad1.abs().max()) > 0
    assert torch.allclose(grad[1], 0.5 * grad1[0], rtol=8 * 2.0 ** -24, atol=1e-30)
    assert abs(float(loss) - (0.5 + 0.5 * float(loss1))) <= 2.0 ** -22


@pytest.mark.parametrize('channel', CHANNELS)
def test_a_samples_gradient_in_a_batch_of_two_is_half_of_its_gradient_alone(channel):
    cases, _ = reference()
    pred, target, weights = cases['smooth', channel, (2, 54, 91)][:3]
    _, grad = run_hip(pred, target, channel, weights)
    for i in range(2):
        _, alone = run_hip(pred[i:i + 1], target[i:i + 1], channel, weights)
        assert torch.allclose(grad[i], 0.5 * alone[0], rtol=8 * 2.0 ** -24, atol=1e-30)


@pytest.mark.parametrize('channel', CHANNELS)
def test_a_pred_without_grad_runs_the_forward_only(channel):
    from mrefsr_amd import hip
    from mrefsr_amd.losses import MSSSIMLoss
    cases, _ = reference()
    pred, target, weights = cases['mixed', channel, (2, 64, 48)][:3]
    with_grad, _ = run_hip(pred, target, channel, weights)
    loss = MSSSIMLoss(channel=channel, weights=weights)(pred.cuda(), target.cuda())
    assert not loss.requires_grad and loss.grad_fn is None and torch.equal(loss, with_grad)
    out, saved, values = hip.msssim_loss_fwd(pred.cuda(), target.cuda(), weights, rgb=channel == 'rgb', want_values=True)
    assert saved is None and torch.equal(out, with_grad) and values.dtype == torch.float64
    assert abs(float(1.0 - values.mean()) - float(out)) <= 2.0 ** -23
    with pytest.raises(NotImplementedError, match='fp32'):
        MSSSIMLoss(channel=channel, weights=weights)(pred.cuda().double(), target.cuda().double())
    with pytest.raises(ValueError, match='at most M = 3'):
        MSSSIMLoss(channel=channel, weights=DEFAULT[:4])(pred.cuda(), target.cuda())
