"""GPU: the kernels of csrc/ssim_loss.hip (through losses.SSIMLoss) against the float64 torch expression of the definition
(losses.ssim_loss_torch) evaluated on the CPU, in both channel modes.

Shapes: a forward block owns TILE = 16 x 32 map positions (rows x columns) of the (H - 10) x (W - 10) map, a backward block 16 x 32
pixels.  11 x 11 (one map position); map extents of tile - 1, tile, tile + 1 and 2 tile + 1, rows and columns separately; 12 x 27;
B = 3 with differing images; 64 x 48, the GT size of the step test.

Error bar: not fixed in advance.  The yardstick is the same expression evaluated by torch in fp32 on the CPU, against float64, on
the same inputs; per input class ("generic": a smooth image plus 0.05 noise, and independent uniform noise; "flat": a constant 0.5
target with 0.01 noise on pred, and a constant 0.98 with 1e-3 noise) the kernels' max |grad - grad64| / max |grad64| and
|loss - loss64| must stay within 4 x the largest value the yardstick reaches in that class over all shapes and both modes (an
equally valid fp32 summation order; a wrong tap, halo or tile seam shows at 1e-2 and above)."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = (16, 32)
_TH, _TW = TILE
SHAPES = ([(1, 11, 11)]
          + [(1, m + 10, 23) for m in (_TH - 1, _TH, _TH + 1, 2 * _TH + 1)]      # map rows 15, 16, 17, 33
          + [(1, 21, m + 10) for m in (_TW - 1, _TW, _TW + 1, 2 * _TW + 1)]      # map columns 31, 32, 33, 65
          + [(1, 12, 27), (3, 27, 43), (2, 64, 48)])
KINDS = {'generic': ('smooth', 'uniform'), 'flat': ('flat50', 'flat98')}
CHANNELS = ('y', 'rgb')
FACTOR = 4.0


def make_inputs(kind, shape, seed):
    """(pred, target) fp32 on the CPU"""
    g = torch.Generator().manual_seed(seed)
    b, h, w = shape
    if kind == 'smooth':
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
        ph = torch.rand(b, 3, 1, 1, generator=g) * 6.28
        target = 0.5 + 0.2 * torch.sin(0.23 * yy + ph) + 0.2 * torch.cos(0.17 * xx - 0.11 * yy + 2 * ph)
        pred = target + 0.05 * torch.randn(b, 3, h, w, generator=g)
    elif kind == 'uniform':
        target, pred = torch.rand(b, 3, h, w, generator=g), torch.rand(b, 3, h, w, generator=g)
    else:
        level, noise = {'flat50': (0.5, 0.01), 'flat98': (0.98, 1e-3)}[kind]
        target = torch.full((b, 3, h, w), level)
        pred = target + noise * torch.randn(b, 3, h, w, generator=g)
    return pred.contiguous(), target.contiguous()


def expression(pred, target, channel, dtype):
    """(loss, grad) of the torch expression in ``dtype`` on the CPU, as float64"""
    from mrefsr_amd.losses import ssim_loss_torch
    p = pred.detach().to(dtype, copy=True).requires_grad_(True)
    loss = ssim_loss_torch(p, target.to(dtype), channel)
    loss.backward()
    return float(loss.detach()), p.grad.double()


def rel_grad_err(grad, grad64):
    return float((grad.double() - grad64).abs().max() / grad64.abs().max())


@functools.lru_cache(maxsize=None)
def reference():
    """every case once: {(kind, channel, shape): (pred, target, loss64, grad64, yardstick loss err, yardstick grad err)} and
    {class: (loss bar, gradient bar)} = FACTOR x the largest yardstick error of the class"""
    cases, bars = {}, {}
    for cls, kinds in KINDS.items():
        worst_l = worst_g = 0.0
        for kind in kinds:
            for ci, channel in enumerate(CHANNELS):
                for si, shape in enumerate(SHAPES):
                    pred, target = make_inputs(kind, shape, 1000 * ci + si)
                    loss64, grad64 = expression(pred, target, channel, torch.float64)
                    loss32, grad32 = expression(pred, target, channel, torch.float32)
                    yl, yg = abs(loss32 - loss64), rel_grad_err(grad32, grad64)
                    cases[kind, channel, shape] = (pred, target, loss64, grad64, yl, yg)
                    worst_l, worst_g = max(worst_l, yl), max(worst_g, yg)
        bars[cls] = (FACTOR * worst_l, FACTOR * worst_g)
    return cases, bars


def run_hip(pred, target, channel, weight=1.0, upstream=None):
    from mrefsr_amd.losses import SSIMLoss
    p = pred.detach().cuda().requires_grad_(True)
    loss = SSIMLoss(loss_weight=weight, channel=channel)(p, target.cuda())
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
        for shape in SHAPES:
            pred, target, loss64, grad64, yl, yg = cases[kind, channel, shape]
            loss, grad = run_hip(pred, target, channel)
            assert loss.dim() == 0 and loss.dtype == torch.float32 and grad.shape == pred.shape
            el, eg = abs(float(loss) - loss64), rel_grad_err(grad.cpu(), grad64)
            print(f'  {kind:8s} {channel:3s} {str(shape):12s} loss64 {loss64:.6e}  |loss err| hip {el:.2e} torch-fp32 {yl:.2e}   '
                  f'grad rel err hip {eg:.2e} torch-fp32 {yg:.2e}')
            if not (el <= loss_bar and eg <= grad_bar and bool(torch.isfinite(grad).all())):
                bad.append((kind, shape, el, eg))
    assert not bad, bad


@pytest.mark.parametrize('channel', CHANNELS)
def test_two_calls_give_identical_bits_and_inputs_are_not_written(channel):
    cases, _ = reference()
    for shape in ((3, 27, 43), (2, 64, 48)):
        pred, target = cases['smooth', channel, shape][:2]
        pc, tc = pred.detach().cuda().requires_grad_(True), target.cuda()
        keep_p, keep_t = pc.detach().clone(), tc.clone()
        out = []
        for _ in range(2):
            from mrefsr_amd.losses import SSIMLoss
            p = pc
            p.grad = None
            loss = SSIMLoss(channel=channel)(p, tc)
            loss.backward()
            out.append((loss.detach().clone(), p.grad.clone()))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        assert torch.equal(pc.detach(), keep_p) and torch.equal(tc, keep_t) and not tc.requires_grad


@pytest.mark.parametrize('channel', CHANNELS)
def test_upstream_gradient_and_loss_weight_scale_the_result(channel):
    """(3 loss).backward(): the kernel reads the 3 from the device and multiplies its scale by it before the coefficients, torch
    multiplies afterwards -- three roundings on either path (scale, coefficient sum, colour coefficient), so the two agree to
    8 x 2^-24 per element.  loss_weight 0.25, a power of two, scales both exactly"""
    cases, _ = reference()
    pred, target = cases['smooth', channel, (3, 27, 43)][:2]
    loss1, grad1 = run_hip(pred, target, channel)
    loss3, grad3 = run_hip(pred, target, channel, upstream=3.0)
    assert torch.equal(loss3, loss1)
    assert float(grad1.abs().max()) > 0 and torch.allclose(grad3, 3.0 * grad1, rtol=8 * 2.0 ** -24, atol=1e-30)
    lossw, gradw = run_hip(pred, target, channel, weight=0.25)
    assert torch.equal(lossw, 0.25 * loss1) and torch.equal(gradw, 0.25 * grad1)


@pytest.mark.parametrize('channel', CHANNELS)
def test_a_pred_without_grad_runs_the_forward_only(channel):
    from mrefsr_amd import hip
    from mrefsr_amd.losses import SSIMLoss
    cases, _ = reference()
    pred, target = cases['uniform', channel, (2, 64, 48)][:2]
    with_grad, _ = run_hip(pred, target, channel)
    loss = SSIMLoss(channel=channel)(pred.cuda(), target.cuda())
    assert not loss.requires_grad and loss.grad_fn is None and torch.equal(loss, with_grad)
    out, maps = hip.ssim_loss_fwd(pred.cuda(), target.cuda(), rgb=channel == 'rgb')
    assert maps is None and torch.equal(out, with_grad)
    with pytest.raises(NotImplementedError, match='fp32'):
        SSIMLoss(channel=channel)(pred.cuda().double(), target.cuda().double())


@pytest.mark.parametrize('channel', CHANNELS)
def test_equal_images_give_no_loss_and_a_gradient_at_rounding_level(channel):
    """pred == target: m = 1 everywhere, so |loss| stays within the generic loss bar.  The true gradient is 0; the kernel's is what
    the rounding of the terms that cancel leaves: 2 X (G^T b) against Y (G^T c), and the two halves of a, each at most
    T = 2 * 255 / C2 * k / count per element (k = the plane's largest coefficient, 128.553 or 255; 1 / B2 <= 1 / C2), each the end of
    a few dozen fp32 operations (22 filter taps): bound 64 x 2^-24 x T, some 1e-4 of the gradient 0.05 noise would give"""
    cases, bars = reference()
    for shape in ((1, 11, 11), (3, 27, 43), (2, 64, 48)):
        target = cases['smooth', channel, shape][1]
        loss, grad = run_hip(target.clone(), target, channel)
        b, h, w = shape
        count = (3 if channel == 'rgb' else 1) * b * (h - 10) * (w - 10)
        t = 2 * 255 / (0.03 * 255) ** 2 * (255.0 if channel == 'rgb' else 128.553) / count
        _, y32 = expression(target, target, channel, torch.float32)
        print(f'  equal images {channel:3s} {str(shape):12s} loss {float(loss):.2e} (bar {bars["generic"][0]:.2e})  max |grad| hip '
              f'{float(grad.abs().max()):.2e} torch-fp32 {float(y32.abs().max()):.2e} (bound {64 * 2.0 ** -24 * t:.2e})')
        assert abs(float(loss)) <= bars['generic'][0]
        assert float(grad.abs().max()) <= 64 * 2.0 ** -24 * t and math.isfinite(float(grad.abs().max()))


CHUNKED = (43, 43, 43)   # map 33 x 33: six tiles per plane


@pytest.mark.parametrize('channel', CHANNELS)
def test_more_partials_than_one_chunk_of_the_last_blocks_sum(channel):
    """The block that draws the last ticket reads the blocks' partials 256 at a time (sum_partials_in_order, csrc/reduce.h).  The
    shapes above stay within one chunk (48 blocks at most); this one has 258 blocks in y mode (one chunk and 2) and 774 in rgb
    (three chunks and 6), so the loop's later passes run, with the barrier in front of each overwrite of the chunk in LDS.  Kept
    out of reference(): the classes' bars come from the cases they always came from.  The bar here is the file's rule on this one
    case: FACTOR x the error of the fp32 torch expression on the same inputs.  Two calls give the same bits (the ticket is back
    at 0, no pass of the loop reads a chunk that is being replaced)"""
    from mrefsr_amd import _lib
    b, h, w = CHUNKED
    blocks = _lib.load().mrefsr_ssim_loss_blocks(b, h, w, int(channel == 'rgb'))
    assert blocks == {'y': 258, 'rgb': 774}[channel] and blocks > 256 and blocks % 256 != 0
    pred, target = make_inputs('smooth', CHUNKED, 5000 + CHANNELS.index(channel))
    loss64, grad64 = expression(pred, target, channel, torch.float64)
    loss32, grad32 = expression(pred, target, channel, torch.float32)
    loss_bar, grad_bar = FACTOR * abs(loss32 - loss64), FACTOR * rel_grad_err(grad32, grad64)
    (loss, grad), (loss2, grad2) = run_hip(pred, target, channel), run_hip(pred, target, channel)
    el, eg = abs(float(loss) - loss64), rel_grad_err(grad.cpu(), grad64)
    print(f'  {channel:3s} {CHUNKED} {blocks} blocks  loss64 {loss64:.6e}  |loss err| hip {el:.2e} bar {loss_bar:.2e}   '
          f'grad rel err hip {eg:.2e} bar {grad_bar:.2e}')
    assert el <= loss_bar and eg <= grad_bar and bool(torch.isfinite(grad).all())
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
