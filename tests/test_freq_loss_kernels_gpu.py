"""GPU: the kernels of csrc/freq_loss.hip (through losses.FFTLoss and losses.FocalFrequencyLoss) against the torch definitions
(losses.fft_loss_torch, losses.focal_frequency_loss_torch) in float64 on the CPU.

Shapes (B, C, H, W): every pass works in TILE = 32 x 32 outputs per block -- rows of X / D, and columns that are the W/2 + 1
stored columns of D in the forward and the W columns of the gradient in the backward.  1 x 1, 1 x 7, 2 x 2, 8 x 8; 17 x 33 (prime
and odd sides, no Nyquist column); 31 x 32; B = 3 with differing images; 64 x 48, the GT of the step test; C = 1 and C = 4; and
extents of tile - 1, tile, tile + 1 and 2 tile + 1 in H, in W, and in W/2 + 1 (W = 61, 62, 65, 129), the other side small.

Error bar: not fixed in advance.  The yardstick is the same definition evaluated by torch in fp32 on the CPU as dense DFT matrix
products (twiddles of (j k) mod n built in float64 and rounded to fp32; X C_W and X S_W, then the column pass; full spectrum)
against float64.  Per input class ("generic": a smooth target plus 0.05 noise on pred, and independent uniform images; "near":
pred = target + 1e-3 noise) the kernels' |loss - loss64| / |loss64| and max |grad - grad64| / max |grad64| must stay within 4 x the
largest value the yardstick reaches in that class over all shapes and all four variants (an equally valid fp32 summation order; a
wrong twiddle, multiplicity, tile seam or transposed pass shows at 1e-2 and above).

sign() is discontinuous, so the inputs are chosen in float64 such that NO component of D is smaller than 1e-5 of the largest one
(except the imaginary parts of the self-conjugate bins, which are structurally zero and do not reach the gradient): the first such
seed of 32; the test fails if there is none."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = (32, 32)
_T = TILE[0]
_EDGES = (_T - 1, _T, _T + 1, 2 * _T + 1)
SHAPES = ([(1, 3, 1, 1), (1, 3, 1, 7), (1, 3, 2, 2), (1, 3, 8, 8), (1, 3, 17, 33), (2, 3, 31, 32), (3, 3, 27, 43), (2, 3, 64, 48),
           (1, 1, 5, 8), (1, 4, 5, 8)]
          + [(1, 3, m, 23) for m in _EDGES]                    # rows of X and D: 31, 32, 33, 65
          + [(1, 3, 21, m) for m in _EDGES]                    # columns of the gradient: 31, 32, 33, 65
          + [(1, 3, 9, 2 * m - 2 + (m & 1)) for m in _EDGES])  # W = 61, 62, 65, 129 -> stored columns of D: 31, 32, 33, 65
KINDS = {'generic': ('smooth', 'uniform'), 'near': ('near',)}
VARIANTS = ('fft-backward', 'fft-ortho', 'focal-1', 'focal-0.5')
FACTOR = 4.0
SEEDS = 32
AMBIGUOUS = 1e-5


def _raw_inputs(kind, shape, seed):
    g = torch.Generator().manual_seed(seed)
    b, c, h, w = shape
    if kind == 'smooth':
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
        ph = torch.rand(b, c, 1, 1, generator=g) * 6.28
        target = 0.5 + 0.2 * torch.sin(0.23 * yy + ph) + 0.2 * torch.cos(0.17 * xx - 0.11 * yy + 2 * ph)
        pred = target + 0.05 * torch.randn(b, c, h, w, generator=g)
    elif kind == 'uniform':
        target, pred = torch.rand(b, c, h, w, generator=g), torch.rand(b, c, h, w, generator=g)
    else:
        target = torch.rand(b, c, h, w, generator=g)
        pred = target + 1e-3 * torch.randn(b, c, h, w, generator=g)
    return pred.contiguous(), target.contiguous()


def ambiguous_components(pred, target):
    """how many components of D = fft2(pred - target) (float64) are below AMBIGUOUS x the largest, the structurally zero
    imaginary parts of the self-conjugate bins aside"""
    h, w = pred.shape[2:]
    d = torch.view_as_real(torch.fft.fft2(pred.double() - target.double()))
    ky, kx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    structural = ((2 * ky) % h == 0) & ((2 * kx) % w == 0)
    small = d.abs() < AMBIGUOUS * d.abs().max()
    small[..., 1] &= ~structural
    return int(small.sum())


def make_inputs(kind, shape, base):
    """(pred, target) fp32 on the CPU: the first of the seeds base ... base + SEEDS - 1 without an ambiguous component"""
    for seed in range(base, base + SEEDS):
        pred, target = _raw_inputs(kind, shape, seed)
        if ambiguous_components(pred, target) == 0:
            return pred, target
    raise AssertionError(f'{kind} {shape}: no seed of {base} ... {base + SEEDS - 1} is free of ambiguous components')


def _parse(variant):
    name, arg = variant.split('-')
    return name == 'focal', arg


def criterion(variant, weight=1.0):
    from mrefsr_amd.losses import FFTLoss, FocalFrequencyLoss
    focal, arg = _parse(variant)
    return FocalFrequencyLoss(loss_weight=weight, alpha=float(arg)) if focal else FFTLoss(loss_weight=weight, norm=arg)


def definition64(pred, target, variant):
    """(loss, grad) of the torch definition in float64 on the CPU"""
    p = pred.detach().double().requires_grad_(True)
    loss = criterion(variant)(p, target.double())
    loss.backward()
    return float(loss.detach()), p.grad


@functools.lru_cache(maxsize=None)
def _dft_matrices(n):
    r = (torch.arange(n).view(-1, 1) * torch.arange(n).view(1, -1)) % n          # exact integers
    ang = 2.0 * math.pi * r.double() / n
    return torch.cos(ang).float(), torch.sin(ang).float()


def dense_fp32(pred, target, variant):
    """the yardstick: (loss, grad as float64) of the same definition in fp32 on the CPU with the transform as dense matrix products"""
    focal, arg = _parse(variant)
    h, w = pred.shape[2:]
    (ch, sh), (cw, sw) = _dft_matrices(h), _dft_matrices(w)
    p = pred.detach().clone().requires_grad_(True)
    x = p - target
    tre, tim = x @ cw, -(x @ sw)
    dre, dim = ch @ tre + sh @ tim, ch @ tim - sh @ tre
    if focal or arg == 'ortho':
        s = 1.0 / math.sqrt(h * w)
        dre, dim = dre * s, dim * s
    if focal:
        m = dre ** 2 + dim ** 2
        wgt = torch.sqrt(m.detach()) ** float(arg)
        wgt = wgt / wgt.amax(dim=(2, 3), keepdim=True)
        wgt = torch.where(torch.isnan(wgt), torch.zeros_like(wgt), wgt).clamp(0.0, 1.0)
        loss = (wgt * m).mean()
    else:
        loss = (dre.abs() + dim.abs()).mean() / 2
    loss.backward()
    return float(loss.detach()), p.grad.double()


def rel_grad_err(grad, grad64):
    return float((grad.double() - grad64).abs().max() / grad64.abs().max())


@functools.lru_cache(maxsize=None)
def reference():
    """every case once: {(kind, variant, shape): (pred, target, loss64, grad64, yardstick loss err, yardstick grad err)} and
    {class: (relative loss bar, gradient bar)} = FACTOR x the largest yardstick error of the class"""
    cases, bars = {}, {}
    for cls, kinds in KINDS.items():
        worst_l = worst_g = 0.0
        for ki, kind in enumerate(kinds):
            for si, shape in enumerate(SHAPES):
                pred, target = make_inputs(kind, shape, 1000 * (ki + 1) + 40 * si)
                for variant in VARIANTS:
                    loss64, grad64 = definition64(pred, target, variant)
                    loss32, grad32 = dense_fp32(pred, target, variant)
                    yl, yg = abs(loss32 - loss64) / abs(loss64), rel_grad_err(grad32, grad64)
                    cases[kind, variant, shape] = (pred, target, loss64, grad64, yl, yg)
                    worst_l, worst_g = max(worst_l, yl), max(worst_g, yg)
        bars[cls] = (FACTOR * worst_l, FACTOR * worst_g)
    return cases, bars


def run_hip(pred, target, variant, weight=1.0, upstream=None):
    p = pred.detach().cuda().requires_grad_(True)
    loss = criterion(variant, weight)(p, target.cuda())
    (loss if upstream is None else upstream * loss).backward()
    return loss.detach(), p.grad


def test_tile_constants_are_the_ones_the_shapes_were_built_for():
    from mrefsr_amd import hip
    assert hip.FREQ_TILE == TILE and len(set(SHAPES)) == len(SHAPES)
    assert sorted(w // 2 + 1 for _, _, h, w in SHAPES if h == 9) == sorted(_EDGES)


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('cls', list(KINDS))
def test_loss_and_gradient_within_the_fp32_yardstick(cls, variant):
    cases, bars = reference()
    loss_bar, grad_bar = bars[cls]
    print(f'class {cls}: relative loss bar {loss_bar:.2e}, gradient bar {grad_bar:.2e} ({FACTOR:g} x the dense fp32 torch products)')
    bad = []
    for kind in KINDS[cls]:
        for shape in SHAPES:
            pred, target, loss64, grad64, yl, yg = cases[kind, variant, shape]
            loss, grad = run_hip(pred, target, variant)
            assert loss.dim() == 0 and loss.dtype == torch.float32 and grad.shape == pred.shape
            el, eg = abs(float(loss) - loss64) / abs(loss64), rel_grad_err(grad.cpu(), grad64)
            print(f'  {kind:8s} {variant:12s} {str(shape):16s} loss64 {loss64:.6e}  loss rel err hip {el:.2e} dense-fp32 {yl:.2e}   '
                  f'grad rel err hip {eg:.2e} dense-fp32 {yg:.2e}')
            if not (el <= loss_bar and eg <= grad_bar and bool(torch.isfinite(grad).all())):
                bad.append((kind, shape, el, eg))
    assert not bad, bad


@pytest.mark.parametrize('variant', VARIANTS)
def test_two_calls_give_identical_bits_and_inputs_are_not_written(variant):
    cases, _ = reference()
    for shape in ((3, 3, 27, 43), (2, 3, 64, 48), (1, 3, 9, 129)):
        pred, target = cases['smooth', variant, shape][:2]
        pc, tc = pred.detach().cuda().requires_grad_(True), target.cuda()
        keep_p, keep_t = pc.detach().clone(), tc.clone()
        out = []
        for _ in range(2):
            pc.grad = None
            loss = criterion(variant)(pc, tc)
            loss.backward()
            out.append((loss.detach().clone(), pc.grad.clone()))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        assert torch.equal(pc.detach(), keep_p) and torch.equal(tc, keep_t) and not tc.requires_grad


@pytest.mark.parametrize('variant', VARIANTS)
def test_upstream_gradient_and_loss_weight_scale_the_result(variant):
    """loss_weight 0.25 and an upstream factor -3: the loss is 0.25 x and the gradient -0.75 x the plain one, exactly -- the kernel
    multiplies loss_weight and the upstream value (read on the device) into one factor, -0.75 without rounding, and applies it
    last, one rounding of the exact product on either side"""
    cases, _ = reference()
    pred, target = cases['smooth', variant, (3, 3, 27, 43)][:2]
    loss1, grad1 = run_hip(pred, target, variant)
    lossw, gradw = run_hip(pred, target, variant, weight=0.25, upstream=-3.0)
    assert float(grad1.abs().max()) > 0
    assert torch.equal(lossw, 0.25 * loss1) and torch.equal(gradw, -0.75 * grad1)


@pytest.mark.parametrize('variant', VARIANTS)
def test_a_pred_without_grad_runs_the_forward_only(variant):
    from mrefsr_amd import hip
    focal, arg = _parse(variant)
    cases, _ = reference()
    pred, target = cases['uniform', variant, (2, 3, 64, 48)][:2]
    with_grad, _ = run_hip(pred, target, variant)
    loss = criterion(variant)(pred.cuda(), target.cuda())
    assert not loss.requires_grad and loss.grad_fn is None and torch.equal(loss, with_grad)
    kw = dict(focal=True, alpha=float(arg)) if focal else dict(norm=arg)
    out, g = hip.freq_loss_fwd(pred.cuda(), target.cuda(), **kw)
    assert g is None and torch.equal(out, with_grad)
    out, g = hip.freq_loss_fwd(pred.cuda(), target.cuda(), want_grad=True, **kw)
    assert g.shape == (6, 64, 25, 2) and torch.equal(out, with_grad)
    with pytest.raises(NotImplementedError, match='fp32'):
        criterion(variant)(pred.cuda().double(), target.cuda().double())


@pytest.mark.parametrize('variant', VARIANTS + ('focal-0',))
def test_equal_images_give_exactly_zero_loss_and_gradient(variant):
    """pred == target: X = 0 exactly, so every product is 0; the focal weight 0 / 0 counts as 0, sign(0) as 0"""
    cases, _ = reference()
    for shape in ((1, 3, 1, 1), (3, 3, 27, 43), (2, 3, 64, 48)):
        target = cases['smooth', 'fft-backward', shape][1]
        loss, grad = run_hip(target.clone(), target, variant)
        assert float(loss) == 0.0 and bool((grad == 0).all())


@pytest.mark.parametrize('variant', VARIANTS)
def test_the_planes_are_independent(variant):
    """a (3, 3, 27, 43) batch.  (a) with the other two images replaced, an image's gradient keeps its bits: no plane reads another
    one's coefficients, and the focal maximum is taken per plane.  (b) against a B = 1 call on the image alone: the mean runs over
    a third of the elements there, so the batch's gradient is that call's times 1/3 -- not in bits, as the map holds
    sign mult / count (2 w D mult / count) and the count enters every product of the adjoint transform differently rounded; both
    are valid fp32 evaluations of the same float64 gradient, so they differ by at most twice the class's bar"""
    cases, bars = reference()
    pred, target = cases['smooth', variant, (3, 3, 27, 43)][:2]
    other_p, other_t = cases['uniform', variant, (3, 3, 27, 43)][:2]
    _, grad = run_hip(pred, target, variant)
    for i in range(3):
        p2, t2 = other_p.clone(), other_t.clone()
        p2[i], t2[i] = pred[i], target[i]
        _, grad2 = run_hip(p2, t2, variant)
        assert torch.equal(grad2[i], grad[i])
        _, alone = run_hip(pred[i:i + 1], target[i:i + 1], variant)
        err = float((3.0 * grad[i].double() - alone[0].double()).abs().max() / alone.double().abs().max())
        print(f'  {variant:12s} image {i}: |3 grad[batch] - grad[alone]| / max = {err:.2e} (bar {2 * bars["generic"][1]:.2e})')
        assert err <= 2 * bars['generic'][1]


CHUNKED = (257, 1, 5, 8)


@functools.lru_cache(maxsize=None)
def chunked_reference():
    """the one case of CHUNKED, as reference() holds its cases: {variant: (loss64, grad64)}, the inputs, and the (relative loss bar,
    gradient bar) of the file's rule on this case -- FACTOR x the largest yardstick error over the four variants"""
    pred, target = make_inputs('smooth', CHUNKED, 9000)
    ref, worst_l, worst_g = {}, 0.0, 0.0
    for variant in VARIANTS:
        loss64, grad64 = definition64(pred, target, variant)
        loss32, grad32 = dense_fp32(pred, target, variant)
        ref[variant] = (loss64, grad64)
        worst_l, worst_g = max(worst_l, abs(loss32 - loss64) / abs(loss64)), max(worst_g, rel_grad_err(grad32, grad64))
    return pred, target, ref, (FACTOR * worst_l, FACTOR * worst_g)


@pytest.mark.parametrize('variant', VARIANTS)
def test_more_partials_than_one_chunk_of_the_last_blocks_sum(variant):
    """The block that draws the last ticket reads the blocks' partials 256 at a time (sum_partials_in_order, csrc/reduce.h); the
    shapes above stay within one chunk.  A plane is at least one block of the column pass and one of the focal finish, so 257
    planes are the fewest with which both launches have more than 256 blocks, and 257 is no multiple of 256: the loop's second
    pass runs, over one partial, behind its barrier.  The planes are the 5 x 8 of the C = 1 case above (a 1 x 1 plane has one real
    coefficient: |x| / count leaves the yardstick nothing to err on).  Kept out of reference(): the classes' bars come from the
    cases they always came from.  The bar is the file's rule on this one case: FACTOR x the largest error of the dense fp32 torch
    products on the same inputs over the four variants.  Two calls give the same bits"""
    from mrefsr_amd import _lib
    b, c, h, w = CHUNKED
    blocks = _lib.load().mrefsr_freq_loss_blocks(b * c, h, w)
    assert blocks == 257 and blocks > 256 and blocks % 256 != 0 and max(h, w) <= 64
    pred, target, ref, (loss_bar, grad_bar) = chunked_reference()
    loss64, grad64 = ref[variant]
    (loss, grad), (loss2, grad2) = run_hip(pred, target, variant), run_hip(pred, target, variant)
    el, eg = abs(float(loss) - loss64) / abs(loss64), rel_grad_err(grad.cpu(), grad64)
    print(f'  {variant:12s} {CHUNKED} {blocks} blocks  loss64 {loss64:.6e}  loss rel err hip {el:.2e} bar {loss_bar:.2e}   '
          f'grad rel err hip {eg:.2e} bar {grad_bar:.2e}')
    assert el <= loss_bar and eg <= grad_bar and bool(torch.isfinite(grad).all())
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
