"""GPU: the kernels of csrc/contextual.hip (hip.contextual_fwd / hip.contextual_bwd) against the float64 definition
losses.contextual_loss_torch.

Inputs: independent Gaussian features saturate the loss (CX -> 1, the gradient underflows) and test nothing, so the maps are
correlated fields: a rank-8 field z [B,8,h+1,w+1] of 5 x 5 box-blurred Gaussian noise times 5, mixed to C channels by a Gaussian
matrix; y = relu(f[:, :, :h, :w]), x = relu(f[:, :, 1:, 1:] + 0.1 noise).  Asserted per case: the float64 CX of every sample lies
in [0.05, 0.98]; the device's jmin / imax differ from the float64 ones in at most 0.5 % of rows / columns, and where they do the
two candidates' float64 values agree to 1e-5 relative.  The float64 gradient the kernels are compared with routes through the
device's own selections.

Yardstick: the same formula in torch fp32 on the GPU against float64, measured here.  The kernels' loss error and their gradient's
relative L2 error may be at most 4 x that (another summation order over up to 512 channels and 1600 positions); the loss yardstick
has a floor of one fp32 ulp of the loss."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (C, h, w, band_width): below one tile; ragged; 480; 512 channels; the shipped tap size (several row and column blocks)
SHAPES = [(64, 9, 7, 0.5), (128, 10, 13, 0.5), (128, 10, 13, 0.1), (256, 24, 20, 0.5), (512, 12, 10, 0.5), (256, 40, 40, 0.5)]
IDS = [f'c{c}_{h}x{w}_bw{bw}' for c, h, w, bw in SHAPES]
B, GUP, WEIGHT, LOSS_WEIGHT = 2, 1.7, 0.6, 0.5
ULP32 = 2.0 ** -23


@pytest.fixture(autouse=True, scope='module')
def _own_zero_chunks():
    """the module's launches draw their zeroed accumulator words (hip.zeros_f32) from chunks of their own and leave the process-wide
    chunk cursor where they found it: tests elsewhere that compare the kernel lists of two steps see its fill launches"""
    from mrefsr_amd import hip
    kept = dict(hip._zero_chunks.entries)
    hip._zero_chunks.entries.clear()
    yield
    hip._zero_chunks.entries.clear()
    hip._zero_chunks.entries.update(kept)


def fields(c, h, w, b, seed):
    """(x, y) [b,c,h,w] float64 on the CPU: the correlated fields of the module docstring"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(b, 8, h + 1, w + 1, generator=g, dtype=torch.float64)
    z = F.avg_pool2d(F.pad(z, (2, 2, 2, 2), mode='replicate'), 5, 1) * 5
    f = torch.einsum('ck,bkhw->bchw', torch.randn(c, 8, generator=g, dtype=torch.float64), z)
    y = F.relu(f[:, :, :h, :w])
    x = F.relu(f[:, :, 1:, 1:] + 0.1 * torch.randn(b, c, h, w, generator=g, dtype=torch.float64))
    return x.contiguous(), y.contiguous()


def definition(x, y, bw, jmin=None, imax=None):
    """contextual_loss_torch in the tensors' dtype and on their device -> (loss, d loss / d x, parts)"""
    from mrefsr_amd.losses import contextual_loss_torch
    xr = x.detach().clone().requires_grad_(True)
    loss, parts = contextual_loss_torch(xr, y, bw, jmin=jmin, imax=imax, parts=True)
    loss.backward()
    return loss.detach(), xr.grad, parts


def rel_l2(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


@functools.lru_cache(maxsize=None)
def reference(c, h, w, bw):
    """per case, computed once and left unchanged: the inputs, the float64 definition, and the yardstick -- torch fp32 on the GPU
    against float64 routed through torch fp32's own selections"""
    x, y = fields(c, h, w, B, seed=c + h)
    l64, g64, p64 = definition(x, y, bw)
    l32, g32, p32 = definition(x.float().cuda(), y.float().cuda(), bw)
    _, g64_32, _ = definition(x, y, bw, jmin=p32['jmin'].cpu(), imax=p32['imax'].cpu())
    yard_loss = max(abs(float(l32) - float(l64)) / abs(float(l64)), ULP32)
    yard_grad = rel_l2(g32, g64_32)
    return dict(x=x, y=y, loss=float(l64), grad=g64, parts=p64, yard_loss=yard_loss, yard_grad=yard_grad)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def device_run(x, y, bw, gup=GUP, weight=WEIGHT, loss_weight=LOSS_WEIGHT, into=None):
    """-> (total [1], saved, d (gup total) / d x [B,h,w,C], max |g| [1])"""
    from mrefsr_amd import hip
    xd, yd = nhwc(x), nhwc(y)
    total, s = hip.contextual_fwd(xd, yd, bw, weight, loss_weight)
    g = torch.empty_like(xd) if into is None else into
    amax = hip.contextual_bwd(s, bw, loss_weight * weight, g, gup=torch.tensor([gup], device='cuda'), accumulate=into is not None)
    return total, s, g, amax


@pytest.mark.parametrize('c,h,w,bw', SHAPES, ids=IDS)
def test_loss_and_gradient_against_float64(c, h, w, bw):
    ref = reference(c, h, w, bw)
    n = h * w
    p64 = ref['parts']
    assert all(0.05 <= v <= 0.98 for v in p64['CX'].tolist()), p64['CX']
    total, s, g, amax = device_run(ref['x'], ref['y'], bw)
    jmin, imax = s['jmin'].cpu().long(), s['imax'].cpu().long()
    assert int(jmin.min()) >= 0 and int(jmin.max()) < n and int(imax.min()) >= 0 and int(imax.max()) < n
    # selections: few differ, and only between candidates that are equal to 1e-5 in float64
    dj, di = jmin != p64['jmin'], imax != p64['imax']
    assert int(dj.sum()) <= 0.005 * B * n and int(di.sum()) <= 0.005 * B * n, (int(dj.sum()), int(di.sum()))
    d_dev, d_ref = p64['d'].gather(2, jmin.unsqueeze(2)).squeeze(2), p64['d'].gather(2, p64['jmin'].unsqueeze(2)).squeeze(2)
    c_dev, c_ref = p64['cx'].gather(1, imax.unsqueeze(1)).squeeze(1), p64['cx'].gather(1, p64['imax'].unsqueeze(1)).squeeze(1)
    assert bool(((d_dev - d_ref).abs() <= 1e-5 * d_ref.abs())[dj].all()) and bool(((c_dev - c_ref).abs() <= 1e-5 * c_ref.abs())[di].all())
    # values: the tap loss, CX, the weighted total
    l64, g64, _ = definition(ref['x'], ref['y'], bw, jmin=jmin, imax=imax)
    loss_err = abs(float(s['tap_loss']) - float(l64)) / abs(float(l64))
    cx_err = float(((s['cx'].cpu().double() - p64['CX']).abs() / p64['CX']).max())
    want_total = torch.tensor(float(s['tap_loss'])) * torch.tensor(WEIGHT) * torch.tensor(LOSS_WEIGHT)
    grad_err = rel_l2(g.permute(0, 3, 1, 2), GUP * LOSS_WEIGHT * WEIGHT * g64)
    print(f'{c} x {h} x {w}, band {bw}: CX {[round(v, 4) for v in p64["CX"].tolist()]}, loss {float(l64):.6f}; differing jmin {int(dj.sum())} '
          f'imax {int(di.sum())} of {B * n}; loss rel err {loss_err:.2e} (torch fp32 {ref["yard_loss"]:.2e}), CX rel err {cx_err:.2e}, gradient '
          f'rel L2 err {grad_err:.2e} (torch fp32 {ref["yard_grad"]:.2e})')
    assert float(total) == float(want_total)
    assert loss_err <= 4 * ref['yard_loss']
    assert grad_err <= 4 * ref['yard_grad']
    assert float(amax) == float(g.abs().max()) > 0


def test_two_calls_give_identical_bits_and_the_inputs_are_not_written():
    from mrefsr_amd import hip
    c, h, w, bw = SHAPES[3]
    ref = reference(c, h, w, bw)
    xd, yd = nhwc(ref['x']), nhwc(ref['y'])
    x0, y0 = xd.clone(), yd.clone()
    runs = []
    for _ in range(2):
        total, s = hip.contextual_fwd(xd, yd, bw, WEIGHT, LOSS_WEIGHT)
        g = torch.empty_like(xd)
        amax = hip.contextual_bwd(s, bw, LOSS_WEIGHT * WEIGHT, g, gup=torch.tensor([GUP], device='cuda'))
        runs.append([total, g, amax] + [s[k] for k in ('xn', 'yn', 'rnorm', 'rowf', 'jmin', 'cxmax', 'imax', 'cx', 'tap_loss')])
        hip._scratch(xd.device, 1 << 20).fill_(0x5a)   # whatever the calls left in scratch is dead
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.equal(xd, x0) and torch.equal(yd, y0)


def test_upstream_gradient_and_weights_scale_the_result():
    """powers of two scale every product exactly: the gradient doubles bit for bit with the upstream value and with the coefficient;
    the running total adds the taps in order and is scaled by loss_weight"""
    from mrefsr_amd import hip
    c, h, w, bw = SHAPES[1]
    ref = reference(c, h, w, bw)
    _, s, g1, _ = device_run(ref['x'], ref['y'], bw, gup=1.0, weight=1.0, loss_weight=1.0)
    _, _, g2, a2 = device_run(ref['x'], ref['y'], bw, gup=2.0, weight=0.5, loss_weight=4.0)
    assert torch.equal(g2, 4.0 * g1) and float(a2) == float(g2.abs().max())
    g3 = torch.empty_like(g1)
    hip.contextual_bwd(s, bw, 1.0, g3, gup=None)
    assert torch.equal(g3, g1)
    xd, yd = nhwc(ref['x']), nhwc(ref['y'])
    t1, s1 = hip.contextual_fwd(xd, yd, bw, 0.3, 0.7)
    first = s1['tap_loss'].clone()
    t2, s2 = hip.contextual_fwd(yd, xd, bw, 1.1, 0.7, run=s1['run'])
    want = (first * 0.3 + s2['tap_loss'] * 1.1) * 0.7
    assert torch.equal(t1, (first * 0.3) * 0.7) and torch.equal(t2, want) and s2['run'] is s1['run']


def test_samples_are_independent():
    """B = 2 gives the bits of each sample alone: statistics and selections as they are, the tap loss up to the final mean, the
    gradient times 1 / 2 (the batch mean, a power of two)"""
    c, h, w, bw = SHAPES[1]
    ref = reference(c, h, w, bw)
    _, s, g, _ = device_run(ref['x'], ref['y'], bw)
    alone = []
    for b in range(B):
        _, sb, gb, _ = device_run(ref['x'][b:b + 1], ref['y'][b:b + 1], bw)
        for k in ('xn', 'yn', 'rnorm', 'jmin', 'cxmax', 'imax', 'cx'):
            assert torch.equal(s[k][b:b + 1], sb[k]), k
        assert torch.equal(s['rowf'][:, b:b + 1], sb['rowf'])
        assert torch.equal(g[b:b + 1], 0.5 * gb)
        alone.append(float(sb['tap_loss']))
    assert abs(float(s['tap_loss']) - sum(alone) / B) <= 2 * ULP32 * abs(float(s['tap_loss']))


def test_accumulate_adds_to_a_non_empty_tap_gradient():
    c, h, w, bw = SHAPES[0]
    ref = reference(c, h, w, bw)
    _, _, g, _ = device_run(ref['x'], ref['y'], bw)
    g0 = torch.randn(g.shape, generator=torch.Generator().manual_seed(5)).cuda() * float(g.abs().max())
    _, _, acc, amax = device_run(ref['x'], ref['y'], bw, into=g0.clone())
    assert torch.equal(acc, g0 + g) and float(amax) == float(acc.abs().max())


def test_an_output_without_grad_runs_the_forward_only(monkeypatch):
    from mrefsr_amd import hip
    from mrefsr_amd.losses import ContextualLoss
    import synth
    loss = ContextualLoss({'relu2_2': 1.0}, band_width=0.5).cuda()
    spec = [(k, tuple(v.shape)) for k, v in loss.state_dict().items()]
    loss.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()})
    g = torch.Generator().manual_seed(6)
    gt = torch.rand(1, 3, 24, 20, generator=g).cuda()
    x = (gt + 0.05 * torch.randn(1, 3, 24, 20, generator=g).cuda())
    with_grad = loss(x.clone().requires_grad_(True), gt)

    def gone(*a, **kw):
        raise AssertionError('the backward ran for an output without grad')
    monkeypatch.setattr(hip, 'contextual_bwd', gone)
    plain = loss(x, gt)
    assert not plain.requires_grad and with_grad.requires_grad and torch.equal(plain, with_grad.detach())
    assert plain.dim() == 0 and bool(torch.isfinite(plain))
