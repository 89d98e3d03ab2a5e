"""GPU: the CoBi kernels of csrc/contextual.hip -- cx_dist with the spatial term (hip.contextual_fwd / hip.contextual_bwd with
weight_sp), hip.cx_patches / hip.cx_subsample and their adjoints -- against the float64 definitions losses.contextual_loss_torch and
losses.cx_patches_torch.

The method is that of tests/test_contextual_kernels_gpu.py (restated here, not imported), B = 2: correlated feature fields; the
float64 CX of every sample in [0.05, 0.98]; the device's jmin / imax differ from the float64 ones in at most 0.5 % of rows / columns,
and only between candidates whose float64 values agree to 1e-5 relative; the float64 gradient the kernels are compared with routes
through the device's own selections.  Yardstick: the same formula in torch fp32 on the GPU against float64; the kernels' loss error
and their gradient's relative L2 error may be at most 4 x that, with a floor of one fp32 ulp for the loss.

The copies (patches forward, subsample and its adjoint) are compared bit for bit.  The patch adjoint adds n <= ceil(size / stride)^2
terms per pixel one after the other in fp32: |error| <= (n - 1) 2^-24 sum |terms| against float64 F.fold."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (C, h, w, band_width, weight_sp): below one tile; ragged; the transposed grid; N = 165, three column tiles, w >> h; the shipped tap
SP_CASES = [(64, 9, 7, 0.5, 0.1), (128, 10, 13, 0.1, 0.5), (128, 13, 10, 0.5, 0.1), (64, 5, 33, 0.5, 0.25), (256, 40, 40, 0.5, 0.1)]
DECISIVE = (64, 9, 14, 0.5, 0.1)   # a field periodic along w: the spatial term decides most selections
# (H, W, size, stride, weight_sp): ragged right and bottom edges, stride that does not divide size, Cpad 64 / 128 / 128 / 256
PATCH_CASES = [(17, 14, 3, 2, 0.1), (23, 19, 5, 3, 0.1), (20, 26, 5, 2, 0.0), (24, 24, 7, 4, 0.1)]
B, GUP, WEIGHT, LOSS_WEIGHT = 2, 1.7, 0.6, 0.5
ULP32 = 2.0 ** -23
SAVED = ('xn', 'yn', 'rnorm', 'rowf', 'jmin', 'cxmax', 'imax', 'cx', 'tap_loss')


def _id(case):
    return '_'.join(str(v) for v in case)


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
    """(x, y) [b,c,h,w] float64 on the CPU: a rank-8 field of 5 x 5 box-blurred Gaussian noise times 5 mixed to c channels;
    y = relu(f[:, :, :h, :w]), x = relu(f[:, :, 1:, 1:] + 0.1 noise)"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(b, 8, h + 1, w + 1, generator=g, dtype=torch.float64)
    z = F.avg_pool2d(F.pad(z, (2, 2, 2, 2), mode='replicate'), 5, 1) * 5
    f = torch.einsum('ck,bkhw->bchw', torch.randn(c, 8, generator=g, dtype=torch.float64), z)
    y = F.relu(f[:, :, :h, :w])
    x = F.relu(f[:, :, 1:, 1:] + 0.1 * torch.randn(b, c, h, w, generator=g, dtype=torch.float64))
    return x.contiguous(), y.contiguous()


def periodic_fields(c, h, w, b, seed):
    """a field with period 4 along w (repetitive texture: the cosine distance alone cannot tell the periods apart): randn
    [b,8,h+1,4] tiled to w + 1 columns, box-blurred over 5 rows, times 3, mixed to c channels; y = relu(f[:, :, :h, :w] + 0.05
    noise), x = relu(f[:, :, 1:, 1:] + 0.05 noise)"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(b, 8, h + 1, 4, generator=g, dtype=torch.float64)
    z = z.repeat(1, 1, 1, (w + 4) // 4)[..., :w + 1]
    z = F.avg_pool2d(F.pad(z, (0, 0, 2, 2), mode='replicate'), (5, 1), 1) * 3
    f = torch.einsum('ck,bkhw->bchw', torch.randn(c, 8, generator=g, dtype=torch.float64), z)
    y = F.relu(f[:, :, :h, :w] + 0.05 * torch.randn(b, c, h, w, generator=g, dtype=torch.float64))
    x = F.relu(f[:, :, 1:, 1:] + 0.05 * torch.randn(b, c, h, w, generator=g, dtype=torch.float64))
    return x.contiguous(), y.contiguous()


def shifted_images(h, w, b, seed):
    """(output, gt) [b,3,h,w] float64: a smooth random image (rand bicubic-upsampled x 2, clamped to [0, 1]); the GT one crop of it,
    the output the crop one pixel down and right plus 0.02 noise"""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(b, 3, (h + 2) // 2, (w + 2) // 2, generator=g, dtype=torch.float64)
    big = F.interpolate(base, scale_factor=2, mode='bicubic', align_corners=False).clamp(0, 1)
    gt = big[:, :, :h, :w]
    x = big[:, :, 1:h + 1, 1:w + 1] + 0.02 * torch.randn(b, 3, h, w, generator=g, dtype=torch.float64)
    return x.contiguous(), gt.contiguous()


def definition(x, y, bw, ws, jmin=None, imax=None, patch=None):
    """contextual_loss_torch (on the patches of the images x, y when patch = (size, stride)) in the tensors' dtype and on their device
    -> (loss, d loss / d x, parts)"""
    from mrefsr_amd.losses import contextual_loss_torch, cx_patches_torch
    xr = x.detach().clone().requires_grad_(True)
    fx, fy = (xr, y) if patch is None else (cx_patches_torch(xr, *patch), cx_patches_torch(y, *patch))
    loss, parts = contextual_loss_torch(fx, fy, bw, jmin=jmin, imax=imax, parts=True, weight_sp=ws)
    loss.backward()
    return loss.detach(), xr.grad, parts


def rel_l2(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


@functools.lru_cache(maxsize=None)
def reference(kind, c, h, w, bw, ws, patch=None):
    """per case, computed once and left unchanged: the inputs, the float64 definition, and the yardstick -- torch fp32 on the GPU
    against float64 routed through torch fp32's own selections"""
    x, y = {'fields': fields, 'periodic': periodic_fields}[kind](c, h, w, B, seed=c + h) if patch is None else shifted_images(h, w, B, seed=h + w)
    l64, g64, p64 = definition(x, y, bw, ws, patch=patch)
    l32, g32, p32 = definition(x.float().cuda(), y.float().cuda(), bw, ws, patch=patch)
    _, g64_32, _ = definition(x, y, bw, ws, jmin=p32['jmin'].cpu(), imax=p32['imax'].cpu(), patch=patch)
    yard_loss = max(abs(float(l32) - float(l64)) / abs(float(l64)), ULP32)
    return dict(x=x, y=y, loss=float(l64), grad=g64, parts=p64, yard_loss=yard_loss, yard_grad=rel_l2(g32, g64_32))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def device_run(xd, yd, bw, ws, gup=GUP, weight=WEIGHT, loss_weight=LOSS_WEIGHT, into=None):
    """xd, yd [B,h,w,C] on the device -> (total [1], saved, d (gup total) / d x [B,h,w,C], max |g| [1])"""
    from mrefsr_amd import hip
    total, s = hip.contextual_fwd(xd, yd, bw, weight, loss_weight, weight_sp=ws)
    g = torch.empty_like(xd) if into is None else into
    amax = hip.contextual_bwd(s, bw, loss_weight * weight, g, gup=torch.tensor([gup], device='cuda'), accumulate=into is not None, weight_sp=ws)
    return total, s, g, amax


def check_against_float64(ref, s, bw, ws, grad, label, patch=None):
    """the selections, the tap loss and the gradient ``grad`` (d (GUP total) / d x in x's layout) of a device run against ``ref``"""
    p64 = ref['parts']
    n = p64['jmin'].shape[1]
    jmin, imax = s['jmin'].cpu().long(), s['imax'].cpu().long()
    assert int(jmin.min()) >= 0 and int(jmin.max()) < n and int(imax.min()) >= 0 and int(imax.max()) < n
    dj, di = jmin != p64['jmin'], imax != p64['imax']
    assert int(dj.sum()) <= 0.005 * B * n and int(di.sum()) <= 0.005 * B * n, (int(dj.sum()), int(di.sum()))
    d_dev, d_ref = p64['d'].gather(2, jmin.unsqueeze(2)).squeeze(2), p64['d'].gather(2, p64['jmin'].unsqueeze(2)).squeeze(2)
    c_dev, c_ref = p64['cx'].gather(1, imax.unsqueeze(1)).squeeze(1), p64['cx'].gather(1, p64['imax'].unsqueeze(1)).squeeze(1)
    assert bool(((d_dev - d_ref).abs() <= 1e-5 * d_ref.abs())[dj].all()) and bool(((c_dev - c_ref).abs() <= 1e-5 * c_ref.abs())[di].all())
    l64, g64, _ = definition(ref['x'], ref['y'], bw, ws, jmin=jmin, imax=imax, patch=patch)
    loss_err = abs(float(s['tap_loss']) - float(l64)) / abs(float(l64))
    grad_err = rel_l2(grad, GUP * LOSS_WEIGHT * WEIGHT * g64)
    print(f'{label}: CX {[round(v, 4) for v in p64["CX"].tolist()]}, loss {float(l64):.6f}; differing jmin {int(dj.sum())} imax {int(di.sum())} '
          f'of {B * n}; loss rel err {loss_err:.2e} (torch fp32 {ref["yard_loss"]:.2e}), gradient rel L2 err {grad_err:.2e} (torch fp32 '
          f'{ref["yard_grad"]:.2e})')
    assert loss_err <= 4 * ref['yard_loss']
    assert grad_err <= 4 * ref['yard_grad']


@pytest.mark.parametrize('case', SP_CASES, ids=_id)
def test_spatial_term_against_float64(case):
    c, h, w, bw, ws = case
    ref = reference('fields', *case)
    assert all(0.05 <= v <= 0.98 for v in ref['parts']['CX'].tolist()), ref['parts']['CX']
    total, s, g, amax = device_run(nhwc(ref['x']), nhwc(ref['y']), bw, ws)
    want_total = torch.tensor(float(s['tap_loss'])) * torch.tensor(WEIGHT) * torch.tensor(LOSS_WEIGHT)
    assert float(total) == float(want_total)
    check_against_float64(ref, s, bw, ws, g.permute(0, 3, 1, 2), f'{case}')
    assert float(amax) == float(g.abs().max()) > 0


def test_a_case_where_the_spatial_term_decides():
    """The row minima of this case are 8e-4 ... 1e-3: with fp32 norms and an fp32 distance product the kernels' loss was 9.0e-7 off
    (the bound: 4 x torch fp32's 1.24e-7) and this test failed; with both in double (cx_normalise<true>, cx_dist<true> on the f64
    MFMA: what the weight_sp entry points launch) it is 4.6e-8 off and the gradient 2.3e-5 against torch fp32's 3.9e-4."""
    c, h, w, bw, ws = DECISIVE
    ref = reference('periodic', *DECISIVE)
    _, _, plain = definition(ref['x'], ref['y'], bw, 0.0)
    p64 = ref['parts']
    moved_j = float((plain['jmin'] != p64['jmin']).double().mean())
    moved_i = float((plain['imax'] != p64['imax']).double().mean())
    print(f'{DECISIVE}: float64 CX {p64["CX"].tolist()} (ws = 0: {plain["CX"].tolist()}); selections that differ from ws = 0: jmin '
          f'{moved_j:.2f}, imax {moved_i:.2f}')
    assert all(0.05 <= v <= 0.98 for v in p64['CX'].tolist()), p64['CX']
    assert moved_j >= 0.5 and moved_i >= 0.5
    _, s, g, amax = device_run(nhwc(ref['x']), nhwc(ref['y']), bw, ws)
    check_against_float64(ref, s, bw, ws, g.permute(0, 3, 1, 2), f'{DECISIVE} periodic')
    assert float(amax) == float(g.abs().max()) > 0


def _sp_entry_points(xd, yd, bw, ws, weight, loss_weight, gup, into=None):
    """the library's *_sp entry points called directly (hip.contextual_fwd routes weight_sp = 0 to the plain ones)
    -> (total, saved, g, amax)"""
    from mrefsr_amd import _lib, hip
    b, h, w, c = xd.shape
    n, dev = h * w, xd.device
    f32 = dict(device=dev, dtype=torch.float32)
    s = dict(xn=torch.empty_like(xd), yn=torch.empty_like(xd), rnorm=torch.empty((b, n), **f32), rowf=torch.empty((2, b, n), **f32),
             jmin=torch.empty((b, n), device=dev, dtype=torch.int32), cxmax=torch.empty((b, n), **f32),
             imax=torch.empty((b, n), device=dev, dtype=torch.int32), cx=torch.empty(b, **f32), tap_loss=torch.empty(1, **f32),
             run=torch.empty(1, **f32))
    total = torch.empty(1, **f32)
    p = hip._p
    need = hip._cx_workspace('contextual_fwd', b, n, c, False)
    _lib.call('mrefsr_contextual_fwd_sp_f32', p(xd), p(yd), b, h, w, c, C.c_float(bw), C.c_float(ws), p(s['xn']), p(s['yn']), p(s['rnorm']),
              p(s['rowf']), p(s['jmin']), p(s['cxmax']), p(s['imax']), p(s['cx']), p(s['tap_loss']), C.c_float(weight), C.c_float(loss_weight),
              1, p(s['run']), p(total), p(hip._scratch(dev, need)), C.c_int64(need), hip._stream())
    g = torch.empty_like(xd) if into is None else into
    amax = torch.zeros(1, **f32)
    up = torch.tensor([gup], device=dev)
    need = hip._cx_workspace('contextual_bwd', b, n, c, True)
    _lib.call('mrefsr_contextual_bwd_sp_f32', p(s['xn']), p(s['yn']), p(s['rnorm']), b, h, w, c, C.c_float(bw), C.c_float(ws), p(s['rowf']),
              p(s['jmin']), p(s['cxmax']), p(s['imax']), p(s['cx']), p(up), C.c_float(loss_weight * weight), p(g), 0 if into is None else 1,
              p(amax), p(hip._scratch(dev, need)), C.c_int64(need), hip._stream())
    return total, s, g, amax


@pytest.mark.parametrize('case', [SP_CASES[1], SP_CASES[3]], ids=_id)
def test_weight_sp_zero_through_the_new_entry_points_is_the_plain_loss_bit_for_bit(case):
    c, h, w, bw, _ = case
    ref = reference('fields', *case)
    xd, yd = nhwc(ref['x']), nhwc(ref['y'])
    t0, s0, g0, a0 = device_run(xd, yd, bw, 0.0)
    t1, s1, g1, a1 = _sp_entry_points(xd, yd, bw, 0.0, WEIGHT, LOSS_WEIGHT, GUP)
    assert torch.equal(t0, t1) and torch.equal(g0, g1) and torch.equal(a0, a1)
    for k in SAVED + ('run',):
        assert torch.equal(s0[k], s1[k]), k
    # (and the entry points are the ones hip.contextual_fwd / hip.contextual_bwd call with a weight: the same bits again)
    ws = case[4]
    t2, s2, g2, a2 = device_run(xd, yd, bw, ws)
    t3, s3, g3, a3 = _sp_entry_points(xd, yd, bw, ws, WEIGHT, LOSS_WEIGHT, GUP)
    assert torch.equal(t2, t3) and torch.equal(g2, g3) and torch.equal(a2, a3) and not torch.equal(t2, t0)
    assert all(torch.equal(s2[k], s3[k]) for k in SAVED)


def test_two_calls_give_identical_bits_and_the_inputs_are_not_written():
    from mrefsr_amd import hip
    c, h, w, bw, ws = SP_CASES[3]
    ref = reference('fields', *SP_CASES[3])
    xd, yd = nhwc(ref['x']), nhwc(ref['y'])
    x0, y0 = xd.clone(), yd.clone()
    runs = []
    for _ in range(2):
        total, s, g, amax = device_run(xd, yd, bw, ws)
        runs.append([total, g, amax] + [s[k] for k in SAVED])
        hip._scratch(xd.device, 1 << 20).fill_(0x5a)   # whatever the calls left in scratch is dead
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.equal(xd, x0) and torch.equal(yd, y0)


def test_samples_are_independent():
    """B = 2 gives the bits of each sample alone: statistics and selections as they are, the gradient times 1 / 2"""
    c, h, w, bw, ws = SP_CASES[2]
    ref = reference('fields', *SP_CASES[2])
    xd, yd = nhwc(ref['x']), nhwc(ref['y'])
    _, s, g, _ = device_run(xd, yd, bw, ws)
    for b in range(B):
        _, sb, gb, _ = device_run(xd[b:b + 1], yd[b:b + 1], bw, ws)
        for k in ('xn', 'yn', 'rnorm', 'jmin', 'cxmax', 'imax', 'cx'):
            assert torch.equal(s[k][b:b + 1], sb[k]), k
        assert torch.equal(s['rowf'][:, b:b + 1], sb['rowf'])
        assert torch.equal(g[b:b + 1], 0.5 * gb)


def test_accumulate_adds_to_a_non_empty_tap_gradient():
    c, h, w, bw, ws = SP_CASES[0]
    ref = reference('fields', *SP_CASES[0])
    xd, yd = nhwc(ref['x']), nhwc(ref['y'])
    _, _, g, _ = device_run(xd, yd, bw, ws)
    g0 = torch.randn(g.shape, generator=torch.Generator().manual_seed(5)).cuda() * float(g.abs().max())
    _, _, acc, amax = device_run(xd, yd, bw, ws, into=g0.clone())
    assert torch.equal(acc, g0 + g) and float(amax) == float(acc.abs().max())


# ---- cx_patches ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', PATCH_CASES, ids=_id)
def test_patches_forward_is_unfold_bit_for_bit(case):
    from mrefsr_amd import hip
    h, w, size, stride, _ = case
    img = torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(h)) * 2 - 1
    oh, ow, k = (h - size) // stride + 1, (w - size) // stride + 1, 3 * size * size
    cpad = hip.cx_patch_channels(size)
    assert cpad == {3: 64, 5: 128, 7: 256}[size]
    for norm in (False, True):
        src = (img + 1.) * 0.5 if norm else img
        want = F.unfold(src, size, stride=stride).reshape(B, k, oh, ow).permute(0, 2, 3, 1)
        got = hip.cx_patches(img.cuda(), size, stride, norm_img=norm).cpu()
        assert got.shape == (B, oh, ow, cpad)
        assert torch.equal(got[..., :k], want) and not bool(got[..., k:].any())


@pytest.mark.parametrize('case', PATCH_CASES, ids=_id)
def test_patches_adjoint_against_float64_fold(case):
    from mrefsr_amd import hip
    h, w, size, stride, _ = case
    oh, ow, k = (h - size) // stride + 1, (w - size) // stride + 1, 3 * size * size
    cpad = hip.cx_patch_channels(size)
    gen = torch.Generator().manual_seed(w)
    g = torch.randn(B, oh, ow, cpad, generator=gen)          # (the padding channels hold values too: the adjoint must not read them)
    cols = g[..., :k].double().permute(0, 3, 1, 2).reshape(B, k, oh * ow)
    want = F.fold(cols, (h, w), size, stride=stride)
    mag = F.fold(cols.abs(), (h, w), size, stride=stride)
    n = F.fold(torch.ones_like(cols), (h, w), size, stride=stride)       # [B,3,h,w]: the patches that cover each pixel
    assert int(n.max()) <= (-(-size // stride)) ** 2
    got = hip.cx_patches_bwd(g.cuda(), (B, 3, h, w), size, stride)
    err = (got.cpu().double() - want).abs()
    bound = (n - 1).clamp_min(0) * 2.0 ** -24 * mag
    print(f'{case}: covering patches per pixel 0 ... {int(n.max())}, uncovered pixels {int((n == 0).sum())}, max |err| {float(err.max()):.2e}, '
          f'max err / bound {float((err / bound.clamp_min(1e-300))[n > 1].max()):.2f}')
    assert bool((err <= bound).all())
    assert not bool(got.cpu()[n == 0].any())                 # an exact 0 where no patch covers the pixel
    if stride * ((h - size) // stride) + size < h or stride * ((w - size) // stride) + size < w:
        assert int((n == 0).sum()) > 0
    # scale, and accumulate: buffer + the written result in one fp32 add
    half = hip.cx_patches_bwd(g.cuda(), (B, 3, h, w), size, stride, scale=0.5)
    assert torch.equal(half, 0.5 * got)
    buf = torch.randn(B, 3, h, w, generator=gen).cuda()
    acc = hip.cx_patches_bwd(g.cuda(), (B, 3, h, w), size, stride, out=buf.clone())
    assert torch.equal(acc, buf + got)


# ---- cx_subsample --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(9, 7), (10, 13)], ids=['9x7', '10x13'])
@pytest.mark.parametrize('s', [2, 3])
def test_subsample_and_its_adjoint_bit_for_bit(h, w, s):
    from mrefsr_amd import hip
    gen = torch.Generator().manual_seed(h * s)
    f = torch.randn(B, h, w, 64, generator=gen).cuda()
    f0 = f.clone()
    sub = hip.cx_subsample(f, s)
    assert torch.equal(sub, f[:, ::s, ::s]) and sub.is_contiguous() and torch.equal(f, f0)
    gs = torch.randn(sub.shape, generator=gen).cuda()
    want = torch.zeros_like(f)
    want[:, ::s, ::s] = gs
    g = torch.full_like(f, float('nan'))                     # write mode: every element is written
    amax = hip.cx_subsample_bwd(gs, g, s)
    assert torch.equal(g, want) and float(amax) == float(want.abs().max())
    buf = torch.randn(f.shape, generator=gen).cuda()         # accumulate: one add at the sampled positions, the rest as it was
    buf[1, 1, 1, 5] = -100.0                                 # (the buffer's maximum sits at a position that is not sampled)
    acc = buf.clone()
    amax = hip.cx_subsample_bwd(gs, acc, s, accumulate=True)
    assert torch.equal(acc, buf + want) and float(amax) == float(acc.abs().max()) == 100.0
    assert hip.cx_subsample_bwd(gs, acc, s, accumulate=True, want_amax=False) is None
    one = hip.cx_subsample(f, 1)
    assert torch.equal(one, f)


# ---- the RGB tap end to end: patches -> contextual loss -> patch adjoint --------------------------------------------------------
@pytest.mark.parametrize('case', PATCH_CASES, ids=_id)
def test_rgb_tap_against_float64(case):
    from mrefsr_amd import hip
    h, w, size, stride, ws = case
    bw = 0.5
    ref = reference('images', 3, h, w, bw, ws, patch=(size, stride))
    assert all(0.05 <= v <= 0.98 for v in ref['parts']['CX'].tolist()), ref['parts']['CX']
    img = torch.cat([ref['x'], ref['y']]).float().cuda()
    p = hip.cx_patches(img, size, stride)
    _, s, gp, _ = device_run(p[:B], p[B:], bw, ws)
    g = hip.cx_patches_bwd(gp, (B, 3, h, w), size, stride)
    check_against_float64(ref, s, bw, ws, g, f'{case} RGB tap', patch=(size, stride))
