"""GPU: the kernels of csrc/texture.hip against the torch restatement of tests/test_texture_cpu.py (selection and swap: bit for bit)
and against fp64 (coefficients, the weighted Gram-Frobenius criterion and its backward)."""
import pytest
import torch
import torch.nn.functional as F

from test_texture_cpu import select, swap

pytestmark = pytest.mark.gpu

H, W = 12, 8
CH = {1: 256, 2: 128, 4: 64}


def _bits(valid):
    return (valid.int() << torch.arange(valid.shape[1], dtype=torch.int32)).sum(1).int().cuda()


def _case(K, B, seed, absent=True):
    """matcher outputs with planted ties, the first and the last patch index, and (K = 3) one absent reference that would win"""
    gh, gw = H - 2, W - 2
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, gh * gw, (K, B, gh, gw), generator=g)
    idx[0, 0, 0, 0], idx[K - 1, B - 1, -1, -1], idx[0, B - 1, 4, 2] = 0, gh * gw - 1, gh * gw - 1
    val = torch.rand(K, B, gh, gw, generator=g) * 3
    valid = torch.ones(B, K, dtype=torch.bool)
    if K > 1:
        val[1, :, 2] = val[0, :, 2]
        val[K - 1, 0, 5] = val[0, 0, 5]
        if absent:
            val[2, 1] = 5.0
            valid[1, 2] = False
    feats = {s: torch.relu(torch.randn(K, B, CH[s], s * H, s * W, generator=g)) for s in (1, 2, 4)}
    return idx, val, valid, feats


def _run(idx, val, valid, feats, masked=True):
    from mrefsr_amd import hip
    K, B = idx.shape[:2]
    sel, wts, pidx = hip.texture_select(idx.cuda(), val.cuda(), _bits(valid) if masked else None)
    maps = {}
    for s, f in feats.items():
        nhwc = f.cuda().permute(0, 1, 3, 4, 2).reshape(K * B, s * H, s * W, -1).contiguous()
        maps[s] = hip.texture_swap_nhwc(nhwc, sel, pidx, K, s).permute(0, 3, 1, 2)
    return sel, wts, pidx, maps


@pytest.mark.parametrize('K', [3, 1])
def test_selection_and_swap_bit_equal_to_the_restatement(K):
    idx, val, valid, feats = _case(K, 2, seed=K)
    sel, wts, pidx, maps = _run(idx, val, valid, feats)
    rsel, rwts, rpidx = select(idx.cuda(), val.cuda(), valid.cuda())
    assert torch.equal(sel.long(), rsel) and torch.equal(wts[:, 0], rwts) and torch.equal(pidx.long(), rpidx)
    if K > 1:
        assert not bool((sel[1] == 2).any()) and not bool((sel[:, 2] == 1).any())     # the absent reference; the planted ties
    for s, f in feats.items():
        want = swap(f.cuda(), rsel, rpidx, s, H, W)
        assert torch.equal(maps[s], want), s
    assert torch.equal(_run(idx, val, valid, feats)[3][4], maps[4])


def test_swap_identity():
    gh, gw = H - 2, W - 2
    idx, val, valid, feats = _case(1, 2, seed=7)
    own = torch.arange(gh * gw).view(1, 1, gh, gw).expand(1, 2, gh, gw).contiguous()
    maps = _run(own, val, valid, feats, masked=False)[3]
    for s, f in feats.items():
        ref = f[0].cuda()
        err = float(((maps[s] - ref).abs() / ref.abs().clamp_min(1e-30))[ref != 0].max())
        print(f'identity swap, scale {s}: max relative error {err:.2e}')
        assert err <= 1e-6, (s, err)
        assert bool((maps[s][ref == 0] == 0).all())


def test_masked_sample_equals_the_sample_fed_alone_with_its_valid_references():
    idx, val, valid, feats = _case(3, 2, seed=5)
    maps = _run(idx, val, valid, feats)[3]
    alone = _run(idx[:2, 1:2].contiguous(), val[:2, 1:2].contiguous(), valid[1:2, :2], {s: f[:2, 1:2].contiguous() for s, f in feats.items()},
                 masked=False)[3]
    for s in feats:
        assert torch.equal(maps[s][1:2], alone[s]), s


def test_coefficients_against_fp64():
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(3)
    wts = torch.rand(2, 1, H - 2, W - 2, generator=g) * 3
    wts[0, 0, 0, 0], wts[1, 0, -1, -1] = 0.0, 3.0
    got = hip.texture_coeff(wts.cuda())
    pad = F.pad(wts.double(), (1, 1, 1, 1), mode='replicate')
    for s in (1, 2, 4):
        want = torch.sigmoid(F.interpolate(pad, None, s, 'bicubic', True) * (-20.) + .65)[:, 0]
        err = float((got[s].cpu().double() - want).abs().max())
        print(f'coeff, scale {s}: max abs error {err:.2e}')
        assert got[s].shape == want.shape and err <= 2e-5, (s, err)


def _crit_ref(fs, ms, cs, divs, lw, up):
    """fp64 autograd of the weighted Gram-Frobenius criterion: -> (norms, terms, total, [d (total * up) / d f])"""
    fs = [f.double().cpu().requires_grad_(True) for f in fs]
    norms, terms = [], []
    for f, m, c in zip(fs, ms, cs):
        n, h, w, ch = f.shape
        fc = (f * c.double().cpu()[..., None]).reshape(n, h * w, ch)
        mc = (m.double().cpu() * c.double().cpu()[..., None]).reshape(n, h * w, ch)
        norms.append(torch.norm(fc.transpose(1, 2) @ fc - mc.transpose(1, 2) @ mc))
    terms = [nm / 4. / d for nm, d in zip(norms, divs)]
    total = sum(terms) / 3. * lw
    (total * up).backward()
    return [v.detach() for v in norms], [v.detach() for v in terms], total.detach(), [f.grad for f in fs]


# (C, pixels as h x w): the three channel counts; 96, 384 and 63 pixels (63: no multiple of the 16-pixel MFMA tile)
CRIT_SHAPES = [((256, 12, 8), (128, 24, 16), (64, 7, 9)), ((64, 12, 8), (256, 7, 9), (128, 24, 16))]


@pytest.mark.parametrize('shapes', CRIT_SHAPES, ids=['a', 'b'])
@pytest.mark.parametrize('accumulate', [False, True])
def test_criterion_and_its_backward_against_fp64(shapes, accumulate):
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(len(shapes) + accumulate)
    n, lw, up = 2, 1e-3, 0.5
    fs = [torch.relu(torch.randn(n, h, w, c, generator=g)).cuda() for c, h, w in shapes]
    ms = [torch.relu(torch.randn(n, h, w, c, generator=g)).cuda() for c, h, w in shapes]
    cs = [torch.rand(n, h, w, generator=g).cuda() for c, h, w in shapes]
    divs = [float((32 * 32 * d) ** 2) for d in (256, 512, 1024)]
    fcs = [hip.texture_scale_nhwc(f, c) for f, c in zip(fs, cs)]
    assert all(torch.equal(fc, f * c[..., None]) for fc, f, c in zip(fcs, fs, cs))
    gxs = [hip.gram_raw_nhwc(fc) for fc in fcs]
    gms = [hip.gram_raw_nhwc(hip.texture_scale_nhwc(m, c)) for m, c in zip(ms, cs)]
    norms, terms, total = hip.texture_crit(gxs, gms, divs, lw)
    rn, rt, rtot, rgrads = _crit_ref(fs, ms, cs, divs, lw, up)
    for l in range(3):
        e_n, e_t = abs(float(norms[l]) - float(rn[l])) / float(rn[l]), abs(float(terms[l]) - float(rt[l])) / float(rt[l])
        print(f'layer {shapes[l]}: norm rel err {e_n:.2e}, term rel err {e_t:.2e}')
        assert e_n <= 1e-5 and e_t <= 1e-5
    e = abs(float(total) - float(rtot)) / float(rtot)
    print(f'total rel err {e:.2e}')
    assert e <= 1e-5
    gup = torch.tensor([up], device='cuda')
    for l in range(3):
        want = rgrads[l]
        base = (torch.randn(fs[l].shape, generator=g) * float(want.abs().max())).cuda() if accumulate else torch.empty_like(fs[l])
        df = base.clone()
        amax = hip.texture_gram_bwd_nhwc(fcs[l], gxs[l], gms[l], cs[l], norms[l:l + 1], df, lw / 3. / 4. / divs[l], gup=gup,
                                         accumulate=accumulate)
        got = df.double().cpu() - (base.double().cpu() if accumulate else 0)
        err = float((got - want).norm() / want.norm())
        print(f'layer {shapes[l]}: dF rel L2 err {err:.2e} (|dF| max {float(want.abs().max()):.2e})')
        # (accumulate: the sum base + dF is rounded at base's magnitude, ~|dF| max: 2^-24 per element on top)
        assert err <= 1e-5, err
        assert float(amax) == float(df.abs().max())
        df2 = base.clone()
        hip.texture_gram_bwd_nhwc(fcs[l], gxs[l], gms[l], cs[l], norms[l:l + 1], df2, lw / 3. / 4. / divs[l], gup=gup, accumulate=accumulate)
        assert torch.equal(df, df2)
    n2, t2, tot2 = hip.texture_crit(gxs, gms, divs, lw)
    assert torch.equal(n2, norms) and torch.equal(t2, terms) and torch.equal(tot2, total)


def test_criterion_with_equal_grams_is_zero_with_zero_gradient():
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(9)
    f = torch.relu(torch.randn(2, 7, 9, 64, generator=g)).cuda()
    c = torch.rand(2, 7, 9, generator=g).cuda()
    fc = hip.texture_scale_nhwc(f, c)
    gx = hip.gram_raw_nhwc(fc)
    norms, terms, total = hip.texture_crit([gx], [gx.clone()], [1e6], 1.0)
    assert float(norms[0]) == 0.0 and float(terms[0]) == 0.0 and float(total) == 0.0
    df = torch.full_like(f, float('nan'))
    amax = hip.texture_gram_bwd_nhwc(fc, gx, gx.clone(), c, norms[0:1], df, 1e-6)
    assert bool((df == 0).all()) and float(amax) == 0.0
    base = torch.randn(f.shape, generator=g).cuda()
    df = base.clone()
    hip.texture_gram_bwd_nhwc(fc, gx, gx.clone(), c, norms[0:1], df, 1e-6, accumulate=True)
    assert torch.equal(df, base)


def test_shape_errors():
    from mrefsr_amd import hip
    z = torch.zeros(2, 4, 4, 64, device='cuda')
    with pytest.raises(ValueError):
        hip.texture_scale_nhwc(z, torch.zeros(2, 4, 5, device='cuda'))
    with pytest.raises(ValueError):
        hip.texture_swap_nhwc(z, torch.zeros(2, 2, 2, dtype=torch.int32, device='cuda'), torch.zeros(2, 2, 2, dtype=torch.int32, device='cuda'), 3, 1)
    with pytest.raises(ValueError):
        hip.texture_select(torch.zeros(1, 2, 2, 2, dtype=torch.int64, device='cuda'), torch.zeros(1, 2, 2, 3, device='cuda'))
    with pytest.raises(ValueError):
        hip.texture_coeff(torch.zeros(2, 2, 2, device='cuda'))
    with pytest.raises(NotImplementedError):
        hip.texture_coeff(torch.zeros(2, 1, 2, 2))
