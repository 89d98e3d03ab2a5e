"""GPU: the multi-tensor EMA and Adam kernels (csrc/optim.hip) on one job table over views into flat buffers, against the float64
formulas.  The views start at odd element offsets (4-byte aligned only); sizes 0, 1, 3, 5, 63, 64, 65, 1023, 1025 (around a lane
group, a wave and the 1024-element chunk), 300 001 (a tensor of many chunks, shared by several blocks) and 400 tensors of 7
elements (more jobs than one block's share of a 2048-block launch; many jobs inside one chunk range)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 5, 63, 64, 65, 1023, 1025, 300001] + [7] * 400
SENTINEL = 12345.0


def _layout(shift=0):
    """element offsets of the views: odd (+ shift), at least one sentinel word between neighbours"""
    offs, off = [], 1
    for n in SIZES:
        off += 1 - off % 2
        offs.append(off + shift)
        off += n + 2
    return offs, off + 8


def _flat(total, fill=SENTINEL):
    return torch.full((total,), fill, device='cuda', dtype=torch.float32)


def _views(buf, offs):
    return [buf[o:o + n] for o, n in zip(offs, SIZES)]


def _fill(views, gen, scale=1.0):
    for v in views:
        v.copy_((torch.randn(v.numel(), generator=gen) * scale).cuda())


def _gaps_untouched(buf, offs):
    mask = torch.ones(buf.numel(), dtype=torch.bool)
    for o, n in zip(offs, SIZES):
        mask[o:o + n] = False
    return bool((buf.cpu()[mask] == SENTINEL).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


# streams that share their offset inside 16 bytes (16-byte accesses with 4-byte edges) and streams that do not (4-byte accesses)
SHIFTS = {'co-aligned': dict(p=0, g=0, m=0, v=0, ema=0), 'mixed': dict(p=0, g=1, m=0, v=2, ema=1)}


@pytest.mark.parametrize('decay', [0.999, 0.0])
@pytest.mark.parametrize('shifts', list(SHIFTS), ids=list(SHIFTS))
def test_ema_multi_against_the_float64_formula(decay, shifts):
    from mrefsr_amd import hip
    sh = SHIFTS[shifts]
    gen = torch.Generator().manual_seed(3)
    (po, total), (eo, _) = _layout(sh['p']), _layout(sh['ema'])
    pbuf, ebuf = _flat(total), _flat(total)
    ps, es = _views(pbuf, po), _views(ebuf, eo)
    assert all(p.data_ptr() % 16 != 0 and p.data_ptr() % 4 == 0 for p in ps if p.numel())   # (an empty view has no address)
    _fill(ps, gen)
    _fill(es, gen, 3.0)
    if decay == 0.0:
        for e in es:
            e.fill_(float('nan'))                             # the copy does not read (or is not disturbed by) what was there
    p0, e0 = pbuf.clone(), ebuf.clone()
    tab = hip.optim_table(ps, emas=es)
    assert hip.optim_table(ps, emas=es, cached=tab) is tab     # nothing moved: the same table
    version = ebuf._version
    hip.ema_multi(tab, decay, es)
    torch.cuda.synchronize()
    assert ebuf._version > version                            # written through raw pointers: the version counter is moved by hand
    assert torch.equal(_bits(pbuf), _bits(p0))                # the parameters are only read
    assert _gaps_untouched(ebuf, eo)
    d, a = np.float32(decay), np.float32(1.0 - decay)
    worst = 0.0
    for p, e, eb, o in zip(ps, es, _views(e0, eo), eo):
        if decay == 0.0:
            assert torch.equal(_bits(e), _bits(p))
            continue
        p64, e64, got = p.cpu().double().numpy(), eb.cpu().double().numpy(), e.cpu().double().numpy()
        want = float(d) * e64 + float(a) * p64
        bound = 2.0 ** -23 * np.maximum(np.abs(e64), np.abs(p64))
        assert (np.abs(got - want) <= bound).all(), (p.numel(), o)
        if p.numel():
            worst = max(worst, float((np.abs(got - want) / np.maximum(bound, 1e-300)).max()))
    print(f'ema_multi decay {decay} {shifts}: worst |err| / bound = {worst:.3f}')
    moved = hip.optim_table(ps[:-1] + [ps[-1].clone()], emas=es, cached=tab)
    assert moved is not tab                                   # an address moved: a new table


GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), dict(lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-4),
          dict(lr=2e-4, betas=(0.5, 0.999), eps=1e-6, weight_decay=0.0), dict(lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)]
EMA_DECAY = 0.999


def _adam64(p, g, m, v, grp, step):
    p, g, m, v = (x.cpu().double().numpy() for x in (p, g, m, v))
    (b1, b2), lr, eps, wd = grp['betas'], grp['lr'], grp['eps'], grp['weight_decay']
    if wd:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr / (1 - b1 ** step) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** step) + eps)
    return p, m, v


def _dev(got, want):
    return float(np.abs(got.cpu().double().numpy() - want).max()) if got.numel() else 0.0


@pytest.mark.parametrize('shifts', list(SHIFTS), ids=list(SHIFTS))
def test_adam_multi_three_steps_against_float64_and_torchs_fused_adam(shifts):
    """per step: the kernel and torch's fused Adam (the update used without train.hip_adam) start from the same fp32 state; the
    largest deviation of each from the float64 formula is taken separately for p, exp_avg and exp_avg_sq, and the kernel's may be
    at most twice torch's (the same number of roundings in a possibly different order); where torch's is 0, one fp32 ulp of the
    value.  Entries without a gradient keep p and both moments bit for bit and still get their EMA update."""
    from mrefsr_amd import hip
    sh = SHIFTS[shifts]
    gen = torch.Generator().manual_seed(11)
    lay = {k: _layout(sh[k]) for k in ('p', 'g', 'm', 'v', 'ema')}
    total = lay['p'][1]
    buf = {k: _flat(total) for k in lay}
    vw = {k: _views(buf[k], lay[k][0]) for k in lay}
    _fill(vw['p'], gen)
    _fill(vw['ema'], gen)
    for k in ('m', 'v'):
        for t in vw[k]:
            t.zero_()
    n = len(SIZES)
    group_of = [i % 4 for i in range(n)]
    no_grad = [i % 5 == 2 and i != 9 for i in range(n)]        # (the 300 001-element tensor, index 9, takes its steps)
    assert sum(no_grad) > 50 and not no_grad[9] and any(no_grad[i] and SIZES[i] > 7 for i in range(n))
    gs = [None if no_grad[i] else vw['g'][i] for i in range(n)]
    ms = [None if no_grad[i] else vw['m'][i] for i in range(n)]
    vs = [None if no_grad[i] else vw['v'][i] for i in range(n)]
    tab = hip.optim_table(vw['p'], gs, ms, vs, vw['ema'], group_of)
    worst = dict(hip=[0.0, 0.0, 0.0], torch=[0.0, 0.0, 0.0])
    for step in (1, 2, 3):
        _fill(vw['g'], gen, 0.1)
        before = {k: buf[k].clone() for k in buf}
        bv = {k: _views(before[k], lay[k][0]) for k in lay}
        # torch's fused Adam on copies of the same state
        tp = [torch.nn.Parameter(bv['p'][i].clone()) for i in range(n)]
        opt = torch.optim.Adam([dict(params=[tp[i] for i in range(n) if group_of[i] == g and SIZES[i]], **GROUPS[g]) for g in range(4)], fused=True)
        for i in range(n):
            if not no_grad[i] and SIZES[i]:
                tp[i].grad = bv['g'][i].clone()
                opt.state[tp[i]] = dict(step=torch.tensor(float(step - 1), device='cuda'), exp_avg=bv['m'][i].clone(), exp_avg_sq=bv['v'][i].clone())
        opt.step()
        # the kernel
        rows = [(grp['lr'], *grp['betas'], grp['eps'], grp['weight_decay'], step) for grp in GROUPS]
        version = buf['p']._version
        hip.adam_multi(tab, rows, vw['p'] + vw['ema'], EMA_DECAY)
        torch.cuda.synchronize()
        assert buf['p']._version > version
        for k in buf:
            assert _gaps_untouched(buf[k], lay[k][0]), k
        assert torch.equal(_bits(buf['g']), _bits(before['g']))
        for i in range(n):
            if no_grad[i]:
                for k in ('p', 'm', 'v'):
                    assert torch.equal(_bits(vw[k][i]), _bits(bv[k][i])), (k, i)
                continue
            if not SIZES[i]:
                continue
            want = _adam64(bv['p'][i], bv['g'][i], bv['m'][i], bv['v'][i], GROUPS[group_of[i]], step)
            st = opt.state[tp[i]]
            for q, (mine, theirs) in enumerate(((vw['p'][i], tp[i].detach()), (vw['m'][i], st['exp_avg']), (vw['v'][i], st['exp_avg_sq']))):
                dh, dt = _dev(mine, want[q]), _dev(theirs, want[q])
                worst['hip'][q], worst['torch'][q] = max(worst['hip'][q], dh), max(worst['torch'][q], dt)
                if dt == 0.0 and mine.numel():   # torch exact here: within one fp32 ulp of the value, element by element
                    ulp = np.spacing(np.abs(want[q]).astype(np.float32)).astype(np.float64)
                    assert (np.abs(mine.cpu().double().numpy() - want[q]) <= ulp).all(), (step, i, q)
        # the EMA written in the same pass == ema_multi on the new parameters, bit for bit (entries without a gradient included)
        ebuf2 = before['ema'].clone()
        es2 = _views(ebuf2, lay['ema'][0])
        hip.ema_multi(hip.optim_table(vw['p'], emas=es2), EMA_DECAY, es2)
        assert torch.equal(_bits(ebuf2), _bits(buf['ema']))
        assert not torch.equal(_bits(vw['ema'][7]), _bits(bv['ema'][7])) and no_grad[7]   # (1023 elements, no gradient: still averaged)
    print(f'adam_multi {shifts}: max |dev from float64|  p {worst["hip"][0]:.3e} m {worst["hip"][1]:.3e} v {worst["hip"][2]:.3e}   '
          f'torch fused  p {worst["torch"][0]:.3e} m {worst["torch"][1]:.3e} v {worst["torch"][2]:.3e}')
    for q, name in enumerate(('p', 'exp_avg', 'exp_avg_sq')):
        if worst['torch'][q] > 0.0:
            assert worst['hip'][q] <= 2.0 * worst['torch'][q], (name, worst['hip'][q], worst['torch'][q])


def test_adam_multi_refuses_what_it_cannot_do():
    from mrefsr_amd import hip
    p, g, m, v = (torch.zeros(8, device='cuda') for _ in range(4))
    with pytest.raises(ValueError, match='both moments'):
        hip.optim_table([p], [g], [m], None)
    with pytest.raises(ValueError, match='does not match'):
        hip.optim_table([p], [g[:4]], [m], [v])
    with pytest.raises(TypeError):
        hip.optim_table([p], emas=[torch.zeros(8, device='cuda', dtype=torch.float64)])
    with pytest.raises(NotImplementedError, match='no CPU path'):
        hip.optim_table([torch.zeros(8)], emas=[torch.zeros(8)])
    tab = hip.optim_table([p], [g], [m], [v])
    with pytest.raises(ValueError, match='step count'):
        hip.adam_multi(tab, [(1e-3, 0.9, 0.999, 1e-8, 0.0, 0)], [p])
    with pytest.raises(ValueError, match='decay'):
        hip.ema_multi(tab, 1.5, [])
