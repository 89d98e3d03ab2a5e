"""GPU: the gradient-norm, finalize, scale and clipped-Adam kernels of csrc/optim.hip on the job table of test_optim_kernels_gpu
(views at odd element offsets into flat buffers; sizes 0, 1, 3, 5, 63, 64, 65, 1023, 1025, 300 001 and 400 x 7; a fifth of the
entries without a gradient; streams that share their offset inside 16 bytes and streams that do not).  Everything between the
views of the gradient buffer -- the gaps and the places of the entries without a gradient -- holds 1e30, whose square overflows:
one such word read would make the norm infinite."""
import types

import numpy as np
import pytest
import torch

from test_optim_kernels_gpu import EMA_DECAY, GROUPS, SHIFTS, SIZES, _adam64, _bits, _fill, _flat, _gaps_untouched, _layout, _views

pytestmark = pytest.mark.gpu

HUGE = 1e30
N = len(SIZES)
GROUP_OF = [i % 4 for i in range(N)]
NO_GRAD = [i % 5 == 2 and i != 9 for i in range(N)]           # (the 300 001-element tensor, index 9, has a gradient)
GRID, CHUNK = 2048, 1024
# The table geometry: job j has ceil((n_j + 3) / 1024) chunks (0 for n = 0), block b of the 2048 takes the chunks
# [T b / 2048, T (b + 1) / 2048) and a lane adds 4 squares per chunk.
T = sum((n + 3 + CHUNK - 1) // CHUNK for n in SIZES if n)
L = 4 * max(T * (b + 1) // GRID - T * b // GRID for b in range(GRID))
# relative error of total_norm: each square one rounding, a lane's L squares L - 1 additions (all terms >= 0: at most L units on
# the sum), everything behind that in double; the square root halves it, its conversion to fp32 adds one: (L + 1) / 2 + 2 covers it
NORM_BOUND = ((L + 1) / 2 + 2) * 2.0 ** -24


def test_table_geometry():
    assert T == 6 + 2 + 2 + 293 + 400 and T < GRID and L == 4   # (fewer chunks than blocks: no block has more than one)


def _state(shifts, seed=11):
    from mrefsr_amd import hip
    sh = SHIFTS[shifts]
    gen = torch.Generator().manual_seed(seed)
    lay = {k: _layout(sh[k]) for k in ('p', 'g', 'm', 'v', 'ema')}
    total = lay['p'][1]
    buf = {k: _flat(total, HUGE if k == 'g' else 12345.0) for k in lay}
    vw = {k: _views(buf[k], lay[k][0]) for k in lay}
    _fill(vw['p'], gen)
    _fill(vw['ema'], gen)
    _fill(vw['m'], gen, 0.01)
    _fill(vw['v'], gen, 0.01)
    for t in vw['v']:
        t.mul_(t)                                             # (exp_avg_sq >= 0)
    with_grad = [vw['g'][i] for i in range(N) if not NO_GRAD[i]]
    _fill(with_grad, gen, 0.1)
    S = types.SimpleNamespace(lay=lay, buf=buf, vw=vw, gen=gen)
    S.gs = [None if NO_GRAD[i] else vw['g'][i] for i in range(N)]
    S.ms = [None if NO_GRAD[i] else vw['m'][i] for i in range(N)]
    S.vs = [None if NO_GRAD[i] else vw['v'][i] for i in range(N)]
    S.tab = hip.optim_table(vw['p'], S.gs, S.ms, S.vs, vw['ema'], GROUP_OF)
    S.clip = hip.GradClipState(buf['p'].device)
    return S


def _norm64(S):
    return float(np.sqrt(sum(float((g.cpu().double() ** 2).sum()) for g in S.gs if g is not None)))


def _read(state):
    torch.cuda.synchronize()
    b = state.buf.cpu()
    return types.SimpleNamespace(total_norm=np.float32(b[0].item()), coef=np.float32(b[1].item()), found_inf=float(b[2]),
                                 skipped=int(state.skipped.item()), bits=_bits(b).clone())


def _coef32(total_norm, max_norm):
    """clip_grad_norm_'s coefficient in fp32 from the kernel's own total_norm (a NaN stays a NaN, as under torch.clamp)"""
    if not max_norm > 0:
        return np.float32(1.0)
    with np.errstate(all='ignore'):
        c = np.float32(max_norm) / (np.float32(total_norm) + np.float32(1e-6))
    return np.float32(1.0) if c > 1 else c


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32), np.asarray(b, dtype=np.float32).view(np.int32))


@pytest.mark.parametrize('shifts', list(SHIFTS), ids=list(SHIFTS))
def test_norm_accuracy_reproducibility_and_coefficient(shifts):
    from mrefsr_amd import hip
    S = _state(shifts)
    assert all(g.data_ptr() % 4 == 0 for g in S.gs if g is not None and g.numel())
    assert len({g.data_ptr() % 16 for g in S.gs if g is not None and g.numel()}) > 1   # every 16-byte phase of a 4-byte aligned start
    want = _norm64(S)
    g0 = S.buf['g'].clone()
    worst = 0.0
    for max_norm in (0.5 * want, 2.0 * want, 0.0, -1.0):
        hip.grad_norm_multi(S.tab, S.clip, max_norm, False)
        a = _read(S.clip)
        ws = S.clip.workspace.clone()
        hip.grad_norm_multi(S.tab, S.clip, max_norm, False)
        b = _read(S.clip)
        assert torch.equal(a.bits, b.bits) and torch.equal(ws.view(torch.int64), S.clip.workspace.view(torch.int64))   # two runs, the same bits
        err = abs(float(a.total_norm) - want) / want
        worst = max(worst, err / NORM_BOUND)
        print(f'grad_norm_multi {shifts} max_norm {max_norm:.4g}: total_norm {a.total_norm!r} float64 {want!r} |rel err| / bound = {err / NORM_BOUND:.3f}'
              f'  coef {a.coef!r}')
        assert np.isfinite(a.total_norm) and err <= NORM_BOUND   # finite: no gap and no entry without a gradient was read (1e30 squared)
        assert _same_bits(a.coef, _coef32(a.total_norm, max_norm)), (max_norm, a.coef)
        assert a.found_inf == 0.0 and a.skipped == 0
    assert _same_bits(_coef32(a.total_norm, 0.5 * want), np.float32(0.5 * want) / (a.total_norm + np.float32(1e-6)))   # (the formula does clip)
    assert float(_coef32(a.total_norm, 0.5 * want)) < 0.51 and float(_coef32(a.total_norm, 2.0 * want)) == 1.0
    assert torch.equal(_bits(S.buf['g']), _bits(g0))           # the gradients are only read
    # the partial sums: one double per block, blocks without chunks write 0 (the workspace starts as garbage)
    S.clip.workspace.fill_(float('nan'))
    hip.grad_norm_multi(S.tab, S.clip, 0.0, False)
    part = S.clip.workspace.cpu().numpy()
    assert np.isfinite(part).all() and int((part == 0).sum()) >= GRID - T
    print(f'grad_norm_multi {shifts}: L = {L}, bound {NORM_BOUND:.3e}, worst |rel err| / bound = {worst:.3f}')


@pytest.mark.parametrize('shifts', list(SHIFTS), ids=list(SHIFTS))
def test_grad_scale_multi_is_one_fp32_product_per_element(shifts):
    from mrefsr_amd import hip
    S = _state(shifts)
    max_norm = 0.5 * _norm64(S)
    hip.grad_norm_multi(S.tab, S.clip, max_norm, False)
    coef = _read(S.clip).coef
    assert 0.49 < float(coef) < 0.51
    before = S.buf['g'].clone()
    version = S.buf['g']._version
    hip.grad_scale_multi(S.tab, S.clip, [g for g in S.gs if g is not None])
    torch.cuda.synchronize()
    assert S.buf['g']._version > version                      # written through raw pointers: the version counter is moved by hand
    want = before.cpu().numpy().copy()
    for i, (o, n) in enumerate(zip(S.lay['g'][0], SIZES)):
        if not NO_GRAD[i]:
            want[o:o + n] = want[o:o + n] * coef               # fl32(g * coef)
    assert _same_bits(S.buf['g'].cpu().numpy(), want)          # gaps and entries without a gradient untouched, the rest bit for bit
    for k in ('p', 'm', 'v', 'ema'):
        assert _gaps_untouched(S.buf[k], S.lay[k][0])


def _torch_twin(S, bv, step, max_norm):
    """clip_grad_norm_ and torch's fused Adam on copies of the state ``bv``"""
    tp = [torch.nn.Parameter(bv['p'][i].clone()) for i in range(N)]
    opt = torch.optim.Adam([dict(params=[tp[i] for i in range(N) if GROUP_OF[i] == g and SIZES[i]], **GROUPS[g]) for g in range(4)], fused=True)
    for i in range(N):
        if not NO_GRAD[i] and SIZES[i]:
            tp[i].grad = bv['g'][i].clone()
            opt.state[tp[i]] = dict(step=torch.tensor(float(step - 1), device='cuda'), exp_avg=bv['m'][i].clone(), exp_avg_sq=bv['v'][i].clone())
    if max_norm:
        torch.nn.utils.clip_grad_norm_([p for p in tp if p.grad is not None], max_norm)
    opt.step()
    return tp, opt


def _check_step(S, bv, coef, step, max_norm, label):
    """the state after one clipped update against float64 Adam on fl32(g * coef) and against clip_grad_norm_ + torch's fused Adam:
    the kernel's largest deviation from float64 may be at most twice torch's (p, exp_avg, exp_avg_sq separately); where torch's is
    0, one fp32 ulp of the value.  Elements that the formula makes non-finite must be non-finite in both."""
    tp, opt = _torch_twin(S, bv, step, max_norm)
    worst = dict(hip=[0.0, 0.0, 0.0], torch=[0.0, 0.0, 0.0])
    for i in range(N):
        if NO_GRAD[i]:
            for k in ('p', 'm', 'v'):
                assert torch.equal(_bits(S.vw[k][i]), _bits(bv[k][i])), (k, i)
            continue
        if not SIZES[i]:
            continue
        with np.errstate(all='ignore'):
            g_eff = torch.from_numpy(bv['g'][i].cpu().numpy() * np.float32(coef))
            want = _adam64(bv['p'][i], g_eff, bv['m'][i], bv['v'][i], GROUPS[GROUP_OF[i]], step)
        st = opt.state[tp[i]]
        for q, (mine, theirs) in enumerate(((S.vw['p'][i], tp[i].detach()), (S.vw['m'][i], st['exp_avg']), (S.vw['v'][i], st['exp_avg_sq']))):
            fin = np.isfinite(want[q])
            mine, theirs = mine.cpu().double().numpy(), theirs.cpu().double().numpy()
            assert np.array_equal(np.isfinite(mine), fin) and np.array_equal(np.isfinite(theirs), fin), (label, i, q)
            if not fin.any():
                continue
            dh, dt = float(np.abs(mine - want[q])[fin].max()), float(np.abs(theirs - want[q])[fin].max())
            worst['hip'][q], worst['torch'][q] = max(worst['hip'][q], dh), max(worst['torch'][q], dt)
            if dt == 0.0:
                ulp = np.spacing(np.abs(want[q][fin]).astype(np.float32)).astype(np.float64)
                assert (np.abs(mine - want[q])[fin] <= ulp).all(), (label, i, q)
    print(f'{label}: max |dev from float64|  p {worst["hip"][0]:.3e} m {worst["hip"][1]:.3e} v {worst["hip"][2]:.3e}   '
          f'clip_grad_norm_ + torch fused  p {worst["torch"][0]:.3e} m {worst["torch"][1]:.3e} v {worst["torch"][2]:.3e}')
    for q, name in enumerate(('p', 'exp_avg', 'exp_avg_sq')):
        if worst['torch'][q] > 0.0:
            assert worst['hip'][q] <= 2.0 * worst['torch'][q], (label, name, worst['hip'][q], worst['torch'][q])


def _snapshot(S):
    before = {k: S.buf[k].clone() for k in S.buf}
    return before, {k: _views(before[k], S.lay[k][0]) for k in S.lay}


def _rows(step):
    return [(grp['lr'], *grp['betas'], grp['eps'], grp['weight_decay'], step) for grp in GROUPS]


def _ema_of(S, before):
    """ema_multi on the EMA buffer of ``before`` and the parameters as they are now"""
    from mrefsr_amd import hip
    ebuf = before['ema'].clone()
    es = _views(ebuf, S.lay['ema'][0])
    hip.ema_multi(hip.optim_table(S.vw['p'], emas=es), EMA_DECAY, es)
    return ebuf


@pytest.mark.parametrize('shifts', list(SHIFTS), ids=list(SHIFTS))
def test_adam_multi_with_clip_against_float64_and_torchs_clip_and_fused_adam(shifts):
    from mrefsr_amd import hip
    S = _state(shifts)
    for step in (1, 2):
        if step > 1:
            _fill([g for g in S.gs if g is not None], S.gen, 0.1)
        max_norm = 0.5 * _norm64(S)
        before, bv = _snapshot(S)
        version = S.buf['p']._version
        hip.grad_norm_multi(S.tab, S.clip, max_norm, False)
        hip.adam_multi(S.tab, _rows(step), S.vw['p'] + S.vw['ema'], EMA_DECAY, clip=S.clip)
        st = _read(S.clip)
        assert S.buf['p']._version > version and 0.49 < float(st.coef) < 0.51
        assert torch.equal(_bits(S.buf['g']), _bits(before['g']))   # g * coef is formed in registers: the gradients keep their bits
        for k in ('p', 'm', 'v', 'ema'):
            assert _gaps_untouched(S.buf[k], S.lay[k][0]), k
        _check_step(S, bv, st.coef, step, max_norm, f'adam_multi clip {shifts} step {step}')
        assert torch.equal(_bits(_ema_of(S, before)), _bits(S.buf['ema']))   # the EMA of the same pass == ema_multi on the new p
    # coef == 1 is multiplied all the same and changes no bit: the unclipped entry point from the same state
    before, bv = _snapshot(S)
    hip.grad_norm_multi(S.tab, S.clip, 0.0, False)
    hip.adam_multi(S.tab, _rows(3), S.vw['p'] + S.vw['ema'], EMA_DECAY, clip=S.clip)
    torch.cuda.synchronize()
    got = {k: S.buf[k].clone() for k in S.buf}
    for k in S.buf:
        S.buf[k].copy_(before[k])
    hip.adam_multi(S.tab, _rows(3), S.vw['p'] + S.vw['ema'], EMA_DECAY)
    torch.cuda.synchronize()
    for k in S.buf:
        assert torch.equal(_bits(got[k]), _bits(S.buf[k])), k


@pytest.mark.parametrize('where', [9, 1], ids=['n300001', 'n1'])
@pytest.mark.parametrize('bad', [float('inf'), float('nan')], ids=['inf', 'nan'])
def test_a_non_finite_gradient(bad, where):
    from mrefsr_amd import hip
    assert SIZES[where] in (300001, 1) and not NO_GRAD[where]
    S = _state('co-aligned')
    max_norm = 0.5 * _norm64(S)
    start, sv = _snapshot(S)
    written = S.vw['p'] + S.vw['ema']
    at = SIZES[where] // 2
    # skipping on: the bad call
    S.vw['g'][where][at] = bad
    hip.grad_norm_multi(S.tab, S.clip, max_norm, True)
    hip.adam_multi(S.tab, _rows(1), written, EMA_DECAY, clip=S.clip, skip=True)
    st = _read(S.clip)
    assert st.found_inf == 1.0 and st.skipped == 1 and not np.isfinite(st.total_norm)
    for k in ('p', 'm', 'v'):
        assert torch.equal(_bits(S.buf[k]), _bits(start[k])), k     # parameters and moments bit for bit
    ema1 = _ema_of(S, start)
    assert torch.equal(_bits(ema1), _bits(S.buf['ema'])) and not torch.equal(_bits(S.buf['ema']), _bits(start['ema']))   # the EMA is still due
    # ... the next, clean call: the host counts 2, the bias corrections are those of step 1
    S.vw['g'][where][at] = sv['g'][where][at]
    hip.grad_norm_multi(S.tab, S.clip, max_norm, True)
    hip.adam_multi(S.tab, _rows(2), written, EMA_DECAY, clip=S.clip, skip=True)
    st = _read(S.clip)
    assert st.found_inf == 0.0 and st.skipped == 1 and np.isfinite(st.total_norm)
    after_skip = {k: S.buf[k].clone() for k in ('p', 'm', 'v')}
    # a run that never saw the bad call
    for k in S.buf:
        S.buf[k].copy_(start[k])
    fresh = hip.GradClipState(S.buf['p'].device)
    hip.grad_norm_multi(S.tab, fresh, max_norm, True)
    hip.adam_multi(S.tab, _rows(1), written, EMA_DECAY, clip=fresh, skip=True)
    assert _read(fresh).skipped == 0
    for k in ('p', 'm', 'v'):
        assert torch.equal(_bits(after_skip[k]), _bits(S.buf[k])), k
        assert not torch.equal(_bits(S.buf[k]), _bits(start[k])), k
    # skipping off: torch's clip and Adam on the same bad gradient (inf: coef 0, the element NaN; NaN: everything NaN)
    for k in S.buf:
        S.buf[k].copy_(start[k])
    S.vw['g'][where][at] = bad
    _, bv = _snapshot(S)
    hip.grad_norm_multi(S.tab, fresh, max_norm, False)
    hip.adam_multi(S.tab, _rows(1), written, EMA_DECAY, clip=fresh)
    st = _read(fresh)
    assert st.found_inf == 1.0 and st.skipped == 0
    assert _same_bits(st.coef, _coef32(st.total_norm, max_norm)) or (np.isnan(st.coef) and np.isnan(_coef32(st.total_norm, max_norm)))
    _check_step(S, bv, st.coef, 1, max_norm, f'non-finite ({bad}) without skipping')
    assert not bool(torch.isfinite(S.vw['p'][where][at]))
