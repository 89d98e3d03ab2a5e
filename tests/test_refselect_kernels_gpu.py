"""GPU: the kernels of csrc/refselect.hip against their statement evaluated in torch on the CPU with fp64 sums.

ref_select.  score 'mean' = (sum_p val[n][b][p]) / P, 'wins' = the number of positions at which n is the present candidate with the
largest val (the lowest n among equal values; a NaN never wins); an absent candidate scores -inf; the present candidates in the
order (score descending, n ascending), a NaN score last; the first min(K, present) of them, emitted in ascending n, -1 behind them;
the mask word has one bit per filled slot.  The inputs of the exact cases are multiples of 2^-10 (or of 2^-2: many ties) in
[-1, 1] with P <= 4096: every fp32 partial sum is a multiple of 2^-10 below 2^12, so it is exact in any order, and the one division
rounds like the fp64 quotient rounded to fp32 (53 >= 2 * 24 + 2 bits).  Scores, selection, words and fillers must EQUAL the oracle.

ref_gather.  out row k B + b = src row sel[b][k] B + b, zeros for -1, nothing written outside the K B rows."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


# ------------------------------------------------------------------------------------------------ the oracle
def _oracle(val, mask, k, mode):
    """val [N,B,P] fp32 (CPU), mask [B,N] bool or None -> (scores fp32 [B,N], sel int32 [B,k], words [B] as unsigned ints)"""
    n, b, p = val.shape
    valid = torch.ones(b, n, dtype=torch.bool) if mask is None else mask
    v = val.double()
    if mode == 'mean':
        s = (v.sum(dim=2) / p).t()
    else:
        eligible = valid.t()[:, :, None] & ~torch.isnan(v)
        x = torch.where(eligible, v, torch.full_like(v, -math.inf))
        is_max = (x == x.max(dim=0).values) & eligible
        first = is_max & (is_max.int().cumsum(0) == 1)
        s = first.sum(dim=2).t().double()
    scores = torch.where(valid, s, torch.full_like(s, -math.inf)).float()
    sel, words = torch.full((b, k), -1, dtype=torch.int32), []
    for i in range(b):
        cand = [j for j in range(n) if valid[i, j]]
        f = [float(x) for x in scores[i]]   # (the score is the fp32 number)
        cand.sort(key=lambda j: (math.isnan(f[j]), 0.0 if math.isnan(f[j]) else -f[j], j))
        keep = sorted(cand[:k])
        sel[i, :len(keep)] = torch.tensor(keep, dtype=torch.int32)
        words.append((1 << len(keep)) - 1)
    return scores, sel, words


def _words_of(mask):
    from mrefsr_amd.archs.arch_util import ref_pool_words
    w = None if mask is None else ref_pool_words(mask)
    return None if w is None else w.to(DEV)


def _same(a, b):
    """equal, NaN where NaN"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def _check(hip, val, mask, k, mode):
    want_scores, want_sel, want_words = _oracle(val, mask, k, mode)
    sel, bits, scores = hip.ref_select(val.to(DEV), _words_of(mask), k, mode)
    assert sel.dtype == torch.int32 and bits.dtype == torch.int32 and scores.dtype == torch.float32
    what = (tuple(val.shape), k, mode, None if mask is None else mask.int().tolist())
    assert _same(scores.cpu(), want_scores), what
    assert torch.equal(sel.cpu(), want_sel), (what, sel.tolist(), want_sel.tolist())
    assert [w & 0xffffffff for w in bits.tolist()] == want_words, what


def _quantised(gen, shape, step):
    q = round(1 / step)
    return torch.randint(-q, q + 1, shape, generator=gen).float() * step


def _masks(gen, b, n):
    """None, and a random mask with at least one candidate per row (N = 32: candidate 31 present in every row, the last row only
    that one and candidate 3)"""
    yield None
    m = torch.rand(b, n, generator=gen) < 0.6
    m[:, int(torch.randint(0, n, (1,), generator=gen))] = True
    if n == 32:
        m[:, 31] = True
        m[-1] = False
        m[-1, 31] = m[-1, 3] = True
    if not bool(m.all()):
        yield m


# ------------------------------------------------------------------------------------------------ ref_select
@pytest.fixture(scope='module')
def hip():
    from mrefsr_amd import hip
    return hip


@pytest.mark.parametrize('n', [1, 2, 5, 17, 32])
@pytest.mark.parametrize('p', [1, 100, 140, 4095])
def test_select_equals_the_oracle_on_exactly_summable_values(hip, p, n):
    gen = torch.Generator().manual_seed(1000 * p + n)
    for b in (1, 3):
        for step in (2.0 ** -10, 0.25):   # (the coarse values tie often: within a position and, at small P, between scores)
            val = _quantised(gen, (n, b, p), step)
            for mask in _masks(gen, b, n):
                for k in sorted({1, max(n - 1, 1), n}):
                    for mode in ('mean', 'wins'):
                        _check(hip, val, mask, k, mode)


@pytest.mark.parametrize('mode', ['mean', 'wins'])
def test_exact_ties_go_to_the_lowest_candidate(hip, mode):
    gen = torch.Generator().manual_seed(7)
    val = _quantised(gen, (5, 2, 100), 2.0 ** -10)
    val[3] = val[1]                       # equal planes: equal means; in 'wins' candidate 1 takes every position the two share
    val[4, 1] = val[0, 1]
    for k in (1, 2, 3, 4):
        _check(hip, val, None, k, mode)
        _check(hip, val, torch.tensor([[0, 1, 1, 1, 1], [1, 1, 0, 1, 1]], dtype=torch.bool), k, mode)
    # all candidates equal everywhere: scores tie (mean) or candidate 0 wins everything (wins); the first k are kept either way
    flat = torch.full((6, 1, 140), 0.5)
    sel, bits, scores = hip.ref_select(flat.to(DEV), None, 3, mode)
    assert sel.tolist() == [[0, 1, 2]] and bits.tolist() == [7]
    assert scores.tolist() == ([[0.5] * 6] if mode == 'mean' else [[140.0, 0, 0, 0, 0, 0]])
    _check(hip, flat, None, 3, mode)
    # equal win counts: candidates 0 and 2 win two positions each, candidate 1 none
    val = torch.tensor([[1.0, 1.0, 0.0, 0.0], [0.5, 0.5, 0.5, 0.5], [0.0, 0.0, 1.0, 1.0]]).view(3, 1, 4)
    _check(hip, val, None, 1, mode)
    _check(hip, val, None, 2, mode)


@pytest.mark.parametrize('mode', ['mean', 'wins'])
def test_fewer_valid_candidates_than_k(hip, mode):
    gen = torch.Generator().manual_seed(11)
    val = _quantised(gen, (6, 3, 140), 2.0 ** -10)
    mask = torch.tensor([[1, 1, 1, 1, 1, 1], [0, 0, 1, 0, 0, 0], [0, 1, 0, 0, 1, 0]], dtype=torch.bool)
    _check(hip, val, mask, 4, mode)
    sel, bits, scores = hip.ref_select(val.to(DEV), _words_of(mask), 4, mode)
    assert sel[1].tolist() == [2, -1, -1, -1] and sel[2].tolist() == [1, 4, -1, -1] and bits.tolist()[1:] == [1, 3] and bits.tolist()[0] == 15
    assert torch.isinf(scores[1, [0, 1, 3, 4, 5]]).all() and (scores[1, [0, 1, 3, 4, 5]] < 0).all()
    # absent planes are never read into a score: NaN filler in them changes nothing
    poisoned = val.clone()
    poisoned[:, 1][~mask[1]] = float('nan')
    again = hip.ref_select(poisoned.to(DEV), _words_of(mask), 4, mode)
    assert torch.equal(again[0], sel) and torch.equal(again[1], bits) and torch.equal(again[2], scores)


@pytest.mark.parametrize('mode', ['mean', 'wins'])
def test_a_nan_plane_ranks_last(hip, mode):
    gen = torch.Generator().manual_seed(13)
    val = _quantised(gen, (4, 2, 100), 2.0 ** -10)
    val[0, 0] = float('nan')       # sample 0: candidate 0, the one every tie would favour
    val[2, 1, 17] = float('nan')   # sample 1: a single NaN in candidate 2
    for k in (1, 2, 3, 4):
        _check(hip, val, None, k, mode)
    sel, _, scores = hip.ref_select(val.to(DEV), None, 3, mode)
    assert sel[0].tolist() == [1, 2, 3]
    if mode == 'mean':
        assert math.isnan(scores[0, 0].item()) and math.isnan(scores[1, 2].item()) and 2 not in sel[1].tolist()
    else:
        assert scores[0, 0].item() == 0 and scores[0, 1:].min().item() > 0


def test_large_p_mean_is_within_the_fp32_sum_bound_and_reproducible(hip):
    p, n, b = 70001, 2, 2
    gen = torch.Generator().manual_seed(17)
    val = torch.rand(n, b, p, generator=gen) * 2 - 1
    dev = val.to(DEV)
    sel, bits, scores = hip.ref_select(dev, None, 1, 'mean')
    again = hip.ref_select(dev, None, 1, 'mean')
    assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip((sel, bits, scores), again))
    want = (val.double().sum(dim=2) / p).t()
    bound = (p - 1) * 2.0 ** -24 * val.double().abs().mean(dim=2).t()
    err = (scores.cpu().double() - want).abs()
    print('large-P mean: max error', err.max().item(), 'bound', bound.min().item())
    assert (err <= bound).all(), (err, bound)
    # the choice follows the scores the kernel returned
    assert sel.cpu().flatten().tolist() == scores.cpu().argmax(dim=1).tolist() and bits.tolist() == [1, 1]
    # 'wins' crosses the same chunk boundaries: exact counts
    _check(hip, val, None, 1, 'wins')
    _check(hip, val, torch.tensor([[1, 1], [0, 1]], dtype=torch.bool), 2, 'wins')


# ------------------------------------------------------------------------------------------------ ref_gather
SENTINEL = 1234.5


def _tables(gen, b, n, k):
    """a full table, one with -1 slots, both [B,k] with ascending candidates per row"""
    full = torch.stack([torch.randperm(n, generator=gen)[:k].sort().values for _ in range(b)]).to(torch.int32)
    holes = full.clone()
    holes[0, k - 1] = -1
    if b > 1 and k > 1:
        holes[b - 1, 1:] = -1
    return [full, holes]


def _gather_oracle(src, sel, n):
    b, k = sel.shape
    rows = src.view(n, b, *src.shape[1:])
    out = torch.zeros((k, b, *src.shape[1:]), dtype=src.dtype)
    for i in range(b):
        for j in range(k):
            if sel[i, j] >= 0:
                out[j, i] = rows[sel[i, j], i]
    return out.view(k * b, *src.shape[1:])


def _same_bits(a, b):
    """a copy keeps every bit pattern: NaN, infinities and -0 included"""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def _gather_case(hip, src, sel, n, misalign=0):
    """src on the CPU; the output goes into the middle of a guard band of sentinel rows"""
    b, k = sel.shape
    want = _gather_oracle(src, sel, n)
    dsrc = src.to(DEV)
    if misalign:   # the same rows at an address that is only 4-byte aligned
        flat = torch.empty(src.numel() + misalign, dtype=src.dtype, device=DEV)
        flat[misalign:] = dsrc.flatten()
        dsrc = flat[misalign:].view(src.shape)
        assert dsrc.data_ptr() % 16 != 0
    fill = SENTINEL if src.dtype == torch.float32 else -77
    band = torch.full((k * b + 3, *src.shape[1:]), fill, dtype=src.dtype, device=DEV)
    out = hip.ref_gather(dsrc, sel.to(DEV), n, out=band[1:])
    assert out.data_ptr() == band[1:].data_ptr()
    got = band.cpu()
    assert _same_bits(got[1:1 + k * b], want), (tuple(src.shape), sel.tolist(), misalign)
    assert (got[0] == fill).all() and (got[1 + k * b:] == fill).all(), 'a row outside the table was written'
    fresh = hip.ref_gather(dsrc, sel.to(DEV), n)
    assert fresh.shape == want.shape and fresh.is_contiguous() and _same_bits(fresh.cpu(), want)
    from mrefsr_amd.archs.nhwc import amax_word
    assert amax_word(fresh) is None   # (not an engine product: no cached max |out| of another tensor)


@pytest.mark.parametrize('shape', [(3, 16, 16), (3, 48, 64), (3, 20, 28)], ids=lambda s: 'x'.join(map(str, s)))
def test_gather_images(hip, shape):
    gen = torch.Generator().manual_seed(sum(shape))
    for b, n, k in ((1, 4, 2), (2, 5, 3), (3, 32, 16)):
        src = torch.randn((n * b, *shape), generator=gen)
        src[0, 0, 0, :4] = torch.tensor([float('nan'), float('inf'), -0.0, -float('inf')])
        for sel in _tables(gen, b, n, k):
            _gather_case(hip, src, sel, n)
    src = torch.randn((4 * 2, *shape), generator=gen)
    for off in (1, 2, 3):   # 4-byte and 8-byte aligned sources
        _gather_case(hip, src, _tables(gen, 2, 4, 2)[1], 4, misalign=off)


def test_gather_match_maps_with_odd_p(hip):
    gen = torch.Generator().manual_seed(35)
    for gh, gw in ((5, 7), (10, 10), (1, 1)):   # P = 35: 8-byte-aligned int64 rows, 4-byte-aligned fp32 rows
        for b, n, k in ((1, 3, 2), (3, 6, 4)):
            idx = torch.randint(0, 1 << 40, (n * b, gh, gw), generator=gen, dtype=torch.int64)
            val = torch.randn((n * b, gh, gw), generator=gen)
            for sel in _tables(gen, b, n, k):
                _gather_case(hip, idx, sel, n)
                _gather_case(hip, val, sel, n)
    # a table entry outside 0..N-1 reads nothing: the slot is zero-filled like a -1
    sel = torch.tensor([[0, 7]], dtype=torch.int32)
    out = hip.ref_gather(torch.ones(3, 5, 7, device=DEV), sel.to(DEV), 3)
    assert out[0].eq(1).all() and out[1].eq(0).all()
