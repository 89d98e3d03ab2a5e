"""The one cache of device scratch in mrefsr_amd.hip (_StreamCache and its three instances) and the capture bookkeeping over it,
on CPU tensors: the stream handle and the capture state come from hip._stream_side, which the tests replace."""
import pytest
import torch

from mrefsr_amd import hip

CPU = torch.device('cpu')
MIB = 1 << 20


@pytest.fixture
def side(monkeypatch):
    """[stream handle, capturing] that hip._stream_side reports; the caches start empty and get their entries back afterwards"""
    state = [7, False]
    monkeypatch.setattr(hip, '_stream_side', lambda: (state[0], state[1]))
    monkeypatch.setattr(hip, '_cap_state', [False, 0])
    saved = [dict(c.entries) for c in hip._caches]
    for c in hip._caches:
        c.entries.clear()
    yield state
    for c, e in zip(hip._caches, saved):
        c.entries.clear()
        c.entries.update(e)


def test_scratch_grows_and_is_kept(side):
    a = hip._scratch(CPU, 100)
    assert a.dtype == torch.uint8 and a.numel() >= MIB            # the floor
    assert hip._scratch(CPU, MIB) is a and hip._scratch(CPU, 1) is a
    b = hip._scratch(CPU, 3 * MIB + 1)
    assert b is not a and b.numel() >= 3 * MIB + 1
    assert hip._scratch(CPU, 100) is b and hip._scratch(CPU, 3 * MIB + 1) is b   # a smaller request gets the grown buffer


def test_scratch_is_keyed_by_stream_and_capture_side(side):
    a = hip._scratch(CPU, 100)
    side[0] = 8
    b = hip._scratch(CPU, 100)
    side[1] = True
    c = hip._scratch(CPU, 100)
    assert len({id(a), id(b), id(c)}) == 3 and len({a.data_ptr(), b.data_ptr(), c.data_ptr()}) == 3
    side[:] = [7, False]
    assert hip._scratch(CPU, 100) is a
    side[:] = [8, True]
    assert hip._scratch(CPU, 100) is c


def test_zeroed_words(side):
    t = hip._zeroed_words(CPU, 'ticket', 1)
    assert t.dtype == torch.int32 and t.shape == (1,) and int(t[0]) == 0
    assert hip._zeroed_words(CPU, 'ticket', 1) is t
    lv = hip._zeroed_words(CPU, 'levels', 48)
    assert lv.shape == (48,) and not lv.any() and hip._zeroed_words(CPU, 'levels', 48) is lv
    assert hip._zeroed_words(CPU, 'levels', 96) is not lv and hip._zeroed_words(CPU, 'ticket', 48) is not lv
    ws, ticket = hip._det_scratch(CPU, 0)
    assert ticket is t and ws is hip._scratch(CPU, 4)
    side[1] = True
    assert hip._zeroed_words(CPU, 'ticket', 1) is not t
    side[:] = [8, False]
    assert hip._zeroed_words(CPU, 'ticket', 1) is not t


def _base(t):
    return t._base if t._base is not None else t


def test_release_and_refs_cover_exactly_the_capture_side(side):
    assert hip.capture_refs() == [] and hip.capture_ptrs() == ()
    eager = [hip._scratch(CPU, 100), hip._zeroed_words(CPU, 'ticket', 1), hip._zeroed_words(CPU, 'levels', 48)]
    ez = hip.zeros_f32(CPU, 5)
    side[0] = 8                      # a second eager stream
    eager += [hip._scratch(CPU, 2 * MIB), hip._zeroed_words(CPU, 'ticket', 1)]
    assert hip.capture_refs() == [] and hip.capture_ptrs() == ()
    side[1] = True                   # the same stream, capturing
    cap = [hip._scratch(CPU, 100), hip._zeroed_words(CPU, 'ticket', 1), hip._zeroed_words(CPU, 'levels', 48)]
    cz = hip.zeros_f32(CPU, 5)
    assert not cz.any() and _base(cz) is not _base(ez)
    cap.append(_base(cz))
    refs = hip.capture_refs()
    assert sorted(map(id, refs)) == sorted(map(id, cap))
    assert hip.capture_ptrs() == tuple(t.data_ptr() for t in refs)
    side[1] = False
    grown = hip._scratch(CPU, 4 * MIB)   # an eager regrowth moves nothing a graph baked in
    assert grown is not eager[3] and sorted(map(id, hip.capture_refs())) == sorted(map(id, cap))
    assert hip.capture_ptrs() == tuple(t.data_ptr() for t in refs)

    hip.release_capture_workspaces()
    assert hip.capture_refs() == [] and hip.capture_ptrs() == ()
    assert all(not k[2] for c in hip._caches for k in c.entries)
    assert hip._scratch(CPU, 100) is grown and hip._zeroed_words(CPU, 'ticket', 1) is eager[4]
    side[0] = 7
    assert hip._scratch(CPU, 100) is eager[0] and hip._zeroed_words(CPU, 'ticket', 1) is eager[1]
    assert hip._zeroed_words(CPU, 'levels', 48) is eager[2]
    assert hip._zero_chunks.entries[hip._zero_chunks.key(CPU)][0] is _base(ez)
    side[:] = [8, True]              # the captured ones are made anew
    assert all(a is not b for a, b in zip((hip._scratch(CPU, 100), hip._zeroed_words(CPU, 'ticket', 1)), cap))


def test_zero_chunks_bump_and_epoch(side):
    a, b = hip.zeros_f32(CPU, 5), hip.zeros_f32(CPU, 200)
    assert _base(a) is _base(b) and b.data_ptr() - a.data_ptr() == 4 * hip._ZALIGN and a.numel() == 5 and b.numel() == 200
    side[1] = True
    assert hip.capture_epoch() == (True, 1)
    c = hip.zeros_f32(CPU, 5)
    side[1] = False
    assert hip.capture_epoch() == (False, 2)
    d = hip.zeros_f32(CPU, 5)        # the capture in between: a fresh eager chunk (the old fill is not replayed with anything)
    assert _base(c) is not _base(a) and _base(d) is not _base(a) and _base(d) is not _base(c)
    assert _base(hip.zeros_f32(CPU, hip._ZCHUNK)) is not _base(d)   # does not fit behind d: the next chunk


def _holds_tensor(v, depth=0):
    if isinstance(v, torch.Tensor):
        return True
    if depth < 4 and isinstance(v, dict):
        return any(_holds_tensor(x, depth + 1) for x in v.values())
    if depth < 4 and isinstance(v, (list, tuple)):
        return any(_holds_tensor(x, depth + 1) for x in v)
    return False


def test_no_cache_of_device_buffers_outside_the_registry(side):
    for name in ('_ws_cache', '_wgrad_ws', '_metrics_ws', '_det_tickets', '_levels_sets', '_workspace', '_wgrad_workspace', '_head_ws',
                 '_conv_ws'):
        assert not hasattr(hip, name), name
    side[1] = True
    hip._det_scratch(CPU, 64), hip._zeroed_words(CPU, 'levels', 48), hip.zeros_f32(CPU, 5)
    assert [type(c) for c in hip._caches] == [hip._StreamCache] * 3 and all(c.entries for c in hip._caches)
    stray = [n for n, v in vars(hip).items() if isinstance(v, dict) and _holds_tensor(v)]
    assert stray == [], stray
