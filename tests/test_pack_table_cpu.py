"""The training step's table of packed weight copies (archs/nhwc_train: _packed, begin_step, reset_packs, capture_state) on CPU
tensors: the four packing entry points of mrefsr_amd.hip are replaced by fakes that record their calls, the capture state
comes from hip._stream_side, which the tests replace."""
import pytest
import torch

from mrefsr_amd import hip
from mrefsr_amd.archs import nhwc_train


class _Job:
    def __init__(self, weight, wscale):
        self.weight, self.wscale = weight.data_ptr(), wscale


class _Log(list):
    """the calls, and cap[0]: whether hip._stream_side reports a capture"""

    def __init__(self):
        super().__init__()
        self.cap = [False]


@pytest.fixture
def calls(monkeypatch):
    """what the table launched, in order: ('one', job), ('table', jobs), ('multi', n); calls.cap[0] = True reports a capture"""
    log = _Log()
    monkeypatch.setattr(hip, '_stream_side', lambda: (7, log.cap[0]))
    monkeypatch.setattr(hip, '_cap_state', [False, 0])

    def plan(weight, cin_slice=None, terms=6, dgrad=False, wscale=1.0):
        return hip.PackedWeight(torch.zeros(8, dtype=torch.uint8), wscale, terms), _Job(weight, wscale)

    def table(jobs, device):
        log.append(('table', list(jobs)))
        return torch.zeros(max(len(jobs), 1), dtype=torch.uint8)
    monkeypatch.setattr(hip, 'conv_pack_plan', plan)
    monkeypatch.setattr(hip, 'conv_pack_one', lambda job: log.append(('one', job)))
    monkeypatch.setattr(hip, 'conv_pack_table', table)
    monkeypatch.setattr(hip, 'conv_pack_multi', lambda tbl, n: log.append(('multi', n)))
    nhwc_train.reset_packs()
    yield log
    nhwc_train.reset_packs()


def _kinds(log):
    return [c[0] for c in log]


def _w(seed=0):
    return torch.nn.Parameter(torch.full((4, 4, 3, 3), float(seed + 1)))


def test_one_single_pack_at_first_use_then_one_multi_launch_per_step(calls):
    w1, w2 = _w(0), _w(1)
    p1 = nhwc_train._packed(w1, None, 16, wscale=2.0)
    assert _kinds(calls) == ['one'] and calls[0][1].weight == w1.data_ptr()
    assert nhwc_train._packed(w1, None, 16, wscale=2.0) is p1 and _kinds(calls) == ['one']    # unchanged version: no repack
    p1d = nhwc_train._packed(w1, None, 16, dgrad=True, wscale=2.0)
    p2 = nhwc_train._packed(w2, (0, 2), 6)
    assert len({id(p1), id(p1d), id(p2)}) == 3 and _kinds(calls) == ['one'] * 3
    del calls[:]
    nhwc_train.begin_step()
    assert _kinds(calls) == ['table', 'multi'] and len(calls[0][1]) == 3 and calls[1][1] == 3
    nhwc_train.begin_step()
    assert _kinds(calls) == ['table', 'multi', 'multi']                                       # the table is rebuilt only when dirty
    assert nhwc_train._packed(w1, None, 16, wscale=2.0) is p1 and nhwc_train._packed(w2, (0, 2), 6) is p2
    assert _kinds(calls) == ['table', 'multi', 'multi']


def test_a_version_bump_repacks_through_the_table(calls):
    w = _w()
    p = nhwc_train._packed(w, None, 6)
    nhwc_train.begin_step()
    del calls[:]
    with torch.no_grad():
        w.mul_(2)
    assert nhwc_train._packed(w, None, 6) is p and _kinds(calls) == ['multi']   # (a caller without begin_step: the lookup refreshes)
    assert nhwc_train._packed(w, None, 6) is p and _kinds(calls) == ['multi']
    # an entry that is not in the table yet (packed after the last refresh) and has moved: the refresh takes it in
    w2 = _w(1)
    p2 = nhwc_train._packed(w2, None, 6)
    with torch.no_grad():
        w2.mul_(2)
    del calls[:]
    assert nhwc_train._packed(w2, None, 6) is p2 and _kinds(calls) == ['table', 'multi'] and calls[1][1] == 2


def test_an_entry_nobody_asks_for_leaves_the_table(calls):
    w1, w2 = _w(0), _w(1)
    nhwc_train._packed(w1, None, 6), nhwc_train._packed(w2, None, 6)
    for _ in range(nhwc_train._PACK_KEEP + 1):
        nhwc_train.begin_step()
        nhwc_train._packed(w1, None, 6)
    assert [c[1] for c in calls if c[0] == 'multi'] == [2] * (nhwc_train._PACK_KEEP + 1)
    del calls[:]
    nhwc_train.begin_step()                                   # w2 was last asked for more than _PACK_KEEP refreshes ago
    assert _kinds(calls) == ['table', 'multi'] and calls[1][1] == 1 and calls[0][1][0].weight == w1.data_ptr()
    del calls[:]
    nhwc_train._packed(w2, None, 6)
    assert _kinds(calls) == ['one']                           # and is packed anew when it comes back


def test_a_dead_parameter_and_a_replaced_storage_leave_the_table(calls):
    w1, w2, w3 = _w(0), _w(1), _w(2)
    for w in (w1, w2, w3):
        nhwc_train._packed(w, None, 6)
    nhwc_train.begin_step()
    assert calls[-1] == ('multi', 3)
    del w1
    w2.data = torch.ones(4, 4, 3, 3)
    del calls[:]
    nhwc_train.begin_step()
    assert _kinds(calls) == ['table', 'multi'] and calls[1][1] == 1 and calls[0][1][0].weight == w3.data_ptr()


def test_under_a_capture_a_dirty_table_is_not_rebuilt(calls):
    w1, w2 = _w(0), _w(1)
    p1 = nhwc_train._packed(w1, None, 6)
    nhwc_train.begin_step()
    _, before = nhwc_train.capture_state()
    del calls[:]
    calls.cap[0] = True
    nhwc_train.begin_step()
    assert _kinds(calls) == ['multi']                         # a clean table is launched under a capture as anywhere
    assert nhwc_train._packed(w1, None, 6) is p1              # (the capture epoch moved: refreshed by that launch, not again)
    assert _kinds(calls) == ['multi']
    p2 = nhwc_train._packed(w2, None, 6)                      # a new entry: the table is dirty from here on
    assert _kinds(calls) == ['multi', 'one']
    with torch.no_grad():
        w1.mul_(2), w2.mul_(2)
    nhwc_train.begin_step()
    assert _kinds(calls) == ['multi', 'one']                  # no upload inside a capture
    assert nhwc_train._packed(w1, None, 6) is p1 and nhwc_train._packed(w2, None, 6) is p2
    assert _kinds(calls) == ['multi', 'one', 'one', 'one']    # each packed alone
    assert nhwc_train._packed(w1, None, 6) is p1 and len(calls) == 4
    assert nhwc_train.capture_state()[1] == before            # what a graph has baked in has not moved
    calls.cap[0] = False
    del calls[:]
    nhwc_train.begin_step()
    assert _kinds(calls) == ['table', 'multi'] and calls[1][1] == 2


def test_a_copy_at_a_superseded_scale_is_dropped_outside_a_capture_only(calls):
    w = _w()
    nhwc_train._packed(w, None, 16, wscale=2.0)
    nhwc_train._packed(w, None, 16, dgrad=True, wscale=2.0)
    nhwc_train._packed(w, None, 16, wscale=4.0)               # drops the forward copy at 2.0, not the input-gradient one
    del calls[:]
    nhwc_train.begin_step()
    assert sorted((j.wscale for j in calls[0][1])) == [2.0, 4.0] and calls[1] == ('multi', 2)
    calls.cap[0] = True
    nhwc_train._packed(w, None, 16, wscale=8.0)               # under a capture the old copy stays: a graph may read it
    calls.cap[0] = False
    del calls[:]
    nhwc_train.begin_step()
    assert sorted((j.wscale for j in calls[0][1])) == [2.0, 4.0, 8.0] and calls[1] == ('multi', 3)


def test_capture_state_addresses_move_when_the_table_is_rebuilt(calls):
    w1, w2 = _w(0), _w(1)
    p1 = nhwc_train._packed(w1, None, 6)
    nhwc_train.begin_step()
    objs, ptrs = nhwc_train.capture_state()
    assert (p1.data.data_ptr(), w1.data_ptr()) in ptrs
    nhwc_train.begin_step()
    assert nhwc_train.capture_state()[1] == ptrs              # a refresh of a clean table moves nothing
    nhwc_train._packed(w2, None, 6)
    assert nhwc_train.capture_state()[1] == ptrs              # (not before the table has been rebuilt)
    nhwc_train.begin_step()
    _, after = nhwc_train.capture_state()
    assert after != ptrs and (p1.data.data_ptr(), w1.data_ptr()) in after
    assert objs[0][0] is not None and objs[0][0].data_ptr() == ptrs[0]   # the old table is alive as long as its holder
