"""The engine's host-side state on CPU tensors: the one parameter stamp (mrefsr_amd.param_cache), the ring of max |out| words
(hip._AmaxRing), the handles a word travels in (archs/nhwc.py) and the fp16 weight scales of the training step
(nhwc_train._WeightScales)."""
import pytest
import torch

from mrefsr_amd import hip
from mrefsr_amd.archs import nhwc
from mrefsr_amd.param_cache import param_stamp

CPU = torch.device('cpu')
HALF = hip.AMAX_POOL // 2


@pytest.fixture
def ring(monkeypatch):
    """a fresh ring for the CPU device (the words of other tests' tensors die with the old one)"""
    monkeypatch.setattr(hip, '_amax_rings', {})
    return hip.amax_ring(CPU)


def _measured():
    return nhwc.AMAX_MEASURED[0]


def _produced(ring, x):
    """x as an engine launch leaves it: a slot of the ring holding max |x|, attached"""
    slot = hip.amax_slot(CPU)
    assert slot.shape == (1,) and slot.dtype == torch.float32 and float(slot) == 0.0
    slot.fill_(float(x.abs().max()))
    return nhwc.attach_amax(x, slot, ring), slot


# ---- the stamp
def test_stamp_moves_with_version_and_storage_not_with_data_writes_and_reads_dead():
    import weakref
    p = torch.nn.Parameter(torch.ones(4, 3))
    ref, s = weakref.ref(p), param_stamp(p)
    assert s.alive and s == param_stamp(ref()) and s == (True, p.data_ptr(), p._version, None)
    p.data.mul_(3)                       # a write through .data: nothing moves (the inference cache catches it on the device)
    p.data[0, 0] = 7
    assert param_stamp(p) == s
    with torch.no_grad():
        p.mul_(2)                        # an in-place op under no_grad: the version
    s2 = param_stamp(p)
    assert s2 != s and s2.ptr == s.ptr and s2.version > s.version
    p.data = torch.zeros(4, 3)           # a replaced storage: the address
    s3 = param_stamp(p)
    assert s3 != s2 and s3.ptr != s2.ptr
    assert param_stamp(p, epoch=4) != param_stamp(p, epoch=5) and param_stamp(p, epoch=4) == param_stamp(ref(), epoch=4)
    del p
    assert ref() is None and not param_stamp(ref()).alive and param_stamp(ref()) != s3


# ---- the ring and the handles
def test_a_word_is_returned_while_live_and_measured_after_a_reset(ring):
    x = torch.randn(2, 5, 5, 8)
    _, slot = _produced(ring, x)
    before = _measured()
    assert nhwc.amax_word(x) is slot and nhwc.amax_of(x) is slot and _measured() == before
    hip.amax_pool_reset()
    assert nhwc.amax_word(x) is None
    a = nhwc.amax_of(x)
    assert _measured() == before + 1 and a is not slot and float(a) == float(x.abs().max())
    assert hip.amax_slot(CPU).data_ptr() == slot.data_ptr()    # (slot 0 again: another launch's word from here on)
    assert nhwc.amax_of(x) is a and _measured() == before + 1    # measured once


def test_a_word_of_half_0_lives_until_the_counter_re_enters_half_0(ring):
    x = torch.randn(3, 4)
    _, slot = _produced(ring, x)                                 # slot 0
    for _ in range(HALF - 1):
        hip.amax_slot(CPU)
    assert nhwc.amax_word(x) is slot                             # the counter stands at the end of half 0
    y = torch.randn(3, 4)
    _, yslot = _produced(ring, y)                                # the first slot of half 1
    for _ in range(HALF - 1):
        hip.amax_slot(CPU)
    assert nhwc.amax_word(x) is slot and nhwc.amax_word(y) is yslot   # the whole ring handed out once: nothing re-issued yet
    again = hip.amax_slot(CPU)                                   # re-enters half 0: zeroed, its words are other launches' now
    assert again.data_ptr() == slot.data_ptr() and float(slot) == 0.0
    assert nhwc.amax_word(x) is None and nhwc.amax_word(y) is yslot
    before = _measured()
    assert float(nhwc.amax_of(x)) == float(x.abs().max()) and _measured() == before + 1


def test_a_caller_s_tensor_is_measured_once_per_version(ring):
    x = torch.randn(2, 6, 6, 4)
    before = _measured()
    a = nhwc.amax_of(x)
    assert _measured() == before + 1 and float(a) == float(x.abs().max())
    assert nhwc.amax_of(x) is a and _measured() == before + 1
    hip.amax_pool_reset()                                        # a measured word is a tensor of its own: no generation
    assert nhwc.amax_of(x) is a and _measured() == before + 1
    x.mul_(100)
    b = nhwc.amax_of(x)
    assert _measured() == before + 2 and float(b) == float(x.abs().max()) and float(b) > 50 * float(a)
    x.data.mul_(100)                                             # a write through .data moves no version and is NOT seen
    assert nhwc.amax_of(x) is b and _measured() == before + 2


def test_views_and_copies_keep_a_live_word_only(ring):
    x = torch.randn(2, 4, 4, 8)
    _, slot = _produced(ring, x)
    v = nhwc.as_nchw(x)
    assert nhwc.amax_word(v) is slot and nhwc.amax_word(nhwc.to_nhwc(v)) is slot
    hip.amax_pool_reset()
    assert nhwc.amax_word(v) is None and nhwc.amax_word(nhwc.as_nchw(x)) is None


def test_add_attaches_the_bound_at_the_new_version(ring):
    h, x = torch.randn(2, 4, 4, 8), torch.randn(2, 4, 4, 8)
    (_, hs), (_, xs) = _produced(ring, h), _produced(ring, x)
    want = float(hs + xs)
    before = _measured()
    assert nhwc.add_(h, x) is h
    assert float(nhwc.amax_of(h)) == want and want >= float(h.abs().max()) and _measured() == before
    assert nhwc.amax_word(x) is xs
    # one operand without a live word: no bound, the sum is measured when it is read
    h2, x2 = torch.randn(2, 4, 4, 8), torch.randn(2, 4, 4, 8)
    _produced(ring, h2)
    nhwc.add_(h2, x2)
    assert nhwc.amax_word(h2) is None
    assert float(nhwc.amax_of(h2)) == float(h2.abs().max()) and _measured() == before + 1


def test_one_half_guard(ring):
    def take(n):
        for _ in range(n):
            hip.amax_slot(CPU)
    take(100)
    with ring.one_half('train.ldl_opt'):
        take(HALF - 100)                                         # up to the end of the first half: fine
    hip.amax_pool_reset()
    take(100)
    with pytest.raises(RuntimeError) as e:
        with ring.one_half('train.ldl_opt'):
            take(HALF - 99)                                      # one word of the second half
    assert str(e.value) == (f'train.ldl_opt: the forward and the EMA pass took {HALF + 1} max |out| words (the pass from 100 on); a '
                            f'step has {HALF} of them, half of hip.AMAX_POOL = {hip.AMAX_POOL}')
    hip.amax_pool_reset()
    take(hip.AMAX_POOL - 10)                                     # (no reset before the pass: the counter is deep in the ring)
    with pytest.raises(RuntimeError, match='train.x_opt: the forward and the EMA pass took 10 max'):
        with ring.one_half('train.x_opt'):
            take(20)                                             # wraps
    hip.amax_pool_reset()
    with ring.one_half('train.ldl_opt'):
        pass


# ---- the fp16 weight scales of the training step
def test_weight_scales_cache_refusal_under_capture_and_refresh_cadence(monkeypatch):
    from mrefsr_amd.archs import nhwc_train
    scales = nhwc_train._WeightScales()
    monkeypatch.setattr(nhwc_train, '_scales', scales)
    monkeypatch.setattr(hip, '_range_flags', {})
    capturing = [False]
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: capturing[0])
    w, z = torch.nn.Parameter(torch.full((4, 4, 3, 3), 0.75)), torch.nn.Parameter(torch.zeros(4))
    assert not scales.has(w)
    assert scales.get(w) == 2.0 ** 14 and scales.has(w) and scales.epoch == 1        # 0.75 * 2^14 in [2^13, 2^14)
    assert scales.get(z) is None and scales.epoch == 2                                # an all-zero weight has no scale
    assert scales.get(w.detach()) == 2.0 ** 14 and scales.epoch == 2                  # another handle of the same storage
    capturing[0] = True
    assert scales.get(w) == 2.0 ** 14                                                 # cached: no readback, fine under a capture
    with pytest.raises(RuntimeError) as e:
        scales.get(torch.nn.Parameter(torch.ones(2, 2, 1, 1)))
    assert str(e.value) == ('nhwc_train: the fp16 weight scale of a parameter is not cached yet (first use, or its holder was freed) and '
                            'deriving it needs a readback, which a hipGraph capture cannot contain: run one eager step first')
    capturing[0] = False
    flag = hip._range_flag(CPU)
    scales.check()
    assert int(flag) == 0 and scales.checks == 1
    with torch.no_grad():
        w.mul_(8)                                                                     # outgrows the 4x headroom: 6 * 2^14 > 60000
    scales.check()
    assert int(flag) == 1 and scales.get(w) == 2.0 ** 14 and scales.epoch == 2
    scales.checks = nhwc_train.REFRESH - 1
    scales.check()                                                                    # the REFRESH-th check takes all scales afresh
    assert scales.get(w) == 2.0 ** 11 and scales.epoch == 3
    del z
    scales.check()
    assert len(scales.entries) == 1                                                   # a parameter that is gone leaves the cache
    scales.reset()
    assert not scales.has(w) and scales.epoch == 4
