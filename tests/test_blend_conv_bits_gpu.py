"""GPU: mrattn_blend_conv_kernel (csrc/mrattn_conv.hip) gives the bits pinned in tests/golden/blend_conv_bits.npz -- the outputs of
tools/kernel_bits.py's `blend_conv` list on the library of the commit before the kernel went to 4-row tiles and two blocks per CU
(8-row tiles, the next pass's tiles carried in registers): the accumulation order of an output (channel chunk, reference group, tap,
term; the blend an fma chain in ascending t) is part of the kernel's contract, its tiling is not.  After an INTENDED change of the
arithmetic, or of the compiler, regenerate the fixture (tools/README.md).  The range flag's launch-level meaning is held here too:
it rises if and only if an in-image value of a PRESENT map leaves the fp16 range after the input scale."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_bits  # noqa: E402

GOLDEN = np.load(os.path.join(ROOT, 'tests', 'golden', 'blend_conv_bits.npz'))
KEYS = [k for k in GOLDEN.files if k not in ('excluded', 'note')]


@pytest.fixture(scope='module')
def runs():
    """the case list, twice"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return kernel_bits.blend_conv_cases(), kernel_bits.blend_conv_cases()


def test_fixture_covers_the_case_list_without_exclusions():
    assert len(GOLDEN['excluded']) == 0 and 'parent' in str(GOLDEN['note'][0])
    names = {k.split('/')[0] for k in KEYS}
    want = set()
    for c in (64, 128, 256):
        for h, w in kernel_bits.BLEND_MAPS:
            for tag in ('t5', 't5_masked') + (('t7',) if c == 64 else ()):
                want |= {f'c{c}_{h}x{w}_{tag}.{var}' for var in ('plain', 'amax', 'amax0')}
    assert names == want and len(KEYS) == len(want)


@pytest.mark.gpu
@pytest.mark.parametrize('key', KEYS)
def test_bits_match_the_pinned_library(runs, key):
    got = kernel_bits.flatten(runs[0])
    assert key in got, f'{key} is pinned but the case list no longer produces it'
    want, have = GOLDEN[key], got[key]
    assert want.shape == have.shape and want.dtype == have.dtype
    if want.dtype != np.uint8:
        print(f'{key}: max |diff| {np.abs(want - have).max()}')
    assert kernel_bits.same(want, have), f'{key}: bits differ from the pinned library'


@pytest.mark.gpu
def test_two_launches_give_the_same_bits(runs):
    a, b = runs
    assert list(a) == list(b)
    for name in a:
        assert kernel_bits.same(a[name][0], b[name][0]), name


@pytest.mark.gpu
def test_the_sample_without_a_present_reference_is_exact_zeros(runs):
    masked = [name for name in runs[0] if '_masked.' in name]
    assert len(masked) == 27
    for name in masked:
        y = runs[0][name][0]
        assert not y[1].any(), name
        assert y[0].any(), name


@pytest.mark.gpu
def test_range_flag_means_a_present_in_image_value_outside_fp16():
    import torch
    from mrefsr_amd import hip
    c, t, (h, w) = 64, 5, kernel_bits.BLEND_MAPS[1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    wt, bias = kernel_bits.blend_weights(c)
    pk, bias_d = hip.conv_pack_weight(dev(wt), 16), dev(bias)
    rng = np.random.default_rng(7)
    base = rng.standard_normal((t * 2, h, w, c)).astype(np.float32)
    _, prob = kernel_bits.blend_inputs(8, c, t, h, w)
    present = np.array([[(m >> k) & 1 for k in range(t)] for m in kernel_bits.BLEND_MASK], np.float32)
    prob_m, vb = dev(prob * present[:, None, None, :]), dev(np.array(kernel_bits.BLEND_MASK, np.int32))
    prob_d = dev(prob)

    def tripped(refs, prob_, vb_=None, amax=False):
        hip.conv_range_tripped(reset=True)
        r = dev(refs)
        hip.mrattn_blend_conv(r, prob_, pk, bias_d, t, vb_, in_amax=r.abs().amax().reshape(1) if amax else None)
        return bool(hip.conv_range_tripped(reset=True))

    assert not tripped(base, prob_d)
    # (map index t * 2 + sample: reference 3 of sample 1 / reference 4 of sample 0 -- present under the mask too -- / reference 0)
    corner, last_col, absent = base.copy(), base.copy(), base.copy()
    corner[3 * 2 + 1, h - 1, w - 1, c - 1] = 1e5
    last_col[4 * 2 + 0, 5, w - 1, 17] = -1e5
    absent[0 * 2 + 0, 0, 0, 0] = absent[0 * 2 + 0, 5, w - 1, 17] = 1e5     # reference 0 is absent from sample 0 under BLEND_MASK
    absent[2 * 2 + 1, h - 1, w - 1, c - 1] = 1e5                           # sample 1 has no reference at all
    assert tripped(corner, prob_d), 'a single 1e5 at an image corner'
    first = base.copy()
    first[0, 0, 0, 0] = 1e5
    assert tripped(first, prob_d), 'a single 1e5 at the first pixel'
    assert tripped(last_col, prob_d), 'a single 1e5 in the last (ragged) column'
    assert tripped(last_col, prob_m, vb), 'the same under a mask that keeps its map'
    assert tripped(absent, prob_d), 'the values trip the flag where their maps are present'
    assert not tripped(absent, prob_m, vb), 'values of absent maps are never read'
    for refs in (corner, first, last_col):
        assert not tripped(refs, prob_d, amax=True), 'scaled by the tensor\'s power of two: inside fp16'
