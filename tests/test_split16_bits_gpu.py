"""GPU: the kernels that take their arithmetic from csrc/split16.h give the bits pinned in tests/golden/split16_bits.npz -- the
outputs of tools/kernel_bits.py's case list on the library before the header existed (one case per kernel template with a replaced
site; every scaled case also with amax = 0).  After an INTENDED change of the arithmetic, or of the compiler, regenerate the
fixture (tools/README.md)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_bits  # noqa: E402

GOLDEN = np.load(os.path.join(ROOT, 'tests', 'golden', 'split16_bits.npz'))
KEYS = [k for k in GOLDEN.files if k != 'excluded']


@pytest.fixture(scope='module')
def got():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return kernel_bits.flatten(kernel_bits.cases())


def test_fixture_covers_the_case_list_within_its_exclusions():
    assert len(GOLDEN['excluded']) <= kernel_bits.MAX_EXCLUDED
    names = {k.split('/')[0] for k in KEYS}
    for stem in ('conv3x3_t16', 'conv8_t16', 'conv1x1_t16', 'conv_wino_t17', 'conv_wino4_t17', 'mrattn_blend_conv'):
        assert {f'{stem}.plain', f'{stem}.amax', f'{stem}.amax0'} <= names
    for stem in ('conv_nhwc_bwd', 'dcn_bwd_data', 'dcn_bwd_weight', 'conv_wgrad1x1', 'conv_wgrad3x3'):
        assert {f'{stem}.amax', f'{stem}.amax0'} <= names
    assert {'dcn_fwd_1tile.t16', 'dcn_fwd_1tile.t6', 'dcn_fwd_2tile.t16', 'dcn_fwd_2tile.t6'} <= names


@pytest.mark.gpu
@pytest.mark.parametrize('key', KEYS)
def test_bits_match_the_pinned_library(got, key):
    assert key in got, f'{key} is pinned but the case list no longer produces it'
    want, have = GOLDEN[key], got[key]
    assert want.shape == have.shape and want.dtype == have.dtype
    assert kernel_bits.same(want, have), \
        f'{key}: bits differ from the pinned library' + ('' if want.dtype == np.uint8 else f' (max |diff| {np.abs(want - have).max()})')
