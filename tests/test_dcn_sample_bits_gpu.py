"""GPU: the DCN kernel paths that sample through csrc/dcn_sample.h give the bits pinned in tests/golden/dcn_sample_bits.npz -- the
outputs of tools/kernel_bits.py's dcn_sample case list (the paths tests/golden/split16_bits.npz does not reach: the portable fp32
forward / im2col / col2im, the fp32-MFMA kernel with the NCHW gather, the one-tile kernel at Co = 256, the paired and eight-channel
gathers, bf16 arithmetic, the fused backward at 16 and 32 channels per group, float64 and float16) on the lattice and heavy_tail
fields, recorded from the library before the header existed; the fixture's `note` says which entries another library recorded.
grad_x of dcn_col2im / dcn_bwd_data (float atomics) is not part of the list.  After an INTENDED change of the arithmetic, or of the
compiler, regenerate the fixture (tools/README.md)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_bits  # noqa: E402

GOLDEN = np.load(os.path.join(ROOT, 'tests', 'golden', 'dcn_sample_bits.npz'))
KEYS = [k for k in GOLDEN.files if k not in ('excluded', 'note')]


@pytest.fixture(scope='module')
def got():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return kernel_bits.flatten(kernel_bits.dcn_sample_cases())


def test_fixture_covers_the_case_list_and_leaves_nothing_out():
    assert len(GOLDEN['excluded']) == 0
    names = {k.split('/')[0] for k in KEYS}
    stems = ['fwd_portable_g8_dg4', 'fwd_portable_g8_4_dg2_groups2_stride2', 'fwd_portable_g12_20_dg3_dil2', 'columns_f32_mask',
             'columns_f32_nomask', 'fwd_mfma_nchw_gather', 'fwd_one_tile_c256', 'fwd_pt_paired_c128', 'fwd_pt_map8_c128_64',
             'fwd_bf16_arith_f32_storage', 'fwd_bf16_arith_bf16_storage', 'bwd_data_cpg16', 'bwd_data_cpg32', 'fwd_f64', 'columns_f64',
             'fwd_f16', 'columns_f16']
    for stem in stems:
        assert {f'{stem}.lattice', f'{stem}.heavy_tail'} <= names
    # columns, grad_offset, grad_mask (none without a mask); grad_offset, grad_mask of the fused backward
    for stem, n in (('columns_f32_mask', 3), ('columns_f32_nomask', 2), ('columns_f64', 3), ('columns_f16', 3), ('bwd_data_cpg16', 2), ('bwd_data_cpg32', 2)):
        for tag in ('lattice', 'heavy_tail'):
            assert {f'{stem}.{tag}/{i}' for i in range(n)} <= set(KEYS)


@pytest.mark.gpu
@pytest.mark.parametrize('key', KEYS)
def test_bits_match_the_pinned_library(got, key):
    assert key in got, f'{key} is pinned but the case list no longer produces it'
    want, have = GOLDEN[key], got[key]
    assert want.shape == have.shape and want.dtype == have.dtype
    assert kernel_bits.same(want, have), \
        f'{key}: bits differ from the pinned library' + ('' if want.dtype == np.uint8 else f' (max |diff| {np.abs(want.astype(np.float64) - have.astype(np.float64)).max()})')
