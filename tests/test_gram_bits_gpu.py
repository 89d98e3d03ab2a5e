"""GPU: the Gram kernels of the style term and the texture loss give the bits pinned in tests/golden/gram_bits.npz -- the outputs of
tools/kernel_bits.py's gram case list (gram_nhwc, gram_raw_nhwc, gram_bwd_nhwc and texture_gram_bwd_nhwc fresh and accumulated onto
a seeded base, the latter also with norm == 0; N = 2 on C = 64, 3 x 3 and C = 128, 9 x 9), recorded from the library before the two
backward bodies moved into csrc/gram.h; the fixture's `note` says which library that was.  None of these kernels adds floats with an
atomic, so nothing is left out.  After an INTENDED change of the arithmetic, or of the compiler, regenerate the fixture
(tools/README.md)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_bits  # noqa: E402

GOLDEN = np.load(os.path.join(ROOT, 'tests', 'golden', 'gram_bits.npz'))
KEYS = [k for k in GOLDEN.files if k not in ('excluded', 'note')]
SHAPES = [f'c{c}_{h}x{w}' for c, h, w in kernel_bits.GRAM_SHAPES]


@pytest.fixture(scope='module')
def got():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return kernel_bits.flatten(kernel_bits.gram_cases())


def test_fixture_covers_the_case_list_and_leaves_nothing_out():
    assert len(GOLDEN['excluded']) == 0 and kernel_bits.LISTS['gram'] == (kernel_bits.gram_cases, 0)
    assert SHAPES == ['c64_3x3', 'c128_9x9']
    # one Gram matrix; df and max |df| of every backward; the base as well where norm == 0
    want = {f'{name}.{shape}/{i}' for shape in SHAPES for name, n in
            (('gram', 1), ('gram_raw', 1), ('bwd_fresh', 2), ('bwd_acc', 2), ('texture_bwd_fresh', 2), ('texture_bwd_acc', 2), ('texture_bwd_norm0', 3))
            for i in range(n)}
    assert set(KEYS) == want
    for shape in SHAPES:   # norm == 0 onto a base: the pinned library left the base's bits
        assert kernel_bits.same(GOLDEN[f'texture_bwd_norm0.{shape}/0'], GOLDEN[f'texture_bwd_norm0.{shape}/2'])


@pytest.mark.gpu
@pytest.mark.parametrize('key', KEYS)
def test_bits_match_the_pinned_library(got, key):
    assert key in got, f'{key} is pinned but the case list no longer produces it'
    want, have = GOLDEN[key], got[key]
    assert want.shape == have.shape and want.dtype == have.dtype
    assert kernel_bits.same(want, have), \
        f'{key}: bits differ from the pinned library' + ('' if want.dtype == np.uint8 else f' (max |diff| {np.abs(want.astype(np.float64) - have.astype(np.float64)).max()})')
