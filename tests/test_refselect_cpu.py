"""CPU: reference pools (ref_select) -- the option's host check, the pool mask helper with its 32 columns, the two entry points of
csrc/refselect.hip in the library and in _lib.py, their argument checks, and MultiRefCUFEDSet's num_refs."""
import ctypes
import os

import pytest
import torch

import make_dataset_files as mk

P = ctypes.c_void_p(8)   # a non-null pointer: every call below is refused before it could be read


def test_check_ref_select_accepts_the_documented_forms_and_refuses_the_rest():
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    check = MultiRefRestorationModel.check_ref_select
    assert check({}) is None and check(dict(ref_select=None)) is None and check(dict(name='x', val=dict())) is None
    assert check(dict(ref_select=dict(top_k=5))) == (5, 'mean')
    assert check(dict(ref_select=dict(top_k=5, score='mean'))) == (5, 'mean')
    assert check(dict(ref_select=dict(top_k=1, score='wins'))) == (1, 'wins')
    assert check(dict(ref_select=dict(top_k=16))) == (16, 'mean')
    bad = [dict(), dict(score='mean'), dict(top_k=True), dict(top_k=False), dict(top_k=2.0), dict(top_k='5'), dict(top_k=None),
           dict(top_k=0), dict(top_k=-3), dict(top_k=17), dict(top_k=5, score='median'), dict(top_k=5, score=None),
           dict(top_k=5, scores='mean'), dict(top_k=5, score='mean', k=5), 5, True, [5]]
    for rs in bad:
        with pytest.raises(ValueError):
            check(dict(ref_select=rs))


def test_pool_mask_helper_admits_32_columns_and_bit_31():
    from mrefsr_amd.archs.arch_util import ref_pool_words, ref_valid_words
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    check = MultiRefRestorationModel.check_ref_pool_valid
    mask = torch.zeros(3, 32, dtype=torch.bool)
    mask[0, 31] = True
    mask[1, 0] = mask[1, 31] = mask[1, 17] = True
    mask[2, :31] = True
    words = check(mask, 3, 32)
    assert words.dtype == torch.int32 and words.shape == (3,)
    assert [w & 0xffffffff for w in words.tolist()] == [1 << 31, (1 << 31) | (1 << 17) | 1, (1 << 31) - 1]
    assert words[0].item() == -2 ** 31
    assert torch.equal(check(mask.to(torch.uint8), 3, 32), words) and torch.equal(ref_pool_words(mask.numpy()), words)
    for n in range(32):   # bit n <-> column n
        one = torch.zeros(1, 32, dtype=torch.bool)
        one[0, n] = True
        assert check(one, 1, 32).tolist()[0] & 0xffffffff == 1 << n
    assert check(torch.ones(2, 32, dtype=torch.bool), 2, 32) is None
    small = torch.tensor([[1, 1, 1], [0, 1, 0]], dtype=torch.bool)
    assert check(small, 2, 3).tolist() == ref_valid_words(small, 2, 3).tolist() == [7, 2]
    for bad, b, n in ((mask, 2, 32), (mask, 3, 31), (mask[0], 3, 32), (mask[None], 3, 32), (torch.ones(1, 33, dtype=torch.bool), 1, 33),
                      (mask.float(), 3, 32)):
        with pytest.raises(ValueError):
            check(bad, b, n)
    empty = mask.clone()
    empty[1] = False
    with pytest.raises(ValueError, match=r'\[1\]'):
        check(empty, 3, 32)
    # the networks' own masks keep their limit
    with pytest.raises(ValueError):
        ref_valid_words(torch.ones(1, 17, dtype=torch.bool), 1, 17)


def test_library_exports_the_entry_points_with_their_signatures():
    from mrefsr_amd import _lib
    lib = _lib.load()
    for name in ('mrefsr_ref_select_f32', 'mrefsr_ref_gather', 'mrefsr_ref_select_workspace_bytes'):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES['mrefsr_ref_select_f32'][1]) == 13 and len(_lib.SIGNATURES['mrefsr_ref_gather'][1]) == 8
    header = open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'mrefsr_hip.h')).read()
    assert 'int mrefsr_ref_select_f32(' in header and 'int mrefsr_ref_gather(' in header
    # one 4-byte word per (candidate, sample, chunk of 1024 positions)
    ws = lib.mrefsr_ref_select_workspace_bytes
    assert ws(10, 1, 15129) == 4 * 10 * 15 and ws(2, 2, 70001) == 4 * 4 * 69 and ws(1, 1, 1) == 4 and ws(32, 3, 1024) == 4 * 96
    assert ws(32, 3, 1025) == 4 * 96 * 2
    assert ws(0, 1, 1) < 0 and ws(1, 0, 1) < 0 and ws(1, 1, 0) < 0


def test_entry_points_validate_their_arguments_without_gpu():
    from mrefsr_amd import _lib
    lib = _lib.load()
    good = [P, None, P, P, P, 10, 2, 100, 5, 0, P, 1 << 20, None]   # val, valid_bits, scores, sel, slot_bits, N, B, P, K, mode, ws, bytes
    for i, v, msg in ((0, None, b'null pointer'), (2, None, b'null pointer'), (10, None, b'null pointer'), (5, 33, b'N=33'), (5, 0, b'N=0'),
                      (8, 0, b'K=0'), (8, 33, b'K=33'), (6, 0, b'B=0'), (7, 0, b'P=0'), (7, (1 << 24) + 1, b'P='), (9, 2, b'mode 2'),
                      (11, 19, b'workspace')):
        bad = list(good)
        bad[i] = v
        assert lib.mrefsr_ref_select_f32(*bad) != 0 and msg in lib.mrefsr_last_error(), (i, v, lib.mrefsr_last_error())
    good = [P, P, P, 10, 2, 5, 3072, None]   # src, dst, sel, N, B, K, row_bytes
    for i, v, msg in ((0, None, b'null pointer'), (1, None, b'null pointer'), (2, None, b'null pointer'), (3, 33, b'N=33'), (5, 0, b'K=0'),
                      (4, 0, b'B=0'), (6, 0, b'row_bytes=0'), (6, 6, b'row_bytes=6'), (4, 20000, b'B=20000')):
        bad = list(good)
        bad[i] = v
        assert lib.mrefsr_ref_gather(*bad) != 0 and msg in lib.mrefsr_last_error(), (i, v, lib.mrefsr_last_error())
    assert lib.mrefsr_ref_gather(ctypes.c_void_p(10), P, P, 10, 2, 5, 3072, None) != 0 and b'4-byte aligned' in lib.mrefsr_last_error()


def test_hip_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from mrefsr_amd import hip
    val, sel = torch.zeros(4, 2, 10, 10), torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        hip.ref_select(val, None, 2)
    with pytest.raises(NotImplementedError):
        hip.ref_gather(val.view(8, 10, 10), sel, 4)
    with pytest.raises(ValueError):
        hip.ref_select(val, None, 2, score='median')
    with pytest.raises(TypeError):
        hip.ref_gather(val.view(8, 10, 10).half(), sel, 4)


def test_cufed_num_refs_looks_up_a_pool_by_name(tmp_path):
    from mrefsr_amd.data import build_dataset
    root = str(tmp_path / 'cufed')
    opt = mk.make_cufed(root)
    by_name = dict(opt, allow_missing_refs=True)
    # num_refs absent is num_refs: 5, array for array
    five, dflt = build_dataset(dict(by_name, num_refs=5)), build_dataset(dict(by_name))
    whole = []
    for i in range(2):
        a, b = five[i], dflt[i]
        whole.append(a)
        assert sorted(a) == sorted(b)
        for key in a:
            assert torch.equal(a[key], b[key]) if torch.is_tensor(a[key]) else a[key] == b[key], (i, key)
        assert a['img_ref_list'].shape == (5, 3, 500, 500) and a['ref_valid'].tolist() == [True] * 5
    # a pool of 7: 000 has 1..5 and 7, 001 has 1..6 without 3
    mk._png(os.path.join(root, '000_7.png'), 'cufed/000/7', 31, 47)
    mk._png(os.path.join(root, '001_6.png'), 'cufed/001/6', 29, 40)
    os.remove(os.path.join(root, '001_3.png'))
    ds = build_dataset(dict(by_name, num_refs=7))
    want_valid = [[1, 1, 1, 1, 1, 0, 1], [1, 1, 0, 1, 1, 1, 0]]
    for i in range(2):
        d = ds[i]
        assert d['ref_valid'].dtype == torch.bool and d['ref_valid'].tolist() == [bool(v) for v in want_valid[i]]
        for key, side in (('img_ref_list', 500), ('img_ref_lq_list', 125), ('img_ref_up_list', 500)):
            assert d[key].shape == (7, 3, side, side) and d[key].dtype == torch.float32, key
            for k in range(7):
                if not want_valid[i][k]:
                    assert not d[key][k].any(), (i, k, key)
                elif k < 5:
                    assert torch.equal(d[key][k], whole[i][key][k]), (i, k, key)
                else:
                    assert d[key][k].any(), (i, k, key)
        for key in ('img_in', 'img_in_lq', 'img_in_up'):
            assert torch.equal(d[key], whole[i][key])
    from torch.utils.data import default_collate
    batch = default_collate([{k: ds[i][k] for k in ('img_ref_list', 'ref_valid')} for i in range(2)])   # (img_in is not padded)
    assert batch['img_ref_list'].shape == (2, 7, 3, 500, 500) and batch['ref_valid'].shape == (2, 7)
    for bad in (0, 33, True, 2.0, '7'):
        with pytest.raises(ValueError):
            build_dataset(dict(by_name, num_refs=bad))
    with pytest.raises(ValueError):   # positional lists have no pools
        build_dataset(dict(opt, num_refs=7))
