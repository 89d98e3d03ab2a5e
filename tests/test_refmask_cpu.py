"""CPU: per-sample reference masks (mixed reference counts in one batch) -- argument checks of the masked attention entry points,
the host check of `ref_valid`, and the two dataset options that produce absent references."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import make_dataset_files as mk

P = ctypes.c_void_p(8)   # a non-null pointer: every call below is refused before it could be read


def test_masked_entry_points_validate_their_arguments_without_gpu():
    from mrefsr_amd import _lib
    lib = _lib.load()
    # (name, arguments with valid_bits at index vb, index of T, index of c or None)
    calls = {
        'mrefsr_mrattn_fwd_masked_f32': ([P, P, P, P, P, P, 2, 3, 32, 64, 35, 0, None], 3, 7, None),
        'mrefsr_mrattn_bwd_masked_f32': ([P, P, P, P, P, P, P, P, P, 2, 3, 32, 64, 35, 0, None], 5, 10, None),
        'mrefsr_mrattn_fwd_nhwc_masked_f32': ([P, P, P, P, P, 2, 3, 64, 35, 1.0, None], 3, 6, 7),
        'mrefsr_mrattn_fwd_nhwc_masked_bf16': ([P, P, P, P, P, 2, 3, 64, 35, None], 3, 6, 7),
        'mrefsr_mrattn_bwd_nhwc_masked_f32': ([P, P, P, P, P, P, P, P, 2, 3, 64, 35, None], 4, 9, 10),
    }
    for name, (args, vb, t, c) in calls.items():
        fn = getattr(lib, name)
        bad = list(args)
        bad[vb] = None
        assert fn(*bad) != 0 and b'null valid_bits' in lib.mrefsr_last_error(), name
        bad = list(args)
        bad[0] = None
        assert fn(*bad) != 0 and b'null pointer' in lib.mrefsr_last_error(), name
        bad = list(args)
        bad[t] = 17
        assert fn(*bad) != 0 and b'T=17' in lib.mrefsr_last_error(), name
        if c is not None:
            bad = list(args)
            bad[c] = 32
            assert fn(*bad) != 0 and b'c=32' in lib.mrefsr_last_error(), name
    with pytest.raises(_lib.MrefsrHipError):
        _lib.call('mrefsr_mrattn_fwd_nhwc_masked_f32', P, P, P, None, P, 2, 3, 64, 35, ctypes.c_float(1.0), None)


def test_hip_wrappers_refuse_cpu_tensors_and_bad_words():
    from mrefsr_amd import hip
    q, emb, ass = torch.zeros(2, 5, 7, 64), torch.zeros(6, 5, 7, 64), torch.zeros(6, 5, 7, 128)
    vb = torch.tensor([7, 2], dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        hip.mrattn_fwd_nhwc_masked(q, emb, ass, 3, vb)
    with pytest.raises(NotImplementedError):
        hip.mrattn_bwd_nhwc_masked(q, emb, ass, ass[:2], 3, vb)
    with pytest.raises(NotImplementedError):
        hip.mrattn_fwd_masked(q, emb, ass, 3, vb)


def test_host_check_of_ref_valid():
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    check = MultiRefRestorationModel.check_ref_valid
    mask = torch.tensor([[1, 1, 1], [0, 1, 0], [1, 0, 1]], dtype=torch.bool)
    words = check(mask, 3, 3)
    assert words.dtype == torch.int32 and words.tolist() == [7, 2, 5]
    assert torch.equal(check(mask.to(torch.uint8), 3, 3), words)
    assert torch.equal(check(mask.numpy(), 3, 3), words)
    for k in range(16):   # bit t <-> column t
        one = torch.zeros(1, 16, dtype=torch.bool)
        one[0, k] = True
        assert check(one, 1, 16).tolist() == [1 << k]
    assert check(torch.ones(3, 3, dtype=torch.bool), 3, 3) is None
    assert check(torch.ones(3, 3, dtype=torch.uint8), 3, 3) is None
    for bad, b, k in ((mask, 2, 3), (mask, 3, 4), (mask[0], 3, 3), (mask[None], 3, 3), (torch.ones(1, 17, dtype=torch.bool), 1, 17),
                      (mask.float(), 3, 3)):
        with pytest.raises(ValueError):
            check(bad, b, k)
    with pytest.raises(ValueError, match=r'\[1\]'):
        check(torch.tensor([[1, 0], [0, 0]], dtype=torch.bool), 2, 2)


def _cufed_with_gaps(root):
    """make_cufed's two inputs plus a third one; 000 loses references 2 and 5, 001 loses 1: positional lists would misalign"""
    opt = mk.make_cufed(root)
    mk._png(os.path.join(root, '002_0.png'), 'cufed/002/0', 40, 40)
    mk._png(os.path.join(root, '002_3.png'), 'cufed/002/3', 30, 44)
    return opt


def test_cufed_allow_missing_refs_matches_files_by_name(tmp_path):
    from mrefsr_amd.data import build_dataset
    root = str(tmp_path / 'cufed')
    opt = mk.make_cufed(root)
    full = build_dataset(dict(opt))
    whole = [full[i] for i in range(2)]
    assert 'ref_valid' not in whole[0]
    assert sorted(whole[0]) == ['img_in', 'img_in_lq', 'img_in_up', 'img_ref_list', 'img_ref_lq_list', 'img_ref_up_list', 'lq_path',
                                'original_size', 'padding']
    _cufed_with_gaps(root)
    for name in ('000_2.png', '000_5.png', '001_1.png'):
        os.remove(os.path.join(root, name))
    ds = build_dataset(dict(opt, allow_missing_refs=True))
    assert len(ds) == 3
    want_valid = [[1, 0, 1, 1, 0], [0, 1, 1, 1, 1], [0, 0, 1, 0, 0]]
    for i in range(3):
        d = ds[i]
        assert d['ref_valid'].dtype == torch.bool and d['ref_valid'].tolist() == [bool(v) for v in want_valid[i]]
        assert d['img_ref_list'].shape == (5, 3, 500, 500)
        for k in range(5):
            for key in ('img_ref_list', 'img_ref_lq_list', 'img_ref_up_list'):
                if want_valid[i][k] and i < 2:
                    assert torch.equal(d[key][k], whole[i][key][k]), (i, k, key)     # the file of that name, not of that position
                elif not want_valid[i][k]:
                    assert not d[key][k].any(), (i, k, key)
        if i < 2:
            assert d['lq_path'] == whole[i]['lq_path'] and torch.equal(d['img_in'], whole[i]['img_in'])
            assert sorted(set(d) - {'ref_valid'}) == sorted(whole[i])
    # an input without any reference is refused when the dataset is built
    os.remove(os.path.join(root, '002_3.png'))
    with pytest.raises(ValueError, match='002'):
        build_dataset(dict(opt, allow_missing_refs=True))


def _draws_of_today():
    """the random draws MultiRefMegaDepthDataset.__getitem__ makes: random.shuffle of the five references, three of augment"""
    random.shuffle(list(range(5)))
    for _ in range(3):
        random.random()


def test_megadepth_ref_drop_prob(tmp_path):
    from mrefsr_amd.data import build_dataset
    opt = mk.make_megadepth(str(tmp_path / 'mega'))
    off, half, all_ = build_dataset(dict(opt)), build_dataset(dict(opt, ref_drop_prob=0.5)), build_dataset(dict(opt, ref_drop_prob=1.0))
    keys = ['img_in', 'img_in_lq', 'img_in_up', 'img_ref_list', 'img_ref_lq_list', 'img_ref_up_list']
    dropped = 0
    for seed in range(6):
        random.seed(seed)
        want = off[seed % 2]
        state_off = random.getstate()
        random.seed(seed)
        _draws_of_today()
        assert random.getstate() == state_off and sorted(want) == keys          # option off: today's dict, today's draws
        random.seed(seed)
        got = half[seed % 2]
        state_half = random.getstate()
        random.seed(seed)
        _draws_of_today()
        flags = [not (random.random() < 0.5) for _ in range(5)]                 # one draw per reference, after today's
        assert random.getstate() == state_half
        if not any(flags):
            flags[0] = True
        assert sorted(got) == sorted(keys + ['ref_valid']) and got['ref_valid'].tolist() == flags
        for key in ('img_in', 'img_in_lq', 'img_in_up'):
            assert torch.equal(got[key], want[key])
        for k, v in enumerate(flags):
            for key in ('img_ref_list', 'img_ref_lq_list', 'img_ref_up_list'):
                assert torch.equal(got[key][k], want[key][k]) if v else not got[key][k].any(), (seed, k, key)
        dropped += flags.count(False)
        random.seed(seed)
        last = all_[seed % 2]
        assert last['ref_valid'].tolist() == [True, False, False, False, False]      # p = 1: the first reference survives
        assert torch.equal(last['img_ref_list'][0], want['img_ref_list'][0]) and not last['img_ref_list'][1:].any()
    assert dropped > 0
    # the default collate stacks the flags into the [B, K] mask feed_data reads
    from torch.utils.data import default_collate
    batch = default_collate([half[0], half[1]])
    assert batch['ref_valid'].shape == (2, 5) and batch['ref_valid'].dtype == torch.bool
