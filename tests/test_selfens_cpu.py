"""CPU: the switch of the x8 geometric self-ensemble (val.self_ensemble) and the refusals of its two kernels' bindings that need
no GPU."""
import ctypes

import pytest
import torch


def test_check_self_ensemble_accepts_absent_none_false_and_true():
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel, RefRestorationModel
    check = MultiRefRestorationModel.check_self_ensemble
    assert RefRestorationModel.check_self_ensemble is check
    assert check(None) is False and check({}) is False and check({'save_img': False}) is False
    assert check({'self_ensemble': None}) is False
    assert check({'self_ensemble': False}) is False
    assert check({'self_ensemble': True}) is True


@pytest.mark.parametrize('value', [1, 8, 'true', [True], 0, 1.0, 'x8'], ids=repr)
def test_check_self_ensemble_refuses_everything_else(value):
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    with pytest.raises(ValueError, match=r'val\.self_ensemble'):
        MultiRefRestorationModel.check_self_ensemble({'self_ensemble': value})


@pytest.mark.parametrize('is_train', [False, True])
def test_constructor_checks_the_option_before_anything_is_built(is_train):
    """training and testing models alike: a bad value is refused although neither of them has touched a network or a device yet"""
    import mrefsr_amd.models.multi_ref_restoration_model as M
    for cls in (M.MultiRefRestorationModel, M.RefRestorationModel):
        with pytest.raises(ValueError, match=r'val\.self_ensemble'):
            cls(dict(is_train=is_train, num_gpu=1, network_map={}, network_extractor={}, network_g={}, path={}, train={},
                     val=dict(self_ensemble=8)))


def test_wrappers_refuse_cpu_tensors():
    from mrefsr_amd import hip
    x = torch.zeros(2, 3, 5, 7)
    for tr in (0, 1):
        with pytest.raises(NotImplementedError):
            hip.dihedral_expand(x, tr)
    with pytest.raises(NotImplementedError):
        hip.dihedral_merge(torch.zeros(4, 3, 5, 7), torch.zeros(4, 3, 7, 5))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """error codes and messages come back before a launch (safe without a device)"""
    from mrefsr_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p
    assert lib.mrefsr_dihedral_expand_f32(None, None, 1, 1, 3, 4, 4, 0, None) != 0 and b'dihedral_expand' in lib.mrefsr_last_error()
    assert lib.mrefsr_dihedral_expand_f32(p(16), p(16), 1, 1, 3, 4, 4, 0, None) != 0          # in place
    assert lib.mrefsr_dihedral_expand_f32(p(16), p(4096), 1, 1, 3, 4, 4, 2, None) != 0        # tr
    assert lib.mrefsr_dihedral_expand_f32(p(16), p(4096), 0, 1, 3, 4, 4, 0, None) != 0        # outer
    assert lib.mrefsr_dihedral_expand_f32(p(16), p(4096), 1, 1, 3, 0, 4, 0, None) != 0        # H
    assert lib.mrefsr_dihedral_expand_f32(p(18), p(4096), 1, 1, 3, 4, 4, 0, None) != 0        # alignment
    assert lib.mrefsr_dihedral_expand_f32(p(16), p(4096), 1, 1, 3, 1 << 16, 1 << 15, 0, None) != 0   # H W > 2^30
    assert lib.mrefsr_dihedral_merge_f32(None, None, None, 1, 3, 4, 4, None) != 0 and b'dihedral_merge' in lib.mrefsr_last_error()
    assert lib.mrefsr_dihedral_merge_f32(p(16), p(4096), p(16), 1, 3, 4, 4, None) != 0        # out is a
    assert lib.mrefsr_dihedral_merge_f32(p(16), p(4096), p(8192), 0, 3, 4, 4, None) != 0      # N
    assert lib.mrefsr_dihedral_merge_f32(p(16), p(4096), p(8192), 1, 3, 4, 0, None) != 0      # W
