"""CPU: the host side of the deterministic mode (fixed-order gradient reductions of net_g's backward): the process-wide switch of
mrefsr_amd/hip.py, the model option that turns it on, and the C ABI of the three fixed-order entry points."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DET_EXPORTS = ('mrefsr_act_bwd_det_workspace_bytes', 'mrefsr_act_bwd_nhwc_det_f32', 'mrefsr_dynagg_prep_bwd_blocks',
               'mrefsr_dynagg_prep_bwd_det_workspace_bytes', 'mrefsr_dynagg_prep_bwd_nhwc_det_f32',
               'mrefsr_conv_nhwc_bwd_det_workspace_bytes', 'mrefsr_conv_nhwc_bwd_det_f32')


@pytest.fixture
def switch():
    """the switch and torch's flag as they were, whatever the test does to them"""
    from mrefsr_amd import hip
    before = hip._deterministic[0]
    flag, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    hip.set_deterministic(None)
    torch.use_deterministic_algorithms(False)
    try:
        yield hip
    finally:
        hip.set_deterministic(before)
        torch.use_deterministic_algorithms(flag, warn_only=warn)


def test_switch_is_off_by_default_and_follows_torchs_flag(switch):
    hip = switch
    assert hip._deterministic[0] is None and not hip.is_deterministic()
    torch.use_deterministic_algorithms(True)
    assert hip.is_deterministic()
    torch.use_deterministic_algorithms(False)
    assert not hip.is_deterministic()


def test_an_explicit_setting_overrides_torchs_flag_and_none_follows_it_again(switch):
    hip = switch
    hip.set_deterministic(True)
    assert hip.is_deterministic()
    torch.use_deterministic_algorithms(True)
    hip.set_deterministic(False)
    assert not hip.is_deterministic()
    hip.set_deterministic(None)
    assert hip.is_deterministic()
    with pytest.raises(TypeError):
        hip.set_deterministic(1)


def test_context_manager_nests_and_restores(switch):
    hip = switch
    with hip.deterministic():
        assert hip.is_deterministic()
        with hip.deterministic(False):
            assert not hip.is_deterministic()
            with hip.deterministic(None):
                assert not hip.is_deterministic()      # None: torch's flag, which is off
            assert not hip.is_deterministic()
        assert hip.is_deterministic()
    assert hip._deterministic[0] is None and not hip.is_deterministic()
    with pytest.raises(ZeroDivisionError):
        with hip.deterministic():
            1 / 0
    assert hip._deterministic[0] is None                # restored behind an exception too


def test_alert_raises_like_torch_or_warns_under_warn_only(switch):
    hip = switch
    hip.nondeterministic_alert('op')                    # off: silent
    with hip.deterministic():
        with pytest.raises(RuntimeError, match='op does not have a deterministic implementation'):
            hip.nondeterministic_alert('op')
        torch.use_deterministic_algorithms(True, warn_only=True)
        with pytest.warns(UserWarning, match='does not have a deterministic implementation'):
            hip.nondeterministic_alert('op')


def _bare_model(cls, train):
    """the model class without its networks (they need a GPU): the option parsing is plain Python on self.opt"""
    m = object.__new__(cls)
    m.opt = dict(dist=False, train=train)
    return m


@pytest.mark.parametrize('cls_name', ['MultiRefRestorationModel', 'RefRestorationModel'])
def test_model_reads_train_deterministic_and_the_global_switch(switch, cls_name, monkeypatch):
    hip = switch
    from mrefsr_amd.models import multi_ref_restoration_model as mm
    monkeypatch.delenv('MREFSR_TRAIN_GRAPH', raising=False)
    cls = getattr(mm, cls_name)
    assert not _bare_model(cls, {})._deterministic_wanted()
    assert not _bare_model(cls, {'deterministic': False})._deterministic_wanted()
    assert _bare_model(cls, {'deterministic': True})._deterministic_wanted()
    torch.use_deterministic_algorithms(True)
    assert _bare_model(cls, {})._deterministic_wanted()
    torch.use_deterministic_algorithms(False)
    with hip.deterministic():
        assert _bare_model(cls, {})._deterministic_wanted()
    _bare_model(cls, {'deterministic': True})._check_deterministic_options()       # fine on its own
    _bare_model(cls, {'hip_graph': True})._check_deterministic_options()
    with pytest.raises(ValueError, match='hip_graph'):                              # the pair is refused, neither is dropped
        _bare_model(cls, {'deterministic': True, 'hip_graph': True})._check_deterministic_options()
    torch.use_deterministic_algorithms(True)
    with pytest.raises(ValueError, match='hip_graph'):
        _bare_model(cls, {'hip_graph': True})._check_deterministic_options()


def test_optimize_parameters_runs_the_step_inside_the_mode_and_logs_it_once(switch, caplog):
    hip = switch
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    seen = []

    class Probe(MultiRefRestorationModel):
        def _optimize_parameters(self, step):
            seen.append((step, hip.is_deterministic()))

    with caplog.at_level('INFO', logger='basicsr'):
        m = _bare_model(Probe, {'deterministic': True})
        m.optimize_parameters(1)
        m.optimize_parameters(2)
        off = _bare_model(Probe, {})
        off.optimize_parameters(3)
    assert seen == [(1, True), (2, True), (3, False)]
    assert not hip.is_deterministic()
    assert sum('deterministic training step' in r.getMessage() for r in caplog.records) == 1


def test_header_declares_the_fixed_order_entry_points_and_the_bindings_name_them():
    from mrefsr_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'mrefsr_hip.h')).read()
    for name in DET_EXPORTS:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in _lib.SIGNATURES, name
    # the entry points that take a workspace say how large, and carry a ticket word
    for name in ('mrefsr_act_bwd_nhwc_det_f32', 'mrefsr_dynagg_prep_bwd_nhwc_det_f32', 'mrefsr_conv_nhwc_bwd_det_f32'):
        decl = re.search(r'\b' + name + r'\s*\(([^;]*)\);', text).group(1)
        assert 'void *workspace' in decl and 'int64_t workspace_bytes' in decl and 'uint32_t *ticket' in decl, name
    assert text.count('bitwise reproducible') >= 3
    # the existing entry points keep their signatures
    assert re.search(r'int mrefsr_act_bwd_nhwc_f32\(const float \*g_out, const float \*out, float \*g_pre, int ld_pre, float \*bias_grad, '
                     r'float \*slope_grad, float \*amax,\s*int64_t npix, int C, int act, float slope, const float \*slope_ptr, int \*flag, '
                     r'mrefsr_stream_t stream\);', text)


def test_workspace_sizes_follow_the_launchers_grid_formulas():
    """host-only entry points: the partials workspace is one row per block of the grid the launcher chooses for the shape"""
    from mrefsr_amd import _lib
    lib = _lib.load()
    # act_bwd: 256 / (C / V) pixels per block and pass, 16 passes before another block is added, at most 512 blocks
    for npix, c, blocks in ((7, 64, 1), (1600, 64, 7), (73728, 64, 288), (153664, 64, 512), (7, 3, 1), (9216, 3, 7), (360000, 3, 265)):
        assert lib.mrefsr_act_bwd_blocks(npix, c) == blocks
        assert lib.mrefsr_act_bwd_det_workspace_bytes(npix, c) == blocks * (c + 1) * 4
    # dynagg_prep_bwd_nhwc: tiles of 32 pixels, `groups` = clamp(HW * B / 16384, 1, 32) tiles per block, B block rows
    for b, dg, h, w, blocks in ((1, 8, 1, 31, 1), (2, 8, 40, 41, 104), (2, 8, 96, 96, 576), (2, 1, 160, 160, 534)):
        assert lib.mrefsr_dynagg_prep_bwd_blocks(b, dg, h, w) == blocks
        assert lib.mrefsr_dynagg_prep_bwd_det_workspace_bytes(b, dg, h, w) == blocks * 27 * dg * 4
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.Cout = 2, 48, 48, 64
    assert lib.mrefsr_conv_nhwc_bwd_det_workspace_bytes(d) == 2 * 12 * 2 * 1 * 64 * 4     # 4 x 32 pixel tiles, one cout block
    d.N, d.H, d.W, d.Cout = 1, 16, 70, 128
    assert lib.mrefsr_conv_nhwc_bwd_det_workspace_bytes(d) == 1 * 4 * 3 * 2 * 64 * 4
