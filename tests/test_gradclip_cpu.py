"""CPU: the host side of gradient-norm clipping and non-finite step skipping -- the C ABI added to csrc/optim.hip, the refusals of
train.grad_clip_norm_g / train.grad_clip_norm_d / train.skip_nonfinite_steps, and HipAdam folding the device's count of skipped
steps into its state dict (the kernels replaced by a stand-in that keeps the count on the host)."""
import copy
import ctypes
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_signatures_and_the_state_struct():
    from mrefsr_amd import _lib
    _vp, _i, _f, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
    want = {
        'mrefsr_grad_norm_workspace_bytes': (_i64, []),
        'mrefsr_grad_sqnorm_multi_f32': (_i, [_vp, _i, _vp, _i64, _vp]),
        'mrefsr_grad_norm_finalize_f32': (_i, [_vp, _i64, _f, _i, _vp, _vp]),
        'mrefsr_grad_scale_multi_f32': (_i, [_vp, _i, _vp, _vp]),
        'mrefsr_adam_multi_clip_f32': (_i, [_vp, _i, _vp, _i, _f, _f, _vp, _i, _vp]),
    }
    header = open(os.path.join(ROOT, 'include', 'mrefsr_hip.h')).read()
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        assert name in header, name
    assert 'mrefsr_grad_clip_state' in header and 'overflows' in header   # (an overflowing square counts as non-finite: said there)
    # four floats (total_norm, coef, found_inf, reserved) and an int64 at offset 16
    S = _lib.GradClipState
    assert ctypes.sizeof(S) == 24 and [f for f, _ in S._fields_] == ['total_norm', 'coef', 'found_inf', 'reserved', 'skipped']
    assert S.found_inf.offset == 8 and S.skipped.offset == 16
    lib = _lib.load()   # (binds every symbol: a missing export raises)
    assert lib.mrefsr_grad_norm_workspace_bytes() == 2048 * 8   # one double per block of the fixed grid
    # argument validation happens before any launch
    assert lib.mrefsr_grad_sqnorm_multi_f32(None, 0, None, 0, None) != 0
    assert lib.mrefsr_grad_norm_finalize_f32(None, 0, 1.0, 0, None, None) != 0
    assert lib.mrefsr_grad_scale_multi_f32(None, 0, None, None) != 0
    assert lib.mrefsr_adam_multi_clip_f32(None, 0, None, 0, 0.0, 1.0, None, 0, None) != 0


def _bare(cls_name, train):
    from mrefsr_amd.models import multi_ref_restoration_model as M
    m = object.__new__(getattr(M, cls_name))
    m.opt = dict(dist=False, train=train)
    return m


@pytest.mark.parametrize('cls_name', ['MultiRefRestorationModel', 'RefRestorationModel'])
def test_the_three_refusals(cls_name, monkeypatch):
    monkeypatch.delenv('MREFSR_TRAIN_GRAPH', raising=False)
    for train in ({'grad_clip_norm_g': 1.0}, {'grad_clip_norm_d': 0.5, 'grad_clip_norm_g': 10}, {'skip_nonfinite_steps': True},
                  {'skip_nonfinite_steps': True, 'fused_adam': True}, {'skip_nonfinite_steps': True, 'fused_adam': False, 'hip_adam': True},
                  {'skip_nonfinite_steps': False, 'fused_adam': False}, {'grad_clip_norm_g': 1.0, 'fused_adam': False},
                  {'skip_nonfinite_steps': False, 'hip_graph': True}):
        _bare(cls_name, train)._check_update_options()
    # 1. not with the hipGraph replay of the training step
    for k, v in (('grad_clip_norm_g', 1.0), ('grad_clip_norm_d', 1.0), ('skip_nonfinite_steps', True)):
        with pytest.raises(ValueError, match=f'{k}.*hip_graph'):
            _bare(cls_name, {k: v, 'hip_graph': True})._check_update_options()
        monkeypatch.setenv('MREFSR_TRAIN_GRAPH', '1')
        with pytest.raises(ValueError, match=f'{k}.*hip_graph'):
            _bare(cls_name, {k: v})._check_update_options()
        monkeypatch.delenv('MREFSR_TRAIN_GRAPH')
    # 2. a clip value that is not a finite number above 0
    for k in ('grad_clip_norm_g', 'grad_clip_norm_d'):
        for bad in (0, 0.0, -1.0, float('inf'), float('nan'), True, '1.0'):
            with pytest.raises(ValueError, match=k):
                _bare(cls_name, {k: bad})._check_update_options()
    # 3. torch's non-fused Adam has no found_inf
    with pytest.raises(ValueError, match='skip_nonfinite_steps.*fused_adam'):
        _bare(cls_name, {'skip_nonfinite_steps': True, 'fused_adam': False})._check_update_options()
    with pytest.raises(ValueError, match='skip_nonfinite_steps.*fused_adam'):
        _bare(cls_name, {'skip_nonfinite_steps': True, 'fused_adam': False, 'hip_adam': False})._check_update_options()


def test_constructor_refuses_before_any_optimizer_exists(monkeypatch):
    from mrefsr_amd.models import multi_ref_restoration_model as M
    monkeypatch.delenv('MREFSR_TRAIN_GRAPH', raising=False)
    monkeypatch.setattr(M, 'build_network', lambda o: torch.nn.Conv2d(3, 4, 3))
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(torch.nn.Module, 'to', lambda self, *a, **k: self)
    for train, match in ((dict(hip_graph=True, grad_clip_norm_g=1.0), 'hip_graph'), (dict(grad_clip_norm_d=-2.0), 'grad_clip_norm_d'),
                         (dict(skip_nonfinite_steps=True, fused_adam=False), 'fused_adam')):
        with pytest.raises(ValueError, match=match):
            M.MultiRefRestorationModel(dict(is_train=True, num_gpu=1, network_map={}, network_extractor={}, network_g={}, path={}, train=train))


def test_hip_adam_refuses_a_bad_clip_value():
    from mrefsr_amd.optim import HipAdam
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='max_grad_norm'):
            HipAdam([torch.nn.Parameter(torch.zeros(1))], max_grad_norm=bad)
    opt = HipAdam([torch.nn.Parameter(torch.zeros(1))], max_grad_norm=2.5, skip_nonfinite=True)
    assert opt.max_grad_norm == 2.5 and opt.skip_nonfinite is True and opt.clip_state is None
    assert type(opt).state_dict is torch.optim.Adam.state_dict   # the folding is a pre-hook: the method stays torch's


class _FakeHip:
    """mrefsr_amd.hip as far as HipAdam.step uses it, on the host: the table and the Adam kernel do nothing, grad_norm_multi does
    what the finalize launch does to ``skipped`` (one more when skipping is asked for and a gradient is not finite)"""

    def __init__(self):
        self.calls = []

    class GradClipState:
        def __init__(self, device):
            self.skipped = torch.zeros((), dtype=torch.int64)

    def optim_table(self, ps, gs=None, ms=None, vs=None, emas=None, groups=None, cached=None):
        self.gs = gs
        return types.SimpleNamespace(table=torch.zeros(1))

    def grad_norm_multi(self, tab, state, max_norm, skip):
        bad = any(g is not None and not bool(torch.isfinite(g).all()) for g in self.gs)
        if bad and skip:
            state.skipped += 1
        self.calls.append(('norm', max_norm, skip))

    def adam_multi(self, tab, groups, written, ema_decay=0.0, clip=None, skip=False):
        self.calls.append(('adam', sorted({int(g[5]) for g in groups}), clip, skip))   # (the step counts of the rows)

    def ema_multi(self, *a):
        raise AssertionError('every step of this test has gradients')


def test_hip_adam_state_dict_folds_the_skipped_steps(monkeypatch):
    from mrefsr_amd import optim
    fake = _FakeHip()
    monkeypatch.setattr(optim, 'hip', fake)
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (5, 7, 3)]
    opt = optim.HipAdam([{'params': ps[:2]}, {'params': ps[2:], 'lr': 1e-5}], lr=1e-4, max_grad_norm=1.0, skip_nonfinite=True)

    def step(poison=False, who=ps):
        for p in ps:
            p.grad = None
        for p in who:
            p.grad = torch.randn_like(p)
        if poison:
            who[0].grad[0] = float('inf')
        opt.step()

    step()
    step(poison=True)
    step()
    step(poison=True)
    assert [c for c in fake.calls if c[0] == 'norm'] == [('norm', 1.0, True)] * 4
    adam = [c for c in fake.calls if c[0] == 'adam']
    assert [c[1] for c in adam] == [[1], [2], [3], [4]]            # the host counts on: the kernel subtracts the device's count
    assert all(c[2] is opt.clip_state and c[3] is True for c in adam)
    assert int(opt.clip_state.skipped) == 2 and opt.skipped_folded == 0
    assert all(float(opt.state[p]['step']) == 4.0 for p in ps)     # (before the fold)
    sd = opt.state_dict()
    assert all(float(s['step']) == 2.0 for s in sd['state'].values())   # the steps really taken
    assert int(opt.clip_state.skipped) == 0 and opt.skipped_folded == 2
    assert all(float(s['step']) == 2.0 for s in opt.state_dict()['state'].values())   # nothing is folded twice
    step()
    assert [c for c in fake.calls if c[0] == 'adam'][-1][1] == [3]
    # a parameter sits out while steps are skipped: the count so far is folded before another set of parameters steps
    step(poison=True)                                              # host 4, device 1
    step(who=ps[:2])                                               # folds first: ps[0:2] at 3 + 1, ps[2] stays at 3
    assert int(opt.clip_state.skipped) == 0 and opt.skipped_folded == 3
    assert [c for c in fake.calls if c[0] == 'adam'][-1][1] == [4]
    assert [float(opt.state[p]['step']) for p in ps] == [4.0, 4.0, 3.0]
    step()                                                         # all three again: two rows, 5 and 4
    assert [c for c in fake.calls if c[0] == 'adam'][-1][1] == [4, 5]
    # the saved state loads into torch's Adam, which goes on from the true counts, and back
    sd = copy.deepcopy(opt.state_dict())
    assert [float(sd['state'][i]['step']) for i in range(3)] == [5.0, 5.0, 4.0]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    back = torch.optim.Adam([{'params': qs[:2]}, {'params': qs[2:], 'lr': 1e-5}], lr=1e-4)
    back.load_state_dict(sd)
    for q in qs:
        q.grad = torch.ones_like(q)
    back.step()
    assert [float(back.state[q]['step']) for q in qs] == [6.0, 6.0, 5.0]
    step(poison=True)                                              # device 1 again ...
    opt.load_state_dict(copy.deepcopy(back.state_dict()))         # ... and gone before the loaded counters are adopted
    assert int(opt.clip_state.skipped) == 0 and opt.skipped_folded == 4
    step()
    assert [c for c in fake.calls if c[0] == 'adam'][-1][1] == [6, 7]
    assert [float(opt.state[p]['step']) for p in ps] == [7.0, 7.0, 6.0]
