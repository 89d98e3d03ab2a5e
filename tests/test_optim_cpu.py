"""CPU: the host side of the parameter update -- the C ABI of csrc/optim.hip, CosineAnnealingRestartLR against the reference's
learning rates (tests/golden/optim_ema.npz), load_network's param_key with its fallback, the options train.ema_decay /
train.hip_adam against train.hip_graph, and HipAdam's state dict in torch's layout."""
import copy
import ctypes
import json
import logging
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_ctypes_signatures():
    from mrefsr_amd import _lib
    _vp, _i, _f, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
    assert _lib.SIGNATURES['mrefsr_ema_multi_f32'] == (_i, [_vp, _i, _f, _f, _vp])
    assert _lib.SIGNATURES['mrefsr_adam_multi_f32'] == (_i, [_vp, _i, _vp, _i, _f, _f, _vp])
    assert _lib.SIGNATURES['mrefsr_optim_job_chunks'] == (_i, [_i64])
    # the structs of include/mrefsr_hip.h: five pointers, int64 n, two int32 / five doubles and an int64
    assert ctypes.sizeof(_lib.OptimJob) == 56 and [f for f, _ in _lib.OptimJob._fields_] == ['p', 'g', 'm', 'v', 'ema', 'n', 'first_chunk', 'group']
    assert ctypes.sizeof(_lib.AdamGroup) == 48 and [f for f, _ in _lib.AdamGroup._fields_] == ['lr', 'beta1', 'beta2', 'eps', 'weight_decay', 'step']
    header = open(os.path.join(ROOT, 'include', 'mrefsr_hip.h')).read()
    for name in ('mrefsr_ema_multi_f32', 'mrefsr_adam_multi_f32', 'mrefsr_optim_job_chunks', 'mrefsr_optim_job', 'mrefsr_adam_group'):
        assert name in header
    lib = _lib.load()   # (binds every symbol: a missing export raises)
    # chunks of 1024 elements, three spare for a tensor that starts up to three words behind a 16-byte boundary
    assert [lib.mrefsr_optim_job_chunks(n) for n in (0, 1, 1021, 1022, 2045, 2046, 300001)] == [0, 1, 1, 2, 2, 3, 293]
    assert lib.mrefsr_optim_job_chunks(-1) == -1


def test_cosine_annealing_restart_lr_reproduces_the_reference(golden):
    from mrefsr_amd.models.multi_ref_restoration_model import _CosineAnnealingRestartLR
    g = golden('optim_ema')
    note = json.loads(str(g['settings']))
    assert len(note['settings']) == 2
    for i, kw in enumerate(note['settings']):
        want = g[f'lr_{i}']
        assert want.shape == (note['iters'] + 1, len(note['base_lrs'])) and want.dtype == np.float64
        params = [torch.nn.Parameter(torch.zeros(1)) for _ in note['base_lrs']]
        opt = torch.optim.Adam([{'params': [p], 'lr': lr} for p, lr in zip(params, note['base_lrs'])])
        sched = _CosineAnnealingRestartLR(opt, **kw)
        got = [[pg['lr'] for pg in opt.param_groups]]
        for _ in range(note['iters']):
            opt.step()
            sched.step()
            got.append([pg['lr'] for pg in opt.param_groups])
        got = np.asarray(got, dtype=np.float64)
        err = np.abs(got - want)                              # rel <= 1e-12 (stated without a division: eta_min 0 is reached exactly)
        assert (err <= 1e-12 * np.abs(want)).all(), (i, err.max())
        assert want.min() < 0.2 * want.max()   # (the fixture does anneal and restart: not a constant rate)


def _bare(train, **opt):
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    m = object.__new__(MultiRefRestorationModel)
    m.opt = dict(dist=False, train=train, **opt)
    m.device = torch.device('cpu')
    return m


def test_model_accepts_the_cosine_scheduler():
    m = _bare(dict(pixel_criterion='L1Loss', pixel_weight=1.0, net_g_pretrain_steps=0,
                   scheduler=dict(type='CosineAnnealingRestartLR', periods=[10, 10], restart_weights=[1, 0.5], eta_min=1e-7)))
    p = torch.nn.Parameter(torch.zeros(1))
    m.optimizers, m.schedulers = [torch.optim.Adam([p], lr=1e-4)], []
    m.init_training_settings()
    assert type(m.schedulers[0]).__name__ == '_CosineAnnealingRestartLR' and m.schedulers[0].periods == [10, 10]


def _net(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.PReLU(), torch.nn.Conv2d(4, 2, 1))


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


def test_load_network_param_key_and_fallback(tmp_path, caplog):
    m = _bare({})
    params, ema = _net(1), _net(2)
    both, only = str(tmp_path / 'both.pth'), str(tmp_path / 'only.pth')
    m.save_network([params, ema], both, param_key=['params', 'params_ema'])
    m.save_network(params, only)
    assert sorted(torch.load(both)) == ['params', 'params_ema'] and sorted(torch.load(only)) == ['params']
    net = _net(3)
    m.load_network(net, both)                                # the default key stays params
    assert _same(net, params) and not _same(net, ema)
    with caplog.at_level(logging.INFO, logger='basicsr'):
        m.load_network(net, both, True, 'params_ema')
        assert _same(net, ema)
        assert 'with param key: [params_ema]' in caplog.text and 'does not exist' not in caplog.text
        caplog.clear()
        net = _net(3)
        m.load_network(net, only, True, 'params_ema')        # a checkpoint without an EMA: params, and the reference's log line
        assert _same(net, params)
        assert 'Loading: params_ema does not exist, use params.' in caplog.text
    flat = str(tmp_path / 'flat.pth')
    torch.save(ema.state_dict(), flat)                       # a flat state dict still loads
    m.load_network(net, flat)
    assert _same(net, ema)


def test_constructor_honours_param_key_g(tmp_path, monkeypatch):
    """path.param_key_g selects the set net_g is loaded from (sr_model.py:27-30); the constructor up to that point on the CPU"""
    from mrefsr_amd.models import multi_ref_restoration_model as M
    params, ema = _net(1), _net(2)
    both = str(tmp_path / 'both.pth')
    _bare({}).save_network([params, ema], both, param_key=['params', 'params_ema'])
    monkeypatch.setattr(M, 'build_network', lambda o: _net(7))
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(torch.nn.Module, 'to', lambda self, *a, **k: self)
    for key, want in (('params_ema', ema), (None, params)):
        path = dict(pretrain_network_g=both, strict_load=True)
        if key:
            path['param_key_g'] = key
        m = M.MultiRefRestorationModel(dict(is_train=False, num_gpu=1, network_map={}, network_extractor={}, network_g={}, path=path))
        assert _same(m.net_g, want)


@pytest.mark.parametrize('cls_name', ['MultiRefRestorationModel', 'RefRestorationModel'])
def test_update_options_are_refused_with_hip_graph(cls_name, monkeypatch):
    from mrefsr_amd.models import multi_ref_restoration_model as M
    monkeypatch.delenv('MREFSR_TRAIN_GRAPH', raising=False)
    cls = getattr(M, cls_name)

    def bare(train):
        m = object.__new__(cls)
        m.opt = dict(dist=False, train=train)
        return m
    for train in ({}, {'ema_decay': 0.999}, {'hip_adam': True}, {'ema_decay': 0.999, 'hip_adam': True}, {'hip_graph': True},
                  {'ema_decay': 0, 'hip_adam': False, 'hip_graph': True}):
        bare(train)._check_update_options()
    with pytest.raises(ValueError, match='ema_decay.*hip_graph'):
        bare({'ema_decay': 0.999, 'hip_graph': True})._check_update_options()
    with pytest.raises(ValueError, match='hip_adam.*hip_graph'):
        bare({'hip_adam': True, 'hip_graph': True})._check_update_options()
    monkeypatch.setenv('MREFSR_TRAIN_GRAPH', '1')
    with pytest.raises(ValueError, match='hip_graph'):
        bare({'hip_adam': True})._check_update_options()
    assert bare({'hip_adam': True})._hip_adam_wanted() and not bare({})._hip_adam_wanted()


def test_constructor_refuses_the_pair(monkeypatch):
    """the refusal happens at construction, before any optimizer exists"""
    from mrefsr_amd.models import multi_ref_restoration_model as M
    monkeypatch.setattr(M, 'build_network', lambda o: _net(7))
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(torch.nn.Module, 'to', lambda self, *a, **k: self)
    for extra in ({'ema_decay': 0.999}, {'hip_adam': True}):
        with pytest.raises(ValueError, match='hip_graph'):
            M.MultiRefRestorationModel(dict(is_train=True, num_gpu=1, network_map={}, network_extractor={}, network_g={}, path={},
                                            train=dict(hip_graph=True, **extra)))


def test_hip_adam_state_dict_round_trips_through_torch_adam():
    from mrefsr_amd.optim import HipAdam

    def make(cls, **kw):
        torch.manual_seed(0)
        ps = [torch.nn.Parameter(torch.randn(n)) for n in (5, 7, 3)]
        return ps, cls([{'params': ps[:2]}, {'params': ps[2:], 'lr': 1e-5, 'weight_decay': 1e-4}], lr=1e-4, betas=(0.9, 0.99), **kw)

    ps, adam = make(torch.optim.Adam)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn_like(p)
        adam.step()
    _, hip_adam = make(HipAdam)
    assert type(hip_adam).step is not torch.optim.Adam.step and type(hip_adam).state_dict is torch.optim.Adam.state_dict
    hip_adam.load_state_dict(copy.deepcopy(adam.state_dict()))   # (load_state_dict adopts the tensors it is given)
    sd = hip_adam.state_dict()
    assert [pg['lr'] for pg in sd['param_groups']] == [1e-4, 1e-5] and sd['param_groups'][1]['weight_decay'] == 1e-4
    for i in range(3):
        assert sorted(sd['state'][i]) == ['exp_avg', 'exp_avg_sq', 'step'] and float(sd['state'][i]['step']) == 2.0
        for k in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(sd['state'][i][k], adam.state_dict()['state'][i][k])
    ps2, back = make(torch.optim.Adam)
    back.load_state_dict(copy.deepcopy(sd))
    for p, q in zip(ps, ps2):                                # and torch's Adam goes on from it exactly as from its own state
        q.data.copy_(p.data)
        g = torch.randn_like(p)
        p.grad, q.grad = g, g.clone()
    adam.step()
    back.step()
    assert all(torch.equal(p, q) for p, q in zip(ps, ps2))
    for k in ('amsgrad', 'maximize', 'fused'):
        with pytest.raises(NotImplementedError):
            HipAdam([torch.nn.Parameter(torch.zeros(1))], **{k: True})
    with pytest.raises(NotImplementedError, match='no CPU path'):   # the step is the HIP kernel: no quiet fall-back
        for p in hip_adam.param_groups[0]['params']:
            p.grad = torch.ones_like(p)
        hip_adam.step()
