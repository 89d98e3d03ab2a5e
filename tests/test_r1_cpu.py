"""CPU: GANLoss('wgan_softplus') and r1_penalty on CPU tensors, the C ABI of csrc/gan_reg.hip, and the refusals of train.r1_reg_weight /
train.net_d_reg_every.  The reference's values (tests/golden/gan_wgan_softplus.npz) come from tests/golden/gen_golden_gan_r1.py."""
import copy
import ctypes
import inspect
import os

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(got, want):
    got, want = got.detach().double(), want.detach().double()
    return ((got - want).norm() / want.norm().clamp_min(1e-300)).item()


def test_exports_and_signatures():
    from mrefsr_amd import _lib
    _vp, _i, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    want = {
        'mrefsr_r1_sqnorm_row_blocks': (_i, [_i64]),
        'mrefsr_r1_sqnorm_workspace_bytes': (_i64, [_i, _i64]),
        'mrefsr_r1_sqnorm_f32': (_i, [_vp, _i, _i64, _vp, _vp, _i64, _vp]),
        'mrefsr_r1_sqnorm_bwd_f32': (_i, [_vp, _vp, _i, _i64, _vp, _vp]),
    }
    header = open(os.path.join(ROOT, 'include', 'mrefsr_hip.h')).read()
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        assert name in header, name
    assert 'losses.py:391-405' in header and 'stylegan2_model.py:208-219' in header   # each entry cites the lines it serves
    lib = _lib.load()   # (binds every symbol: a missing export raises)
    # the grid is a pure function of (batch, n): T = ceil((n + 3) / 1024) chunks, min(ceil(T / 2), 512) blocks per row
    for n, blocks in ((1, 1), (1021, 1), (1022, 1), (2046, 2), (12288, 7), (49159, 25), (3 * 1024 * 1024, 512)):
        assert lib.mrefsr_r1_sqnorm_row_blocks(n) == blocks, n
        assert lib.mrefsr_r1_sqnorm_workspace_bytes(3, n) == 3 * blocks * 8
    assert lib.mrefsr_r1_sqnorm_row_blocks(0) == -1 and lib.mrefsr_r1_sqnorm_workspace_bytes(0, 8) == -1
    assert lib.mrefsr_r1_sqnorm_workspace_bytes(65536, 8) == -1
    # argument validation happens before any launch
    assert lib.mrefsr_r1_sqnorm_f32(None, 0, 0, None, None, 0, None) != 0
    assert lib.mrefsr_r1_sqnorm_f32(None, 1, 8, None, None, 0, None) != 0
    assert lib.mrefsr_r1_sqnorm_bwd_f32(None, None, 1, 8, None, None) != 0


def test_lane_squares_of_the_error_bound():
    from mrefsr_amd import hip
    # L = 4 ceil(T / blocks): one chunk or two per lane until a row has more than 1024 chunks
    assert [hip.r1_lane_squares(n) for n in (1, 3, 255, 1025, 12288, 49159)] == [4, 4, 4, 8, 8, 8]
    assert hip.r1_lane_squares(3 * 1024 * 1024) == 4 * 7   # 3073 chunks over 512 blocks


@pytest.mark.parametrize('shape', [(4, 1), (2, 1, 8, 8)])
def test_wgan_softplus_values_and_gradients(shape):
    """against F.softplus written out in float64: 1e-6 relative, for both targets, is_disc true and false, and a loss_weight"""
    from mrefsr_amd.losses import GANLoss
    torch.manual_seed(sum(shape))
    x = torch.randn(shape) * 4
    for real in (True, False):
        for is_disc in (True, False):
            for w in (1.0, 0.25):
                crit = GANLoss('wgan_softplus', loss_weight=w)
                assert crit.get_target_label(x, real) is real   # the label is a bool, as for wgan
                t = x.clone().requires_grad_(True)
                loss = crit(t, real, is_disc=is_disc)
                grad, = torch.autograd.grad(loss, t)
                t64 = x.double().requires_grad_(True)
                want = F.softplus(-t64 if real else t64).mean() * (1.0 if is_disc else w)
                wgrad, = torch.autograd.grad(want, t64)
                assert loss.dtype == torch.float32 and loss.dim() == 0
                assert _rel(loss, want) <= 1e-6 and _rel(grad, wgrad) <= 1e-6, (real, is_disc, w, _rel(loss, want), _rel(grad, wgrad))


def test_wgan_softplus_against_the_reference(golden):
    """the reference class's constructor signature, and its values and input gradients on the fixture's inputs"""
    from mrefsr_amd.losses import GANLoss
    g = golden('gan_wgan_softplus')
    sig = inspect.signature(GANLoss.__init__)
    assert list(sig.parameters) == [str(n) for n in g['ctor_names']]
    defaults = [repr(p.default) if p.default is not inspect.Parameter.empty else '' for p in sig.parameters.values()]
    assert defaults == [str(d) for d in g['ctor_defaults']]
    cases = [str(c) for c in g['cases']]
    assert len(cases) == 16
    for key in cases:
        xname, real, disc, w = key.split('_')
        x = torch.from_numpy(g[xname]).requires_grad_(True)
        loss = GANLoss('wgan_softplus', loss_weight=float(w[1:]))(x, real == 'real1', is_disc=disc == 'disc1')
        grad, = torch.autograd.grad(loss, x)
        want, wgrad = torch.from_numpy(g[key + '_loss']), torch.from_numpy(g[key + '_grad'])
        assert _rel(loss, want) <= 1e-6 and _rel(grad, wgrad) <= 1e-6, key


def test_wgan_softplus_has_a_double_backward():
    from mrefsr_amd.losses import GANLoss
    x = torch.linspace(-3, 3, 8).view(4, 2).double().requires_grad_(True)
    assert torch.autograd.gradgradcheck(lambda t: GANLoss('wgan_softplus')(t, True, is_disc=True), (x, ))
    with pytest.raises(NotImplementedError, match='wgan_softplus'):   # the refusal names what is implemented
        GANLoss('wgan_hinge')


def test_r1_penalty_on_cpu_tensors():
    """against the float64 formula for a small module that is differentiable twice"""
    from mrefsr_amd.losses import r1_penalty
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.Softplus(), torch.nn.Conv2d(4, 2, 3, stride=2),
                              torch.nn.Tanh(), torch.nn.Flatten(), torch.nn.Linear(2 * 3 * 3, 1))
    x = torch.randn(3, 3, 8, 8)
    xi = x.clone().requires_grad_(True)
    pen = r1_penalty(net(xi), xi)
    assert pen.dim() == 0 and pen.requires_grad
    grads = torch.autograd.grad(pen, list(net.parameters()), allow_unused=True)
    net64 = copy.deepcopy(net).double()
    x64 = x.double().requires_grad_(True)
    g64, = torch.autograd.grad(net64(x64).sum(), x64, create_graph=True)
    want = g64.pow(2).reshape(3, -1).sum(1).mean()
    wgrads = torch.autograd.grad(want, list(net64.parameters()), allow_unused=True)
    assert _rel(pen, want) <= 1e-5
    assert [a is None for a in grads] == [b is None for b in wgrads] == [False] * 5 + [True]   # (d D / d x does not see the last bias)
    for a, b in zip(grads[:5], wgrads[:5]):
        assert _rel(a, b) <= 1e-4


def _bare(cls_name, train):
    from mrefsr_amd.models import multi_ref_restoration_model as M
    m = object.__new__(getattr(M, cls_name))
    m.opt = dict(dist=False, train=train)
    return m


@pytest.mark.parametrize('cls_name', ['MultiRefRestorationModel', 'RefRestorationModel'])
def test_the_option_refusals(cls_name, monkeypatch):
    monkeypatch.delenv('MREFSR_TRAIN_GRAPH', raising=False)
    for train in ({}, {'r1_reg_weight': 10}, {'r1_reg_weight': 10.0, 'net_d_reg_every': 16}, {'r1_reg_weight': 0.5, 'net_d_reg_every': 1},
                  {'r1_reg_weight': 0}, {'r1_reg_weight': 0.0}, {'r1_reg_weight': 1.0, 'grad_clip_norm_d': 1.0, 'hip_adam': True}):
        _bare(cls_name, train)._check_update_options()
    for bad in (-1.0, -1, float('inf'), float('-inf'), float('nan'), True, False, '10', [10]):
        with pytest.raises(ValueError, match='r1_reg_weight'):
            _bare(cls_name, {'r1_reg_weight': bad})._check_update_options()
    for bad in (0, -2, 1.0, 2.5, float('inf'), float('nan'), True, False, '2'):
        with pytest.raises(ValueError, match='net_d_reg_every'):
            _bare(cls_name, {'r1_reg_weight': 10.0, 'net_d_reg_every': bad})._check_update_options()
    for train in ({'net_d_reg_every': 2}, {'net_d_reg_every': 2, 'r1_reg_weight': 0}, {'net_d_reg_every': 1, 'r1_reg_weight': 0.0}):
        with pytest.raises(ValueError, match='net_d_reg_every without train.r1_reg_weight'):
            _bare(cls_name, train)._check_update_options()


def _constructed(monkeypatch, train, **opt):
    """the constructor up to init_training_settings, through the seam of tests/test_gradclip_cpu.py"""
    from mrefsr_amd.models import multi_ref_restoration_model as M
    monkeypatch.delenv('MREFSR_TRAIN_GRAPH', raising=False)
    monkeypatch.setattr(M, 'build_network', lambda o: torch.nn.Conv2d(3, 4, 3))
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(torch.nn.Module, 'to', lambda self, *a, **k: self)
    base = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, beta_g=[0.9, 0.999], fused_adam=False,
                scheduler=dict(type='MultiStepLR', milestones=[10], gamma=0.5), net_g_pretrain_steps=0, pixel_criterion='L1Loss', pixel_weight=1.0)
    base.update(train)
    return M.MultiRefRestorationModel(dict(is_train=True, num_gpu=1, network_map={}, network_extractor={}, network_g={}, path={}, train=base, **opt))


def test_constructor_refusals_and_defaults(monkeypatch):
    with pytest.raises(ValueError, match='r1_reg_weight'):
        _constructed(monkeypatch, dict(r1_reg_weight=-1.0))
    with pytest.raises(ValueError, match='net_d_reg_every'):
        _constructed(monkeypatch, dict(net_d_reg_every=4))
    with pytest.raises(NotImplementedError, match='r1_reg_weight without network_d'):
        _constructed(monkeypatch, dict(r1_reg_weight=10.0, net_d_reg_every=16))
    gan = dict(gan_type='wgan_softplus', gan_weight=1e-3, grad_penalty_weight=0, lr_d=1e-4, beta_d=[0.9, 0.999])
    m = _constructed(monkeypatch, dict(gan, r1_reg_weight=10, net_d_reg_every=16), network_d=dict(type='StyleGAN2Discriminator', out_size=64))
    assert m.r1_reg_weight == 10.0 and m.net_d_reg_every == 16 and m.cri_gan.gan_type == 'wgan_softplus' and m.cri_grad_penalty is None
    m = _constructed(monkeypatch, dict(gan, r1_reg_weight=2.5), network_d=dict(type='StyleGAN2Discriminator', out_size=64))
    assert m.r1_reg_weight == 2.5 and m.net_d_reg_every == 1   # the default: every step
    m = _constructed(monkeypatch, dict(gan), network_d=dict(type='StyleGAN2Discriminator', out_size=64))
    assert m.r1_reg_weight == 0.0 and m.net_d_reg_every == 1   # absent: no R1
    # train.hip_graph already refuses a discriminator: the graph replay is not wanted then, R1 or not
    m = _constructed(monkeypatch, dict(gan, r1_reg_weight=10.0, hip_graph=True), network_d=dict(type='StyleGAN2Discriminator', out_size=64))
    assert not m._train_graph_wanted()
