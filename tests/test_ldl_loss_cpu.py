"""CPU: the LDL artifact loss (mrefsr_amd/losses: ldl_artifact_map_torch, ldl_loss_torch, LDLLoss) and train.ldl_opt -- the torch
expression in float64 against the reference's own function with autograd (tests/golden/ldl.npz, written by
tests/golden/gen_golden_ldl.py), its gradient against central differences, the zero-variance rule, the independence of the samples
of a batch, the options the module and the model refuse.  The GPU side: tests/test_ldl_loss_kernels_gpu.py,
tests/test_ldl_loss_train_gpu.py."""
import os

import numpy as np
import pytest
import torch

import ldl_cases
from test_losses_cpu import _Bare

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ldl.npz')


def _loss_and_grad(out, gt, ema, dtype=torch.float64, weight=1.0):
    from mrefsr_amd.losses import LDLLoss
    o = out.detach().to(dtype, copy=True).requires_grad_(True)
    loss = LDLLoss(loss_weight=weight)(o, gt.to(dtype), ema.to(dtype))
    loss.backward()
    return loss.detach(), o.grad


@pytest.mark.parametrize('cls', ldl_cases.CLASSES)
def test_float64_expression_is_the_reference_with_autograd(cls):
    """map, loss and gradient (through the map) within 1e-12 relative of the reference's float64 values, on every pixel"""
    from mrefsr_amd.losses import LDLLoss, ldl_artifact_map_torch
    z = np.load(GOLDEN)
    for shape in ldl_cases.GOLDEN_SHAPES:
        key = ldl_cases.golden_key(cls, shape)
        out, gt, ema = (torch.from_numpy(z[f'{key}_{n}']) for n in ('out', 'gt', 'ema'))
        again = ldl_cases.make_inputs(cls, shape, 7000 + 100 * ldl_cases.CLASSES.index(cls) + ldl_cases.GOLDEN_SHAPES.index(shape))
        assert all(torch.equal(a, b) for a, b in zip(again, (out, gt, ema)))     # the fixture's inputs are ldl_cases' own
        w64, grad64 = torch.from_numpy(z[f'{key}_w']), torch.from_numpy(z[f'{key}_grad'])
        w = ldl_artifact_map_torch(gt.double(), out.double(), ema.double())
        loss, grad = _loss_and_grad(out, gt, ema, weight=float(z['loss_weight']))
        ew = float((w - w64).abs().max() / w64.abs().max())
        el = abs(float(loss) - float(z[f'{key}_loss'])) / float(z[f'{key}_loss'])
        eg = float((grad - grad64).abs().max() / grad64.abs().max())
        print(f'{key:22s} map {ew:.1e}  loss {el:.1e}  gradient {eg:.1e}  masked {float((w64 == 0).double().mean()):.2f}')
        assert w.shape == (shape[0], 1, *shape[1:]) and torch.equal(w == 0, w64 == 0)
        assert ew <= 1e-12 and el <= 1e-12 and eg <= 1e-12
        assert torch.equal(LDLLoss().artifact_map(out.double(), gt.double(), ema.double()), w)


@pytest.mark.parametrize('cls', ldl_cases.CLASSES)
def test_gradient_against_central_differences(cls):
    """2 x 9 x 8, float64, h = 1e-6, 40 elements with |out - gt| >= 1e-3 at pixels with |r - r_e| >= 1e-3: a step of h crosses
    neither the kink of |.| nor the mask's boundary there, and it moves r at no other pixel, so every other mask bit stays (exact ties
    sit on the boundary and are not probed).  Away from those kinks the loss is smooth and the quotient's error is its rounding,
    eps |loss| / h ~ 2e-16 * 2e-4 / 1e-6 = 4e-14, plus the truncation h^2 / 6 times a third derivative: bound 1e-7 of max |grad|
    ~ 1e-4, i.e. 1e-11 (measured 4e-14); a wrong tap or multiplicity shows at 1e-2 of the gradient"""
    out, gt, ema = (t.double() for t in ldl_cases.make_inputs(cls, (2, 9, 8), 11))
    _, grad = _loss_and_grad(out, gt, ema)
    from mrefsr_amd.losses import ldl_loss_torch
    r, r_e = (gt - out).abs().sum(1), (gt - ema).abs().sum(1)
    ok = (((r - r_e).abs() >= 1e-3)[:, None] & ((out - gt).abs() >= 1e-3)).flatten()
    h, worst, probed = 1e-6, 0.0, 0
    for i in torch.randperm(out.numel(), generator=torch.Generator().manual_seed(3)).tolist():
        if not ok[i] or probed == 40:
            continue
        up, down = out.clone().view(-1), out.clone().view(-1)
        up[i] += h
        down[i] -= h
        fd = (float(ldl_loss_torch(up.view_as(out), gt, ema)) - float(ldl_loss_torch(down.view_as(out), gt, ema))) / (2 * h)
        worst = max(worst, abs(fd - float(grad.view(-1)[i])))
        probed += 1
    scale = float(grad.abs().max())
    print(f'class {cls}: {probed} elements, max |central difference - autograd| = {worst:.2e}, max |grad| = {scale:.2e}')
    assert probed == 40 and scale > 0 and worst <= 1e-7 * scale


def test_zero_variance_sample_gives_no_loss_and_a_finite_zero_gradient():
    """out == gt in sample 0: the reference's gradient is NaN there (0 * 0^(-4/5)); here it is 0, and sample 1 is what it is alone
    (the mean over B = 2 halves it)"""
    out, gt, ema = (t.double() for t in ldl_cases.make_inputs('generic', (2, 11, 10), 5))
    out[0] = gt[0]
    loss, grad = _loss_and_grad(out, gt, ema)
    alone, grad_alone = _loss_and_grad(out[1:], gt[1:], ema[1:], weight=0.5)
    assert bool(torch.isfinite(grad).all()) and float(grad[0].abs().max()) == 0.0
    assert float(loss) > 0 and abs(float(loss) - float(alone)) <= 1e-15 * float(alone)
    assert float((grad[1:] - grad_alone).abs().max()) <= 1e-15 * float(grad_alone.abs().max())
    # a constant residual that is not 0 has no variance either
    out[0] = gt[0] + 0.25
    loss2, grad2 = _loss_and_grad(out, gt, ema)
    assert bool(torch.isfinite(grad2).all()) and float(grad2[0].abs().max()) == 0.0 and abs(float(loss2) - float(alone)) <= 1e-15 * float(alone)
    from mrefsr_amd.losses import ldl_artifact_map_torch
    assert float(ldl_artifact_map_torch(gt, out, ema)[0].abs().max()) == 0.0


def test_samples_of_a_batch_do_not_mix():
    """two samples with residuals 30 x apart: the batch is each sample alone with loss_weight 1 / 2 (the per-sample variance g_b must
    not be a batch variance: g of the pair would exceed the small sample's own by (30^2)^(1/5) ~ 4)"""
    out, gt, ema = (t.double() for t in ldl_cases.make_inputs('generic', (2, 12, 13), 6, scales=[0.01, 0.3]))
    loss, grad = _loss_and_grad(out, gt, ema)
    total = 0.0
    for b in range(2):
        lb, gb = _loss_and_grad(out[b:b + 1], gt[b:b + 1], ema[b:b + 1], weight=0.5)
        total += float(lb)
        assert float((grad[b:b + 1] - gb).abs().max()) <= 1e-14 * float(gb.abs().max())
    assert abs(float(loss) - total) <= 1e-14 * total


def test_options_and_inputs_refused():
    from mrefsr_amd.losses import LOSS_REGISTRY, LDLLoss, build_loss
    assert 'LDLLoss' in LOSS_REGISTRY
    cri = build_loss(dict(type='LDLLoss', loss_weight=0.5))
    assert (cri.loss_weight, cri.ksize) == (0.5, 7) and not list(cri.parameters()) and not list(cri.buffers())
    for bad in (5, 9, 7.5, True):
        with pytest.raises(NotImplementedError, match='LDLLoss'):
            LDLLoss(ksize=bad)
    x = torch.rand(1, 3, 6, 6)
    for shape in ((1, 1, 6, 6), (1, 4, 6, 6), (3, 6, 6)):
        with pytest.raises(NotImplementedError, match='LDLLoss'):
            cri(torch.rand(shape), torch.rand(shape), torch.rand(shape))
    for shape in ((1, 3, 3, 6), (1, 3, 6, 3)):
        with pytest.raises(ValueError, match='LDLLoss'):
            cri(torch.rand(shape), torch.rand(shape), torch.rand(shape))
    with pytest.raises(ValueError, match='LDLLoss'):
        cri(x, torch.rand(1, 3, 6, 7), x)
    with pytest.raises(ValueError, match='LDLLoss'):
        cri(x, x, torch.rand(2, 3, 6, 6))
    assert cri(x, torch.rand(1, 3, 6, 6), torch.rand(1, 3, 6, 6)).dtype == torch.float32   # CPU tensors of any float dtype: the torch expression
    assert cri(torch.rand(1, 3, 4, 4).double(), torch.rand(1, 3, 4, 4).double(), torch.rand(1, 3, 4, 4).double()).dtype == torch.float64
    # target and pred_ema are constants
    t, e = torch.rand(1, 3, 6, 6, requires_grad=True), torch.rand(1, 3, 6, 6, requires_grad=True)
    p = x.clone().requires_grad_(True)
    cri(p, t, e).backward()
    assert p.grad is not None and t.grad is None and e.grad is None
    assert not LDLLoss().artifact_map(p, t, e).requires_grad


def test_model_builds_the_criterion_from_ldl_opt():
    from mrefsr_amd.losses import L1Loss, LDLLoss
    opt = dict(type='L1Loss', loss_weight=0.7, reduction='mean')
    m = _Bare.settings(dict(ema_decay=0.999, ldl_opt=dict(opt)))
    assert isinstance(m.cri_ldl, LDLLoss) and m.cri_ldl.loss_weight == 0.7 and m.cri_ldl.ksize == 7 and isinstance(m.cri_pix, L1Loss)
    assert _Bare.settings(dict(ema_decay=0.999, ldl_opt=dict(opt, ksize=7))).cri_ldl.ksize == 7
    assert _Bare.settings(dict(ema_decay=0.999)).cri_ldl is None and _Bare.settings({}).cri_ldl is None
    for ema in ({}, dict(ema_decay=0), dict(ema_decay=None)):
        with pytest.raises(ValueError, match='ema_decay'):
            _Bare.settings(dict(ema, ldl_opt=dict(opt)))
    with pytest.raises(NotImplementedError, match='type'):
        _Bare.settings(dict(ema_decay=0.999, ldl_opt=dict(opt, type='MSELoss')))
    with pytest.raises(NotImplementedError, match='reduction'):
        _Bare.settings(dict(ema_decay=0.999, ldl_opt=dict(opt, reduction='sum')))
    with pytest.raises(NotImplementedError, match='LDLLoss'):
        _Bare.settings(dict(ema_decay=0.999, ldl_opt=dict(opt, ksize=5)))
    with pytest.raises(ValueError, match='unknown'):
        _Bare.settings(dict(ema_decay=0.999, ldl_opt=dict(opt, detach=True)))


def test_graph_capture_is_not_asked_for_with_an_ldl_loss():
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    m = MultiRefRestorationModel.__new__(MultiRefRestorationModel)
    m.opt = dict(train=dict(hip_graph=True))
    assert m._train_graph_wanted()
    m.opt = dict(train=dict(hip_graph=True, ema_decay=0.999, ldl_opt=dict(type='L1Loss', loss_weight=1.0, reduction='mean')))
    assert not m._train_graph_wanted()


def test_library_refuses_bad_shapes_before_any_launch():
    """host-side argument checks of csrc/ldl_loss.hip (no GPU needed): the block count of a shape, and error codes with messages"""
    import ctypes
    from mrefsr_amd import _lib
    lib = _lib.load()
    assert lib.mrefsr_ldl_loss_blocks(1, 4, 4) == 1 and lib.mrefsr_ldl_loss_blocks(4, 160, 160) == 4 * 10 * 5
    assert lib.mrefsr_ldl_loss_blocks(3, 17, 33) == 3 * 2 * 2
    assert lib.mrefsr_ldl_loss_blocks(1, 3, 64) == -1 and lib.mrefsr_ldl_loss_blocks(1, 64, 3) == -1 and lib.mrefsr_ldl_loss_blocks(0, 64, 64) == -1
    p = ctypes.c_void_p(16)
    assert lib.mrefsr_ldl_loss_fwd_f32(p, p, p, 1, 3, 64, 1.0, None, None, None, p, p, p, p, None) == -1
    assert b'ldl_loss_fwd' in lib.mrefsr_last_error()
    assert lib.mrefsr_ldl_loss_fwd_f32(p, p, p, 1, 64, 64, 1.0, p, None, None, p, p, p, p, None) == -1
    assert b'both' in lib.mrefsr_last_error()
    assert lib.mrefsr_ldl_loss_bwd_f32(p, p, p, p, p, p, None, 1, 64, 64, 1.0, p, None) == -1
    assert b'null' in lib.mrefsr_last_error()
    assert lib.mrefsr_ldl_loss_map_f32(p, None, 1, 64, 64, p, None) == -1
