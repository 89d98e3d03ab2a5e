"""CPU: FFTLoss and FocalFrequencyLoss (mrefsr_amd/losses) and train.freq_opt -- closed forms of the two torch definitions, their
gradients against central differences, the options and inputs they refuse, how the model builds the criterion, and the library's
host-side shape checks.  The GPU side: tests/test_freq_loss_kernels_gpu.py, tests/test_freq_loss_train_gpu.py."""
import math

import pytest
import torch

from test_losses_cpu import _Bare


def _pair(shape, seed, noise=0.1):
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(shape, dtype=torch.float64, generator=g)
    return target + noise * torch.randn(shape, dtype=torch.float64, generator=g), target


def test_closed_forms_of_the_definitions():
    """float64, 1e-12: a 1 x 1 transform is the identity; alpha = 0 makes every weight 1 and the ortho transform is unitary
    (Parseval); the two norms of FFTLoss differ by sqrt(H W)"""
    from mrefsr_amd.losses import FFTLoss, FocalFrequencyLoss, fft_loss_torch, focal_frequency_loss_torch
    pred, target = _pair((2, 3, 1, 1), 0)
    assert abs(float(FFTLoss(loss_weight=0.7)(pred, target)) - 0.7 * float((pred - target).abs().mean()) / 2) <= 1e-12
    for shape in ((2, 3, 8, 6), (1, 2, 7, 9), (1, 3, 1, 5)):
        pred, target = _pair(shape, 1)
        mse = float(((pred - target) ** 2).mean())
        assert abs(float(FocalFrequencyLoss(loss_weight=0.3, alpha=0)(pred, target)) - 0.3 * mse) <= 1e-12
        assert abs(float(focal_frequency_loss_torch(pred, target, alpha=0.0)) - mse) <= 1e-12
        h, w = shape[2:]
        ortho, backward = float(FFTLoss(norm='ortho')(pred, target)), float(FFTLoss(norm='backward')(pred, target))
        assert abs(ortho * math.sqrt(h * w) - backward) <= 1e-12 * max(1.0, backward)
        assert abs(backward - float(fft_loss_torch(pred, target))) == 0.0
        # the mean over the stacked real and imaginary parts of the full spectrum, spelt out
        d = torch.fft.fft2(pred) - torch.fft.fft2(target)
        assert abs(backward - float(torch.nn.functional.l1_loss(torch.stack([d.real, d.imag], -1), torch.zeros(*shape, 2, dtype=torch.float64)))) <= 1e-12
    # alpha = 1: the weight is |D| over its per-plane maximum, a constant
    pred, target = _pair((2, 3, 8, 6), 2)
    d = torch.fft.fft2(pred, norm='ortho') - torch.fft.fft2(target, norm='ortho')
    m = d.real ** 2 + d.imag ** 2
    w = m.sqrt() / m.sqrt().amax(dim=(2, 3), keepdim=True)
    assert abs(float(FocalFrequencyLoss()(pred, target)) - float((w * m).mean())) <= 1e-12


def _central_differences(fn, pred, n, h, gen):
    out = []
    for i in torch.randperm(pred.numel(), generator=gen)[:n].tolist():
        up, down = pred.clone().view(-1), pred.clone().view(-1)
        up[i] += h
        down[i] -= h
        out.append((i, (float(fn(up.view_as(pred))) - float(fn(down.view_as(pred)))) / (2 * h)))
    return out


@pytest.mark.parametrize('kind', ['fft-backward', 'fft-ortho', 'focal-1', 'focal-0.5'])
def test_gradient_against_central_differences(kind):
    """1 x 2 x 8 x 6 images in float64, all 96 pixels probed with h = 1e-6.  The L1 form is piecewise linear (exact quotient away
    from a kink; the inputs have no component within 1e-4 of zero, asserted), the focal form with its weight held fixed -- it is
    detached -- is quadratic (exact central quotient): what is left is the rounding eps |loss| / h ~ 1e-10 at most"""
    from mrefsr_amd.losses import FFTLoss, FocalFrequencyLoss, focal_frequency_loss_torch, focal_frequency_weight_torch
    gen = torch.Generator().manual_seed(3)
    pred, target = _pair((1, 2, 8, 6), 3)
    p = pred.clone().requires_grad_(True)
    t = target.clone().requires_grad_(True)
    if kind.startswith('fft'):
        norm = kind.split('-')[1]
        cri = FFTLoss(loss_weight=0.5, norm=norm)
        d = torch.view_as_real(torch.fft.fft2(pred - target, norm=norm))
        ky, kx = torch.meshgrid(torch.arange(8), torch.arange(6), indexing='ij')
        structural = ((ky % 4 == 0) & (kx % 3 == 0)).expand(1, 2, 8, 6)          # imaginary parts that are zero for a real input
        comps = torch.cat([d[..., 0].flatten(), d[..., 1][~structural].flatten()])
        assert float(comps.abs().min()) > 1e-4
        fn = lambda x: cri(x, target)
    else:
        alpha = float(kind.split('-')[1])
        cri = FocalFrequencyLoss(loss_weight=0.5, alpha=alpha)
        w = focal_frequency_weight_torch(pred, target, alpha)
        assert float(w.max()) == 1.0 and float(w.min()) >= 0.0
        fn = lambda x: 0.5 * focal_frequency_loss_torch(x, target, alpha, weight=w)
    cri(p, t).backward()
    assert t.grad is None                                   # the target is a constant
    worst = max(abs(fd - float(p.grad.view(-1)[i])) for i, fd in _central_differences(fn, pred, 96, 1e-6, gen))
    print(f'{kind}: max |central difference - autograd| = {worst:.2e}, max |grad| = {float(p.grad.abs().max()):.2e}')
    assert float(p.grad.abs().max()) > 1e-4 and worst <= 1e-9


def test_equal_images_give_zero_loss_and_a_zero_finite_gradient():
    from mrefsr_amd.losses import FFTLoss, FocalFrequencyLoss
    x = torch.rand(2, 3, 9, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    for cri in (FFTLoss(), FFTLoss(norm='ortho'), FocalFrequencyLoss(), FocalFrequencyLoss(alpha=0.5), FocalFrequencyLoss(alpha=0)):
        p = x.clone().requires_grad_(True)
        loss = cri(p, x.clone())
        loss.backward()
        assert float(loss.detach()) == 0.0 and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) == 0.0


def test_options_and_inputs_refused():
    from mrefsr_amd.losses import LOSS_REGISTRY, FFTLoss, FocalFrequencyLoss, build_loss
    assert 'FFTLoss' in LOSS_REGISTRY and 'FocalFrequencyLoss' in LOSS_REGISTRY
    cri = build_loss(dict(type='FFTLoss', loss_weight=0.5))
    assert (cri.loss_weight, cri.reduction, cri.norm) == (0.5, 'mean', 'backward')
    ffl = build_loss(dict(type='FocalFrequencyLoss', loss_weight=2.0, alpha=0.5))
    assert (ffl.loss_weight, ffl.alpha, ffl.patch_factor, ffl.ave_spectrum, ffl.log_matrix, ffl.batch_matrix) == (2.0, 0.5, 1, False, False, False)
    for c in (cri, ffl):
        assert not list(c.parameters()) and not list(c.buffers())
    for bad in (dict(reduction='sum'), dict(reduction='none'), dict(norm='forward'), dict(norm=None)):
        with pytest.raises(NotImplementedError, match='FFTLoss'):
            FFTLoss(**bad)
    for bad in (dict(patch_factor=2), dict(ave_spectrum=True), dict(log_matrix=True), dict(batch_matrix=True)):
        with pytest.raises(NotImplementedError, match='FocalFrequencyLoss'):
            FocalFrequencyLoss(**bad)
    for bad in (-1.0, float('inf'), float('nan'), 'one'):
        with pytest.raises(ValueError, match='alpha'):
            FocalFrequencyLoss(alpha=bad)
    for c, name in ((cri, 'FFTLoss'), (ffl, 'FocalFrequencyLoss')):
        for shape in ((3, 12, 12), (1, 1, 3, 12, 12), (1, 3, 0, 12), (1, 3, 12, 1025), (1, 3, 1025, 12)):
            with pytest.raises(ValueError, match=name):
                c(torch.rand(shape), torch.rand(shape))
        with pytest.raises(ValueError, match=name):
            c(torch.rand(1, 3, 12, 12), torch.rand(1, 3, 12, 13))
        x = torch.rand(2, 5, 12, 7)                                     # C is free: the planes are B C
        assert c(x, torch.rand(2, 5, 12, 7)).dtype == torch.float32     # CPU tensors of any float dtype take the torch expression
        assert c(x.double(), x.double() + 0.1).dtype == torch.float64
        assert float(c(torch.rand(1, 1, 1024, 3), torch.rand(1, 1, 1024, 3))) > 0


def test_model_builds_the_criterion_from_freq_opt():
    from mrefsr_amd.losses import FFTLoss, FocalFrequencyLoss, L1Loss
    m = _Bare.settings(dict(freq_opt=dict(type='FFTLoss', loss_weight=0.05, norm='ortho')))
    assert isinstance(m.cri_freq, FFTLoss) and m.cri_freq.loss_weight == 0.05 and m.cri_freq.norm == 'ortho'
    assert isinstance(m.cri_pix, L1Loss) and m.cri_perceptual is None and m.cri_ssim is None
    alone = _Bare.settings(dict(pixel_weight=0, freq_opt=dict(type='FocalFrequencyLoss', alpha=0.5)))
    assert alone.cri_pix is None and isinstance(alone.cri_freq, FocalFrequencyLoss) and alone.cri_freq.alpha == 0.5
    assert _Bare.settings({}).cri_freq is None and _Bare.settings(dict(freq_opt={})).cri_freq is None
    for bad in (dict(type='SSIMLoss'), dict(type='L1Loss', loss_weight=1.0), dict(loss_weight=1.0)):
        with pytest.raises(ValueError, match='FFTLoss or FocalFrequencyLoss'):
            _Bare.settings(dict(freq_opt=bad))
    with pytest.raises(NotImplementedError, match='FocalFrequencyLoss'):
        _Bare.settings(dict(freq_opt=dict(type='FocalFrequencyLoss', patch_factor=4)))
    opt = dict(type='FFTLoss', loss_weight=0.1)
    _Bare.settings(dict(freq_opt=opt))
    assert opt == dict(type='FFTLoss', loss_weight=0.1)                 # the options are not written to


def test_graph_capture_is_not_asked_for_with_a_frequency_loss():
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    m = MultiRefRestorationModel.__new__(MultiRefRestorationModel)
    m.opt = dict(train=dict(hip_graph=True))
    assert m._train_graph_wanted()
    m.opt = dict(train=dict(hip_graph=True, freq_opt=dict(type='FFTLoss')))
    assert not m._train_graph_wanted()


def test_library_refuses_bad_shapes_before_any_launch():
    """host-side argument checks of csrc/freq_loss.hip (no GPU needed): the block count of a shape, and error codes with messages"""
    import ctypes
    from mrefsr_amd import _lib
    from mrefsr_amd.hip import FREQ_MAX_SIDE, FREQ_TILE
    assert FREQ_TILE == (32, 32) and FREQ_MAX_SIDE == 1024
    lib = _lib.load()
    assert lib.mrefsr_freq_loss_blocks(1, 1, 1) == 1 and lib.mrefsr_freq_loss_blocks(12, 160, 160) == 12 * 5 * 3   # 81 columns
    assert lib.mrefsr_freq_loss_blocks(3, 33, 62) == 3 * 2 * 1 and lib.mrefsr_freq_loss_blocks(3, 33, 64) == 3 * 2 * 2
    assert lib.mrefsr_freq_loss_blocks(1, 1024, 1024) == 32 * 17
    for planes, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 1025, 8), (1, 8, 1025), (65536, 8, 8), (4096, 1024, 1024)):
        assert lib.mrefsr_freq_loss_blocks(planes, h, w) == -1
    p = ctypes.c_void_p(16)
    for planes, h, w in ((0, 8, 8), (1, 1025, 8), (1, 8, 0)):
        assert lib.mrefsr_freq_loss_fwd_f32(p, p, planes, h, w, 0, 0, 1.0, 1.0, p, p, p, p, 1, p, p, p, None) == -1
        assert b'freq_loss_fwd' in lib.mrefsr_last_error()
        assert lib.mrefsr_freq_loss_bwd_f32(p, p, planes, h, w, 1.0, p, p, p, p, None) == -1
        assert b'freq_loss_bwd' in lib.mrefsr_last_error()
    assert lib.mrefsr_freq_loss_fwd_f32(p, p, 1, 8, 8, 0, 0, 1.0, 1.0, p, p, None, p, 1, p, p, p, None) == -1
    assert b'null' in lib.mrefsr_last_error()
    assert lib.mrefsr_freq_loss_fwd_f32(p, p, 1, 8, 8, 1, 0, 1.0, 1.0, p, p, p, None, 0, p, p, p, None) == -1
    assert b'map g' in lib.mrefsr_last_error()
    assert lib.mrefsr_freq_loss_fwd_f32(p, p, 1, 8, 8, 1, 0, -1.0, 1.0, p, p, p, p, 0, p, p, p, None) == -1
    assert b'alpha' in lib.mrefsr_last_error()
    assert lib.mrefsr_freq_loss_bwd_f32(p, None, 1, 8, 8, 1.0, p, p, p, p, None) == -1
    assert b'null' in lib.mrefsr_last_error()
