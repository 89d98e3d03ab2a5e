"""CPU: SSIMLoss (mrefsr_amd/losses) and train.ssim_opt -- the definition against the numpy validation metric, its gradient against
finite differences, the options it refuses, and how the model builds it.  The GPU side: tests/test_ssim_loss_kernels_gpu.py,
tests/test_ssim_loss_train_gpu.py."""
import numpy as np
import pytest
import torch

from test_losses_cpu import _Bare


def _u8_pair(h, w, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    b = np.clip(a.astype(int) + rng.integers(-25, 26, a.shape), 0, 255).astype(np.uint8)
    return a, b


def _as_batch(img):
    return torch.from_numpy(img.astype(np.float64) / 255.0).permute(2, 0, 1)[None].contiguous()


@pytest.mark.parametrize('channel,tol', [('rgb', 1e-12), ('y', 1e-9)])
def test_one_minus_the_loss_is_the_validation_metric(channel, tol):
    """float64, uint8-valued images / 255: 1 - loss = metrics.calculate_ssim.  'y' differs by rgb_to_y's float32 division alone"""
    from mrefsr_amd.losses import SSIMLoss
    from mrefsr_amd.metrics import calculate_ssim
    a, b = _u8_pair(37, 45, 0)
    loss = SSIMLoss(channel=channel)(_as_batch(a), _as_batch(b))
    want = calculate_ssim(a, b, 0, test_y_channel=channel == 'y')
    err = abs((1.0 - float(loss)) - want)
    print(f'channel {channel}: |1 - loss - calculate_ssim| = {err:.2e} (ssim {want:.6f})')
    assert loss.dtype == torch.float64 and err <= tol
    # a batch is the mean over its images, and loss_weight multiplies
    c, d = _u8_pair(37, 45, 1)
    both = SSIMLoss(loss_weight=0.25, channel=channel)(torch.cat([_as_batch(a), _as_batch(c)]), torch.cat([_as_batch(b), _as_batch(d)]))
    want2 = 0.25 * (1.0 - 0.5 * (want + calculate_ssim(c, d, 0, test_y_channel=channel == 'y')))
    assert abs(float(both) - want2) <= tol


@pytest.mark.parametrize('channel', ['y', 'rgb'])
def test_gradient_against_central_differences(channel):
    """13 x 14 image (a 3 x 4 map), 36 pixels probed with h = 1e-5 in float64: the difference quotient's own error is the rounding
    eps |loss| / h ~ 1e-11 plus the truncation h^2 / 6 |f'''| ~ 1e-10 for third derivatives of order 10, so the two agree to 1e-9
    (measured: 3e-11); a wrong tap or coefficient shows at 1e-3 of the gradient's 1e-1"""
    from mrefsr_amd.losses import SSIMLoss
    cri = SSIMLoss(channel=channel)
    g = torch.Generator().manual_seed(1)
    pred = torch.rand(1, 3, 13, 14, dtype=torch.float64, generator=g)
    target = (pred + 0.1 * torch.randn(pred.shape, dtype=torch.float64, generator=g)).clamp(0, 1)
    p = pred.clone().requires_grad_(True)
    t = target.clone().requires_grad_(True)
    cri(p, t).backward()
    assert t.grad is None                                   # the target is a constant
    h, worst = 1e-5, 0.0
    for i in torch.randperm(pred.numel(), generator=g)[:36].tolist():
        up, down = pred.clone().view(-1), pred.clone().view(-1)
        up[i] += h
        down[i] -= h
        fd = (float(cri(up.view_as(pred), target)) - float(cri(down.view_as(pred), target))) / (2 * h)
        worst = max(worst, abs(fd - float(p.grad.view(-1)[i])))
    print(f'channel {channel}: max |central difference - autograd| = {worst:.2e}, max |grad| = {float(p.grad.abs().max()):.2e}')
    assert float(p.grad.abs().max()) > 1e-3 and worst <= 1e-9


@pytest.mark.parametrize('channel', ['y', 'rgb'])
def test_equal_images_give_zero_loss_and_zero_gradient(channel):
    from mrefsr_amd.losses import SSIMLoss
    x = torch.rand(2, 3, 19, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    p = x.clone().requires_grad_(True)
    loss = SSIMLoss(channel=channel)(p, x.clone())
    loss.backward()
    print(f'channel {channel}: loss {float(loss.detach()):.2e}, max |grad| {float(p.grad.abs().max()):.2e}')
    assert abs(float(loss.detach())) <= 1e-14 and float(p.grad.abs().max()) <= 1e-14    # float64 rounding of terms of order 1


def test_options_and_inputs_refused():
    from mrefsr_amd.losses import LOSS_REGISTRY, SSIMLoss, build_loss
    assert 'SSIMLoss' in LOSS_REGISTRY
    cri = build_loss(dict(type='SSIMLoss', loss_weight=0.5))
    assert (cri.loss_weight, cri.channel, cri.window_size, cri.sigma) == (0.5, 'y', 11, 1.5)
    assert not list(cri.parameters()) and not list(cri.buffers())
    for bad in (dict(window_size=7), dict(sigma=1.0), dict(channel='l'), dict(channel='Y')):
        with pytest.raises(NotImplementedError, match='SSIMLoss'):
            SSIMLoss(**bad)
    x = torch.rand(1, 3, 12, 12)
    for shape in ((1, 1, 12, 12), (1, 4, 12, 12), (3, 12, 12)):
        with pytest.raises(NotImplementedError, match='SSIMLoss'):
            cri(torch.rand(shape), torch.rand(shape))
    for shape in ((1, 3, 10, 12), (1, 3, 12, 10)):
        with pytest.raises(ValueError, match='SSIMLoss'):
            cri(torch.rand(shape), torch.rand(shape))
    with pytest.raises(ValueError, match='SSIMLoss'):
        cri(x, torch.rand(1, 3, 12, 13))
    assert cri(x, torch.rand(1, 3, 12, 12)).dtype == torch.float32     # CPU tensors of any float dtype take the torch expression
    assert cri(x.half().float().bfloat16(), x.bfloat16()).dtype == torch.bfloat16


def test_model_builds_the_criterion_from_ssim_opt():
    from mrefsr_amd.losses import L1Loss, SSIMLoss
    m = _Bare.settings(dict(ssim_opt=dict(loss_weight=0.3, channel='rgb')))
    assert isinstance(m.cri_ssim, SSIMLoss) and m.cri_ssim.loss_weight == 0.3 and m.cri_ssim.channel == 'rgb'
    assert isinstance(m.cri_pix, L1Loss) and m.cri_perceptual is None and m.cri_texture is None
    alone = _Bare.settings(dict(pixel_weight=0, ssim_opt=dict(loss_weight=1.0)))
    assert alone.cri_pix is None and alone.cri_ssim.channel == 'y'
    assert _Bare.settings({}).cri_ssim is None
    with pytest.raises(NotImplementedError, match='SSIMLoss'):
        _Bare.settings(dict(ssim_opt=dict(window_size=9)))


def test_graph_capture_is_not_asked_for_with_an_ssim_loss():
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    m = MultiRefRestorationModel.__new__(MultiRefRestorationModel)
    m.opt = dict(train=dict(hip_graph=True))
    assert m._train_graph_wanted()
    m.opt = dict(train=dict(hip_graph=True, ssim_opt=dict(loss_weight=1.0)))
    assert not m._train_graph_wanted()


def test_library_refuses_bad_shapes_before_any_launch():
    """host-side argument checks of csrc/ssim_loss.hip (no GPU needed): the block count of a shape, and error codes with messages"""
    import ctypes
    from mrefsr_amd import _lib
    lib = _lib.load()
    assert lib.mrefsr_ssim_loss_blocks(1, 11, 11, 0) == 1 and lib.mrefsr_ssim_loss_blocks(1, 11, 11, 1) == 3
    assert lib.mrefsr_ssim_loss_blocks(4, 160, 160, 0) == 4 * 10 * 5          # 150 x 150 map in 16 x 32 tiles
    assert lib.mrefsr_ssim_loss_blocks(2, 27, 43, 1) == 6 * 2 * 2
    assert lib.mrefsr_ssim_loss_blocks(1, 10, 64, 0) == -1 and lib.mrefsr_ssim_loss_blocks(0, 64, 64, 0) == -1
    p = ctypes.c_void_p(16)
    assert lib.mrefsr_ssim_loss_fwd_f32(p, p, 1, 10, 64, 0, 1.0, None, None, None, p, p, p, None) == -1
    assert b'ssim_loss_fwd' in lib.mrefsr_last_error()
    assert lib.mrefsr_ssim_loss_fwd_f32(p, p, 1, 64, 64, 0, 1.0, p, None, None, p, p, p, None) == -1
    assert b'all three' in lib.mrefsr_last_error()
    assert lib.mrefsr_ssim_loss_bwd_f32(p, p, p, p, p, None, 1, 64, 64, 0, 1.0, p, None) == -1
    assert b'null' in lib.mrefsr_last_error()
