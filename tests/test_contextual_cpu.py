"""CPU: ContextualLoss (mrefsr_amd/losses) and train.contextual_opt -- closed forms of the torch definition of one tap, its gradient
against central differences, the options and inputs refused, how the model builds the criterion, and the library's host-side shape
checks.  The GPU side: tests/test_contextual_kernels_gpu.py, tests/test_contextual_train_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

from test_losses_cpu import _Bare

LAYERS = {'relu2_2': 1.0, 'relu3_1': 0.5}


def _fields(c, h, w, b, seed):
    """correlated feature maps (independent Gaussian features saturate the loss): a blurred rank-8 field mixed to c channels; y its
    top-left window, x the window one position down and right plus noise, both through a ReLU"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(b, 8, h + 1, w + 1, generator=g, dtype=torch.float64)
    z = F.avg_pool2d(F.pad(z, (2, 2, 2, 2), mode='replicate'), 5, 1) * 5
    f = torch.einsum('ck,bkhw->bchw', torch.randn(c, 8, generator=g, dtype=torch.float64), z)
    return F.relu(f[:, :, 1:, 1:] + 0.1 * torch.randn(b, c, h, w, generator=g, dtype=torch.float64)).contiguous(), \
        F.relu(f[:, :, :h, :w]).contiguous()


def test_closed_forms_of_the_definition():
    from mrefsr_amd.losses import contextual_loss_torch
    x, y = _fields(16, 6, 5, 2, 0)
    # x = y: every position's nearest neighbour is itself at distance 0, exp(1 / h) dominates its row: CX = 1 up to rounding
    loss, parts = contextual_loss_torch(y, y, 0.1, parts=True)
    assert float((parts['CX'] - 1.0).abs().max()) <= 1e-9 and abs(float(loss) + torch.log(torch.tensor(1.0 + 1e-5, dtype=torch.float64))) <= 1e-9
    n = 30
    assert torch.equal(parts['jmin'], torch.arange(n).expand(2, n)) and torch.equal(parts['imax'], torch.arange(n).expand(2, n))
    # permuting the positions of x permutes the rows of the distance matrix: the column maxima, and so the loss, stay
    base, parts = contextual_loss_torch(x, y, 0.5, parts=True)
    assert 0.05 < float(parts['CX'].min()) and float(parts['CX'].max()) < 0.98
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    xp = x.flatten(2)[:, :, perm].reshape(x.shape)
    assert abs(float(contextual_loss_torch(xp, y, 0.5)) - float(base)) <= 1e-12
    # the feature means are taken per sample: B = 2 is the mean of the two samples fed alone
    alone = [float(contextual_loss_torch(x[b:b + 1], y[b:b + 1], 0.5)) for b in range(2)]
    assert abs(float(base) - sum(alone) / 2) <= 1e-12
    # given selections route the values: the computed ones give the same loss, and the target gets no gradient
    again = contextual_loss_torch(x, y, 0.5, jmin=parts['jmin'], imax=parts['imax'])
    assert float(again) == float(base)
    xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    contextual_loss_torch(xr, yr, 0.5).backward()
    assert yr.grad is None and float(xr.grad.abs().max()) > 0


@pytest.mark.parametrize('bw', [0.5, 0.1])
def test_gradient_against_central_differences(bw):
    """float64, 2 x 8 x 5 x 4 maps, 60 elements probed with step 1e-6.  The loss is smooth where no selection changes inside the
    step (asserted: the selections at x +- step are those at x), so the central quotient is exact to O(step^2) + rounding"""
    from mrefsr_amd.losses import contextual_loss_torch
    x, y = _fields(8, 5, 4, 2, 2)
    xr = x.clone().requires_grad_(True)
    loss, parts = contextual_loss_torch(xr, y, bw, parts=True)
    loss.backward()
    step, worst = 1e-6, 0.0
    for i in torch.randperm(x.numel(), generator=torch.Generator().manual_seed(3))[:60].tolist():
        vals = []
        for sgn in (1.0, -1.0):
            xs = x.clone().view(-1)
            xs[i] += sgn * step
            v, p = contextual_loss_torch(xs.view_as(x), y, bw, parts=True)
            assert torch.equal(p['jmin'], parts['jmin']) and torch.equal(p['imax'], parts['imax'])
            vals.append(float(v))
        worst = max(worst, abs((vals[0] - vals[1]) / (2 * step) - float(xr.grad.view(-1)[i])))
    print(f'band {bw}: max |central difference - autograd| = {worst:.2e}, max |grad| = {float(xr.grad.abs().max()):.2e}')
    assert float(xr.grad.abs().max()) > 1e-4 and worst <= 1e-7 * max(1.0, float(xr.grad.abs().max()))


def test_options_and_inputs_refused():
    from mrefsr_amd.losses import LOSS_REGISTRY, ContextualLoss, build_loss, contextual_loss_torch
    assert 'ContextualLoss' in LOSS_REGISTRY
    cri = build_loss(dict(type='ContextualLoss', layer_weights=LAYERS, band_width=0.25, loss_weight=0.1))
    assert (cri.band_width, cri.loss_weight, cri.norm_img, cri.layer_weights) == (0.25, 0.1, False, LAYERS)
    assert ContextualLoss(LAYERS).band_width == 0.5 and ContextualLoss(LAYERS).loss_weight == 1.0
    assert not [p for p in cri.parameters() if p.requires_grad]      # the VGG is frozen
    with pytest.raises(NotImplementedError, match='batch-normalised'):
        ContextualLoss(LAYERS, vgg_type='vgg19_bn')
    for bad in (0.0, -0.5, float('inf'), float('nan'), 'wide', None, True):
        with pytest.raises(ValueError, match='band_width'):
            ContextualLoss(LAYERS, band_width=bad)
    for bad in ({}, None, ['relu2_2']):
        with pytest.raises(ValueError, match='layer_weights'):
            ContextualLoss(bad)
    for shape in ((3, 32, 32), (1, 1, 32, 32), (1, 4, 32, 32), (1, 1, 3, 32, 32)):
        with pytest.raises(ValueError, match='ContextualLoss'):
            cri(torch.rand(shape), torch.rand(shape))
    with pytest.raises(ValueError, match='differ'):
        cri(torch.rand(1, 3, 32, 32), torch.rand(1, 3, 32, 36))
    with pytest.raises(NotImplementedError, match='no CPU path'):
        cri(torch.rand(1, 3, 32, 32), torch.rand(1, 3, 32, 32))
    with pytest.raises(ValueError, match='one shape'):
        contextual_loss_torch(torch.rand(1, 8, 4, 4), torch.rand(1, 8, 4, 5))
    with pytest.raises(ValueError, match='band_width'):
        contextual_loss_torch(torch.rand(1, 8, 4, 4), torch.rand(1, 8, 4, 4), 0.0)
    with pytest.raises(ValueError, match='2 positions'):
        contextual_loss_torch(torch.rand(1, 8, 1, 1), torch.rand(1, 8, 1, 1))
    # any dtype, any device: the definition runs where its tensors are
    x, y = _fields(8, 4, 4, 1, 4)
    assert contextual_loss_torch(x.float(), y.float()).dtype == torch.float32 and contextual_loss_torch(x, y).dtype == torch.float64


def test_model_builds_the_criterion_from_contextual_opt():
    from mrefsr_amd.losses import ContextualLoss, L1Loss
    opt = dict(layer_weights=dict(LAYERS), band_width=0.2, loss_weight=0.05)
    m = _Bare.settings(dict(contextual_opt=opt))
    assert isinstance(m.cri_contextual, ContextualLoss) and m.cri_contextual.band_width == 0.2 and m.cri_contextual.loss_weight == 0.05
    assert isinstance(m.cri_pix, L1Loss) and m.cri_perceptual is None and m.cri_texture is None and m.cri_freq is None
    assert opt == dict(layer_weights=dict(LAYERS), band_width=0.2, loss_weight=0.05)       # the options are not written to
    alone = _Bare.settings(dict(pixel_weight=0, contextual_opt=dict(layer_weights=LAYERS)))
    assert alone.cri_pix is None and isinstance(alone.cri_contextual, ContextualLoss)
    assert _Bare.settings({}).cri_contextual is None and _Bare.settings(dict(contextual_opt={})).cri_contextual is None
    with pytest.raises(ValueError, match='band_width'):
        _Bare.settings(dict(contextual_opt=dict(layer_weights=LAYERS, band_width=0)))
    with pytest.raises(NotImplementedError, match='batch-normalised'):
        _Bare.settings(dict(contextual_opt=dict(layer_weights=LAYERS, vgg_type='vgg16_bn')))


def test_graph_capture_is_not_asked_for_with_a_contextual_loss():
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    m = MultiRefRestorationModel.__new__(MultiRefRestorationModel)
    m.opt = dict(train=dict(hip_graph=True))
    assert m._train_graph_wanted()
    m.opt = dict(train=dict(hip_graph=True, contextual_opt=dict(layer_weights=LAYERS)))
    assert not m._train_graph_wanted()


def test_library_refuses_bad_shapes_before_any_launch():
    """host-side argument checks of csrc/contextual.hip (no GPU needed): the workspace of a shape, and error codes with messages"""
    import ctypes
    from mrefsr_amd import _lib
    from mrefsr_amd.hip import CX_MAX_N
    assert CX_MAX_N == 4096
    lib = _lib.load()
    ws = lib.mrefsr_contextual_workspace_bytes
    # mu | the N x ld distance matrix per sample, ld = N rounded up to 16 | (backward) dxn, each region 256-byte aligned
    assert ws(1, 2, 64, 0) == 256 + 256 and ws(1, 2, 64, 1) == 256 + 256 + 512
    assert ws(4, 1600, 256, 0) == 4 * 256 * 4 + 4 * 1600 * 1600 * 4 and ws(4, 1600, 256, 1) == ws(4, 1600, 256, 0) + 4 * 1600 * 256 * 4
    assert ws(2, 63, 64, 0) == 512 + 2 * 63 * 64 * 4 and ws(1, CX_MAX_N, 512, 0) > 0
    for b, n, c in ((0, 16, 64), (1, 1, 64), (1, 0, 64), (65536, 16, 64), (1, 16, 0)):
        assert ws(b, n, c, 0) == -1 and ws(b, n, c, 1) == -1
    for b, n, c in ((1, CX_MAX_N + 1, 64), (1, 16, 32), (1, 16, 96), (1, 16, 1024)):
        assert ws(b, n, c, 0) == -2 and ws(b, n, c, 1) == -2
    p = ctypes.c_void_p(16)
    big = ctypes.c_int64(1 << 40)

    def fwd(b, n, c, bw=0.5, x=p, nbytes=big):
        return lib.mrefsr_contextual_fwd_f32(x, p, b, n, c, bw, p, p, p, p, p, p, p, p, p, 1.0, 1.0, 1, p, p, p, nbytes, None)

    def bwd(b, n, c, bw=0.5, dx=p, nbytes=big):
        return lib.mrefsr_contextual_bwd_f32(p, p, p, b, n, c, bw, p, p, p, p, p, None, 1.0, dx, 0, None, p, nbytes, None)
    for call, name in ((fwd, b'contextual_fwd'), (bwd, b'contextual_bwd')):
        for b, n, c in ((0, 16, 64), (1, 1, 64)):
            assert call(b, n, c) == -1 and name in lib.mrefsr_last_error()
        for b, n, c in ((1, CX_MAX_N + 1, 256), (2, 16, 96)):
            assert call(b, n, c) == -2 and name in lib.mrefsr_last_error() and b'4096' in lib.mrefsr_last_error()
        for bw in (0.0, -1.0, float('inf'), float('nan')):
            assert call(1, 16, 64, bw=bw) == -1 and b'band_width' in lib.mrefsr_last_error()
        assert call(1, 16, 64, nbytes=ctypes.c_int64(100)) == -1 and b'workspace' in lib.mrefsr_last_error()
    assert fwd(1, 16, 64, x=None) == -1 and b'null' in lib.mrefsr_last_error()
    assert bwd(1, 16, 64, dx=None) == -1 and b'null' in lib.mrefsr_last_error()
    assert fwd(1, 16, 64, x=ctypes.c_void_p(20)) == -1 and b'aligned' in lib.mrefsr_last_error()


def test_python_side_names_the_bound():
    """hip._cx_workspace turns the library's refusal into the exceptions of the file: NotImplementedError with the bound for a tap
    that is too large, ValueError for a shape that is none"""
    from mrefsr_amd import hip
    with pytest.raises(NotImplementedError, match='at most 4096 positions'):
        hip._cx_workspace('contextual_fwd', 1, 4097, 256, False)
    with pytest.raises(NotImplementedError, match='64, 128, 256 or 512 channels'):
        hip._cx_workspace('contextual_bwd', 1, 100, 96, True)
    with pytest.raises(ValueError, match='N >= 2'):
        hip._cx_workspace('contextual_fwd', 1, 1, 64, False)
    assert hip._cx_workspace('contextual_fwd', 1, 4096, 64, False) > 0
