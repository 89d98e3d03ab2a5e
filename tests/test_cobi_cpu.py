"""CPU: CoBi, the contextual bilateral loss (Zhang et al., ICCV 2019) -- the spatial term of losses.contextual_loss_torch, the RGB
patch features losses.cx_patches_torch, the options ContextualLoss refuses, and the host-side checks of the library's new entry
points.  The GPU side: tests/test_cobi_kernels_gpu.py, tests/test_cobi_train_gpu.py."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

LAYERS = {'relu2_2': 1.0, 'relu3_1': 0.5}


def _fields(c, h, w, b, seed):
    """correlated feature maps (tests/test_contextual_cpu.py): a blurred rank-8 field mixed to c channels; y its top-left window,
    x the window one position down and right plus noise, both through a ReLU"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(b, 8, h + 1, w + 1, generator=g, dtype=torch.float64)
    z = F.avg_pool2d(F.pad(z, (2, 2, 2, 2), mode='replicate'), 5, 1) * 5
    f = torch.einsum('ck,bkhw->bchw', torch.randn(c, 8, generator=g, dtype=torch.float64), z)
    return F.relu(f[:, :, 1:, 1:] + 0.1 * torch.randn(b, c, h, w, generator=g, dtype=torch.float64)).contiguous(), \
        F.relu(f[:, :, :h, :w]).contiguous()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['fp32', 'fp64'])
def test_weight_sp_zero_is_the_plain_loss_bit_for_bit(dtype):
    from mrefsr_amd.losses import contextual_loss_torch
    x, y = _fields(16, 6, 5, 2, 0)
    x, y = x.to(dtype), y.to(dtype)
    outs = []
    for kw in ({}, dict(weight_sp=0.0), dict(weight_sp=0)):
        xr = x.clone().requires_grad_(True)
        loss, parts = contextual_loss_torch(xr, y, 0.5, parts=True, **kw)
        loss.backward()
        outs.append((loss.detach(), xr.grad, parts['d'], parts['cx'], parts['jmin'], parts['imax']))
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))


def test_the_spatial_term_as_spelled_out():
    """d = (1 - ws) d_cos + ws d_sp with d_sp = |p_i - p_j|^2 / (h^2 + w^2) on the map's grid, i = r w + c; d_sp in [0, 1)"""
    from mrefsr_amd.losses import contextual_loss_torch
    x, y = _fields(8, 3, 4, 1, 1)
    _, p0 = contextual_loss_torch(x, y, 0.5, parts=True)
    _, p1 = contextual_loss_torch(x, y, 0.5, parts=True, weight_sp=0.25)
    h, w = 3, 4
    dsp = torch.empty(h * w, h * w, dtype=torch.float64)
    for i in range(h * w):
        for j in range(h * w):
            dsp[i, j] = ((i // w - j // w) ** 2 + (i % w - j % w) ** 2) / (h * h + w * w)
    assert 0.0 == float(dsp.min()) and float(dsp.max()) == (2 * 2 + 3 * 3) / 25
    assert float((p1['d'][0] - (0.75 * p0['d'][0] + 0.25 * dsp)).abs().max()) <= 1e-15


def test_gradient_with_the_spatial_term_against_central_differences():
    """ws = 0.3 on a 5 x 7 grid, float64, 60 elements probed with step 1e-6, the tolerance of tests/test_contextual_cpu.py for the plain
    loss; the selections at x +- step are those at x (asserted)"""
    from mrefsr_amd.losses import contextual_loss_torch
    x, y = _fields(8, 5, 7, 2, 2)
    xr = x.clone().requires_grad_(True)
    loss, parts = contextual_loss_torch(xr, y, 0.5, parts=True, weight_sp=0.3)
    loss.backward()
    step, worst = 1e-6, 0.0
    for i in torch.randperm(x.numel(), generator=torch.Generator().manual_seed(3))[:60].tolist():
        vals = []
        for sgn in (1.0, -1.0):
            xs = x.clone().view(-1)
            xs[i] += sgn * step
            v, p = contextual_loss_torch(xs.view_as(x), y, 0.5, parts=True, weight_sp=0.3)
            assert torch.equal(p['jmin'], parts['jmin']) and torch.equal(p['imax'], parts['imax'])
            vals.append(float(v))
        worst = max(worst, abs((vals[0] - vals[1]) / (2 * step) - float(xr.grad.view(-1)[i])))
    print(f'ws 0.3: max |central difference - autograd| = {worst:.2e}, max |grad| = {float(xr.grad.abs().max()):.2e}')
    assert float(xr.grad.abs().max()) > 1e-4 and worst <= 1e-7 * max(1.0, float(xr.grad.abs().max()))


def test_transposing_both_maps_leaves_the_loss():
    """an h x w grid becomes w x h: the pairs and their squared offsets are the same, r and c swapped"""
    from mrefsr_amd.losses import contextual_loss_torch
    x, y = _fields(8, 5, 7, 2, 4)
    a = contextual_loss_torch(x, y, 0.5, weight_sp=0.3)
    b = contextual_loss_torch(x.transpose(2, 3).contiguous(), y.transpose(2, 3).contiguous(), 0.5, weight_sp=0.3)
    assert abs(float(a) - float(b)) <= 1e-12
    # (and the term is there: the plain loss is another number)
    assert abs(float(a) - float(contextual_loss_torch(x, y, 0.5))) > 1e-3


@pytest.mark.parametrize('h,w,size,stride', [(17, 14, 3, 2), (23, 19, 5, 3), (20, 26, 5, 2), (24, 24, 7, 4), (6, 5, 1, 1), (13, 13, 13, 1)])
def test_patches_are_unfold(h, w, size, stride):
    from mrefsr_amd.losses import cx_patches_torch
    img = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(h))
    oh, ow = (h - size) // stride + 1, (w - size) // stride + 1
    p = cx_patches_torch(img, size, stride)
    assert p.shape == (2, 3 * size * size, oh, ow)
    assert torch.equal(p, F.unfold(img, size, stride=stride).reshape(2, 3 * size * size, oh, ow))


def test_options_refused():
    from mrefsr_amd.losses import ContextualLoss, build_loss, contextual_loss_torch, cx_patches_torch
    cri = build_loss(dict(type='ContextualLoss', layer_weights=LAYERS, weight_sp=0.1, tap_stride={'relu2_2': 2},
                          rgb_patch=dict(size=5, stride=4, weight=0.5)))
    assert (cri.weight_sp, cri.tap_stride, cri.rgb_patch) == (0.1, {'relu2_2': 2}, dict(size=5, stride=4, weight=0.5))
    plain = ContextualLoss(LAYERS)
    assert (plain.weight_sp, plain.tap_stride, plain.rgb_patch) == (0.0, {}, None)
    for bad in (-0.1, 1.0, 1.5, float('nan'), float('inf'), 'a', None, True):
        with pytest.raises(ValueError, match='weight_sp'):
            ContextualLoss(LAYERS, weight_sp=bad)
        with pytest.raises(ValueError, match='weight_sp'):
            contextual_loss_torch(torch.rand(1, 8, 4, 4), torch.rand(1, 8, 4, 4), weight_sp=bad)
    for bad in ({'relu2_2': 0}, {'relu2_2': 1.5}, {'relu2_2': True}, {'relu2_2': None}):
        with pytest.raises(ValueError, match='tap relu2_2'):
            ContextualLoss(LAYERS, tap_stride=bad)
    for bad in ({'relu5_1': 2}, [2], 2):
        with pytest.raises(ValueError, match='tap_stride'):
            ContextualLoss(LAYERS, tap_stride=bad)
    for bad in (dict(size=0, stride=1), dict(size=2.0, stride=1), dict(size=3, stride=0), dict(size=3, stride='2'), dict(size=True)):
        with pytest.raises(ValueError, match='tap rgb_patch'):
            ContextualLoss(LAYERS, rgb_patch=bad)
    for bad in (dict(stride=2), dict(size=3, step=2), [3, 2], 3):
        with pytest.raises(ValueError, match='rgb_patch'):
            ContextualLoss(LAYERS, rgb_patch=bad)
    with pytest.raises(NotImplementedError, match='tap rgb_patch.*588 channels'):
        ContextualLoss(LAYERS, rgb_patch=dict(size=14, stride=4))
    assert ContextualLoss({}, rgb_patch=dict(size=13, stride=4)).rgb_patch == dict(size=13, stride=4, weight=1.0)
    # empty layer_weights: allowed with rgb_patch (no VGG is built), still refused without
    alone = ContextualLoss({}, rgb_patch=dict(size=5, stride=4))
    assert alone.vgg is None and not list(alone.parameters()) and not alone.state_dict()
    for bad in ({}, None, ['relu2_2']):
        with pytest.raises(ValueError, match='layer_weights'):
            ContextualLoss(bad)
    with pytest.raises(ValueError, match='layer_weights'):
        ContextualLoss(None, rgb_patch=dict(size=5, stride=4))
    with pytest.raises(NotImplementedError, match='no CPU path'):
        alone(torch.rand(1, 3, 32, 32), torch.rand(1, 3, 32, 32))
    for size, stride in ((0, 1), (3, 0), (2.0, 1)):
        with pytest.raises(ValueError, match='cx_patches_torch'):
            cx_patches_torch(torch.rand(1, 3, 8, 8), size, stride)
    with pytest.raises(ValueError, match='cx_patches_torch'):
        cx_patches_torch(torch.rand(1, 3, 4, 8), 5, 1)
    with pytest.raises(ValueError, match='cx_patches_torch'):
        cx_patches_torch(torch.rand(1, 1, 8, 8), 3, 1)


def test_plan_carries_the_new_fields():
    from mrefsr_amd.archs.nhwc_train import ContextualLossPlan
    from mrefsr_amd.losses import ContextualLoss
    cri = ContextualLoss({'relu3_1': 0.5, 'relu2_2': 1.0}, weight_sp=0.1, tap_stride={'relu2_2': 2}, rgb_patch=dict(size=5, stride=4, weight=2.0))
    plan = ContextualLossPlan(cri.vgg.vgg_net, cri.layer_weights, 0.5, 0.1, False, weight_sp=cri.weight_sp, tap_stride=cri.tap_stride,
                              rgb_patch=cri.rgb_patch)
    assert plan.names == ['relu2_2', 'relu3_1'] and plan.strides == [2, 1] and plan.weight_sp == 0.1
    assert plan.rgb == dict(size=5, stride=4, weight=2.0)
    old = ContextualLossPlan(cri.vgg.vgg_net, cri.layer_weights, 0.5, 0.1, False)
    assert old.strides == [1, 1] and old.weight_sp == 0.0 and old.rgb is None
    bare = ContextualLossPlan(None, {}, 0.5, 1.0, True, rgb_patch=dict(size=3, stride=2, weight=1.0))
    assert bare.taps == [] and bare.layers == [] and bare.names == [] and bare.norm_img
    with pytest.raises(ValueError, match='no tap'):
        ContextualLossPlan(None, {}, 0.5, 1.0, False)


def test_model_passes_the_new_keys_through():
    from test_losses_cpu import _Bare
    opt = dict(layer_weights=dict(LAYERS), weight_sp=0.1, tap_stride={'relu2_2': 2}, rgb_patch=dict(size=5, stride=4, weight=1.0))
    m = _Bare.settings(dict(contextual_opt=opt))
    assert (m.cri_contextual.weight_sp, m.cri_contextual.tap_stride, m.cri_contextual.rgb_patch) == (0.1, {'relu2_2': 2}, opt['rgb_patch'])
    with pytest.raises(ValueError, match='weight_sp'):
        _Bare.settings(dict(contextual_opt=dict(layer_weights=LAYERS, weight_sp=1.0)))


def test_library_refuses_bad_arguments_before_any_launch():
    """host-side checks of the new entry points (no GPU needed): error codes with messages"""
    from mrefsr_amd import _lib
    from mrefsr_amd.hip import CX_MAX_N
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    big = ctypes.c_int64(1 << 40)

    def fwd(b, h, w, c, bw=0.5, ws=0.1, x=p, nbytes=big):
        return lib.mrefsr_contextual_fwd_sp_f32(x, p, b, h, w, c, bw, ws, p, p, p, p, p, p, p, p, p, 1.0, 1.0, 1, p, p, p, nbytes, None)

    def bwd(b, h, w, c, bw=0.5, ws=0.1, dx=p, nbytes=big):
        return lib.mrefsr_contextual_bwd_sp_f32(p, p, p, b, h, w, c, bw, ws, p, p, p, p, p, None, 1.0, dx, 0, None, p, nbytes, None)
    for call, name in ((fwd, b'contextual_fwd_sp'), (bwd, b'contextual_bwd_sp')):
        for b, h, w, c in ((0, 4, 4, 64), (1, 1, 1, 64), (1, 0, 4, 64), (1, 4, -1, 64), (65536, 4, 4, 64), (1, 4, 4, 0)):
            assert call(b, h, w, c) == -1 and name in lib.mrefsr_last_error()
        for b, h, w, c in ((1, 64, 65, 256), (1, 1, CX_MAX_N + 1, 64), (1, 1 << 16, 1 << 16, 64), (2, 4, 4, 96)):
            assert call(b, h, w, c) == -2 and name in lib.mrefsr_last_error() and b'4096' in lib.mrefsr_last_error()
        for ws in (-0.1, 1.0, 2.0, float('inf'), float('nan')):
            assert call(1, 4, 4, 64, ws=ws) == -1 and b'weight_sp' in lib.mrefsr_last_error()
        for bw in (0.0, -1.0, float('inf'), float('nan')):
            assert call(1, 4, 4, 64, bw=bw) == -1 and b'band_width' in lib.mrefsr_last_error()
        assert call(1, 4, 4, 64, nbytes=ctypes.c_int64(100)) == -1 and b'workspace' in lib.mrefsr_last_error()
    assert fwd(1, 4, 4, 64, x=None) == -1 and b'null' in lib.mrefsr_last_error()
    assert bwd(1, 4, 4, 64, dx=None) == -1 and b'null' in lib.mrefsr_last_error()
    assert fwd(1, 4, 4, 64, x=ctypes.c_void_p(20)) == -1 and b'aligned' in lib.mrefsr_last_error()
    # patches: Cpad is the smallest of 64 / 128 / 256 / 512 that holds 3 size^2
    ch = lib.mrefsr_cx_patch_channels
    assert [ch(s) for s in range(1, 14)] == [64, 64, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512]
    assert ch(0) == -1 and ch(-3) == -1 and ch(14) == -2
    pf = lib.mrefsr_cx_patches_f32
    pb = lib.mrefsr_cx_patches_bwd_f32
    for args in ((0, 8, 8, 3, 1, 64), (1, 8, 8, 0, 1, 64), (1, 8, 8, 3, 0, 64), (1, 2, 8, 3, 1, 64), (1, 8, 8, 3, 1, 128), (1, 8, 8, 5, 1, 64)):
        b, h, w, size, stride, cpad = args
        assert pf(p, b, h, w, size, stride, 0, p, cpad, None) == -1 and b'cx_patches' in lib.mrefsr_last_error()
        assert pb(p, b, h, w, size, stride, cpad, 1.0, p, 0, None) == -1 and b'cx_patches_bwd' in lib.mrefsr_last_error()
    assert pf(p, 1, 32, 32, 14, 1, 0, p, 512, None) == -2 and pb(p, 1, 32, 32, 14, 1, 512, 1.0, p, 0, None) == -2
    assert pf(None, 1, 8, 8, 3, 1, 0, p, 64, None) == -1 and b'null' in lib.mrefsr_last_error()
    assert pf(p, 1, 8, 8, 3, 1, 0, ctypes.c_void_p(20), 64, None) == -1 and b'aligned' in lib.mrefsr_last_error()
    sf, sb = lib.mrefsr_cx_subsample_f32, lib.mrefsr_cx_subsample_bwd_f32
    for b, h, w, c, s in ((0, 4, 4, 64, 2), (1, 0, 4, 64, 2), (1, 4, 4, 6, 2), (1, 4, 4, 64, 0)):
        assert sf(p, b, h, w, c, s, p, None) == -1 and b'cx_subsample' in lib.mrefsr_last_error()
        assert sb(p, b, h, w, c, s, p, 0, None, None) == -1 and b'cx_subsample_bwd' in lib.mrefsr_last_error()
    assert sf(p, 1, 4, 4, 64, 2, None, None) == -1 and b'null' in lib.mrefsr_last_error()
    assert sb(ctypes.c_void_p(20), 1, 4, 4, 64, 2, p, 0, None, None) == -1 and b'aligned' in lib.mrefsr_last_error()


def test_python_side_refusals():
    from mrefsr_amd import hip
    t = torch.zeros(1, 3, 8, 8)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match='size'):
            hip.cx_patch_channels(bad)
    with pytest.raises(NotImplementedError, match='588 channels'):
        hip.cx_patch_channels(14)
    assert hip.cx_patch_channels(5) == 128
    with pytest.raises(NotImplementedError, match='no CPU path'):
        hip.cx_patches(t, 3, 2)
    with pytest.raises(NotImplementedError, match='no CPU path'):
        hip.cx_subsample(torch.zeros(1, 4, 4, 64), 2)
    for bad in (-0.5, 1.0, 'x', None):
        with pytest.raises(ValueError, match='weight_sp'):
            hip._cx_weight_sp('contextual_fwd', bad)
