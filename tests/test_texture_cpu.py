"""No GPU: the texture loss (train.texture_opt) -- how the model builds it, what it still refuses, TextureLoss's registry entry,
signature and state-dict keys, and the invariants of the torch restatement of the swapped maps that the GPU tests use
as their yardstick."""
import inspect

import pytest
import torch

from test_losses_cpu import _Bare


# ---- the restatement of selection and patch swap: the yardstick of tests/test_texture_kernels_gpu.py ------------------------------
def select(idx, val, valid):                    # idx, val [K,B,gh,gw]; valid [B,K] bool
    v = val.masked_fill(~valid.t()[:, :, None, None], float('-inf'))
    wts = v.max(0).values
    sel = (v == wts[None]).float().argmax(0)    # lowest k among the maxima
    return sel, wts, torch.gather(idx, 0, sel[None])[0]


def swap(feat, sel, pidx, s, h, w, probe=None):  # feat [K,B,C,s*h,s*w] -> [B,C,s*h,s*w]
    K, B, C = feat.shape[:3]
    gh, gw = h - 2, w - 2
    acc = feat.new_zeros(B, C, s * h, s * w)
    cnt = feat.new_zeros(1, 1, s * h, s * w)
    Y = torch.arange(s * h, device=feat.device)[:, None].expand(s * h, s * w)
    X = torch.arange(s * w, device=feat.device)[None].expand(s * h, s * w)
    bb = torch.arange(B, device=feat.device)[:, None, None]
    for dy in (2, 1, 0):                        # ascending y = Y//s - dy, then ascending x
        for dx in (2, 1, 0):
            y, x = Y // s - dy, X // s - dx
            ok = (y >= 0) & (y < gh) & (x >= 0) & (x < gw)
            yc, xc = y.clamp(0, gh - 1), x.clamp(0, gw - 1)
            k, p = sel[:, yc, xc], pidx[:, yc, xc]
            sy_raw, sx_raw = s * (p // gw) + (Y - s * y), s * (p % gw) + (X - s * x)
            if probe is not None:               # (the unclamped source indices and selected references of the terms that count)
                probe.append((ok, sy_raw, sx_raw, k))
            sy, sx = sy_raw.clamp(0, s * h - 1), sx_raw.clamp(0, s * w - 1)
            g = feat[k, bb, :, sy, sx].permute(0, 3, 1, 2)
            acc = acc + torch.where(ok[None, None], g, g.new_zeros(()))
            cnt = cnt + ok[None, None].to(feat.dtype)
    if probe is not None:
        probe.append(cnt)
    return acc / cnt


def test_model_builds_the_texture_criterion():
    from mrefsr_amd.losses import TextureLoss
    m = _Bare.settings(dict(texture_opt=dict(use_weights=True, loss_weight=1e-3)))
    assert isinstance(m.cri_texture, TextureLoss) and m.cri_texture.loss_weight == 1e-3 and m.cri_texture.use_weights is True
    assert _Bare.settings({}).cri_texture is None


def test_model_refuses_texture_opt_without_use_weights():
    for opt in (dict(loss_weight=1.0), dict(loss_weight=1.0, use_weights=False)):
        with pytest.raises(NotImplementedError, match='texture_opt') as e:
            _Bare.settings(dict(texture_opt=opt))
        assert 'use_weights: true' in str(e.value)


def test_texture_loss_registry_signature_and_state_dict():
    from mrefsr_amd import losses
    from mrefsr_amd.losses import LOSS_REGISTRY, TextureLoss, build_loss
    assert LOSS_REGISTRY.get('TextureLoss') is TextureLoss and 'TextureLoss' in losses.__all__
    sig = inspect.signature(TextureLoss.__init__)
    assert list(sig.parameters) == ['self', 'use_weights', 'loss_weight', 'vgg_type', 'layer_weights', 'use_input_norm']
    d = {k: p.default for k, p in sig.parameters.items() if k != 'self'}
    assert d == dict(use_weights=False, loss_weight=1.0, vgg_type='vgg19', layer_weights={'relu1_1': 1.0, 'relu2_1': 1.0, 'relu3_1': 1.0},
                     use_input_norm=True)
    assert list(inspect.signature(TextureLoss.forward).parameters) == ['self', 'x', 'maps', 'weights']
    cri = build_loss(dict(type='TextureLoss', use_weights=True))
    convs = ['conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1']
    assert sorted(cri.state_dict()) == sorted(['vgg.mean', 'vgg.std'] + [f'vgg.vgg_net.{c}.{p}' for c in convs for p in ('weight', 'bias')])
    assert all(not p.requires_grad for p in cri.parameters())


def test_texture_loss_refusals():
    from mrefsr_amd.losses import TextureLoss
    with pytest.raises(NotImplementedError, match='use_weights'):
        TextureLoss()
    with pytest.raises(NotImplementedError, match='relu4_1'):
        TextureLoss(use_weights=True, layer_weights={'relu3_1': 1.0, 'relu4_1': 1.0})
    with pytest.raises(NotImplementedError, match='vgg19_bn'):
        TextureLoss(use_weights=True, vgg_type='vgg19_bn')
    cri = TextureLoss(use_weights=True)
    x, maps = torch.zeros(1, 3, 16, 16), {k: torch.zeros(1, 1, 1, 1) for k in ('relu1_1', 'relu2_1', 'relu3_1')}
    with pytest.raises(NotImplementedError, match='dict'):
        cri(x, maps, {k: torch.zeros(1, 1, 2, 2) for k in maps})
    with pytest.raises(NotImplementedError, match='CPU'):
        cri(x, maps, torch.zeros(1, 1, 2, 2))


def test_graph_step_is_not_wanted_with_texture_opt():
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    m = MultiRefRestorationModel.__new__(MultiRefRestorationModel)
    m.opt = dict(train=dict(hip_graph=True))
    assert m._train_graph_wanted()
    m.opt = dict(train=dict(hip_graph=True, texture_opt=dict(use_weights=True)))
    assert not m._train_graph_wanted()


def test_want_val_defaults_to_off():
    from mrefsr_amd.archs.corres_generation_arch import CorrespondenceGenerationArch
    from mrefsr_amd.archs.ref_map_util import match_normalised_batch
    assert inspect.signature(match_normalised_batch).parameters['want_val'].default is False
    assert inspect.signature(CorrespondenceGenerationArch.offsets).parameters['want_val'].default is False


@pytest.mark.parametrize('s', [1, 2, 4])
def test_restatement_invariants(s):
    K, B, h, w, C = 3, 2, 12, 8, 4
    gh, gw = h - 2, w - 2
    g = torch.Generator().manual_seed(s)
    idx = torch.randint(0, gh * gw, (K, B, gh, gw), generator=g)
    idx[0, 0, 0, 0], idx[1, 1, -1, -1], idx[2, 0, 3, 3] = 0, gh * gw - 1, gh * gw - 1
    val = torch.rand(K, B, gh, gw, generator=g) * 3
    val[1, :, 2] = val[0, :, 2]                       # ties: the lowest k wins
    val[2, 1] = 5.0                                   # the absent reference would win everywhere
    valid = torch.tensor([[True, True, True], [True, True, False]])
    sel, wts, pidx = select(idx, val, valid)
    assert not bool((sel[1] == 2).any()) and bool((sel[0, 2] != 1).all())
    assert torch.equal(wts, torch.where(valid.t()[:, :, None, None], val, val.new_full((), float('-inf'))).max(0).values)
    assert torch.equal(pidx, torch.gather(idx, 0, sel[None])[0])
    feat = torch.rand(K, B, C, s * h, s * w, generator=g)
    probe = []
    out = swap(feat, sel, pidx, s, h, w, probe=probe)
    cnt = probe.pop()
    assert float(cnt.min()) >= 1 and float(cnt.max()) == 9 and set(cnt.flatten().tolist()) == {1., 2., 3., 4., 6., 9.}
    for ok, sy, sx, k in probe:
        okb = ok[None].expand_as(sy)
        assert int(sy[okb].min()) >= 0 and int(sy[okb].max()) < s * h and int(sx[okb].min()) >= 0 and int(sx[okb].max()) < s * w
        assert not bool((k[1][ok] == 2).any())
    assert out.shape == (B, C, s * h, s * w) and bool(torch.isfinite(out).all())
    # identity: every position matched to itself reproduces the reference map
    own = torch.arange(gh * gw).view(1, gh, gw).expand(B, gh, gw)
    ident = swap(feat[:1], torch.zeros(B, gh, gw, dtype=torch.long), own, s, h, w)
    assert float(((ident - feat[0]).abs() / feat[0].abs().clamp_min(1e-30)).max()) <= 1e-6


def test_library_refuses_a_batch_beyond_the_grid_limit_by_name():
    """host-side check of the three Gram launchers (no GPU needed): N is gridDim.z, so N = 65536 is an invalid argument with a
    message that names the function, not a launch failure"""
    import ctypes
    from mrefsr_amd import _lib
    lib = _lib.load()
    p, n, big = ctypes.c_void_p(16), 65536, ctypes.c_int64(1 << 50)
    calls = ((b'gram_nhwc', lambda: lib.mrefsr_gram_nhwc_scaled_f32(p, n, 9, 64, 1.0, p, p, big, None)),
             (b'gram_bwd_nhwc', lambda: lib.mrefsr_gram_bwd_nhwc_f32(p, p, p, p, n, 9, 64, None, 1.0, 1.0, 0, None, None)),
             (b'texture_gram_bwd_nhwc', lambda: lib.mrefsr_texture_gram_bwd_nhwc_f32(p, p, p, p, p, None, p, n, 9, 64, 1.0, 0, None, None)))
    for name, call in calls:
        assert call() == -1, name                       # MREFSR_E_INVALID
        msg = lib.mrefsr_last_error()
        assert msg.startswith(name + b':') and b'N=65536' in msg, msg
