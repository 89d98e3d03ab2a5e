"""GPU: the channels-last reflect pad / crop kernels of csrc/pad.hip and their adjoints (MRAPAFusion's pad to a multiple of 4 and
crop back, ref_mrapa_restoration_arch.py:306-311, 348) against torch on the same tensors: the pad bit for bit against
F.pad(mode='reflect'), its adjoint against fp64 autograd of F.pad, the crop and its adjoint exactly."""
import pytest
import torch
import torch.nn.functional as F

from mrefsr_amd import hip
from mrefsr_amd._lib import MrefsrHipError

pytestmark = pytest.mark.gpu

PADS = [(0, 0), (0, 1), (1, 0), (2, 3), (3, 2), (1, 1), (3, 3), (0, 3), (2, 0)]
SHAPES = [(1, 5, 7, 64), (3, 13, 9, 256), (6, 4, 11, 64), (2, 19, 13, 256)]


def _ref_pad(x, ph, pw):
    """F.pad of the logical NCHW view, back to [N,H,W,C]"""
    return F.pad(x.permute(0, 3, 1, 2), [0, pw, 0, ph], mode='reflect').permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('pads', PADS, ids=lambda p: f'p{p[0]}{p[1]}')
def test_reflect_pad_is_f_pad_and_its_adjoint_is_fp64_autograd(shape, pads):
    ph, pw = pads
    n, h, w, c = shape
    torch.manual_seed(n * 1000 + h * 10 + ph * 4 + pw)
    x = torch.randn(shape, device='cuda')
    got = hip.reflect_pad_nhwc(x, ph, pw)
    assert torch.equal(got, _ref_pad(x, ph, pw))
    # adjoint: fp64 autograd of F.pad on the CPU (gradients with bf16 mantissas: the up to four terms of a pixel add up exactly in
    # fp32 unless their magnitudes lie 2^16 apart, so the comparison sees where each contribution went, not the rounding of the sum)
    g = torch.randn(tuple(got.shape), device='cuda').bfloat16().float()
    xr = x.double().cpu().requires_grad_()
    _ref_pad(xr, ph, pw).backward(g.double().cpu())
    gx = hip.reflect_pad_bwd_nhwc(g, ph, pw)
    assert gx.shape == x.shape
    want = xr.grad
    err = float((gx.double().cpu() - want).abs().max()) / float(want.abs().max())
    assert err <= 1e-7, err
    # (deterministic: no atomics)
    assert torch.equal(hip.reflect_pad_bwd_nhwc(g, ph, pw), gx)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('pads', PADS, ids=lambda p: f'p{p[0]}{p[1]}')
def test_crop_and_its_adjoint_are_exact_and_the_crop_measures_its_own_max(shape, pads):
    ph, pw = pads
    n, h, w, c = shape
    hp, wp = h + ph, w + pw
    torch.manual_seed(n * 1000 + h * 10 + ph * 4 + pw + 1)
    x = torch.randn((n, hp, wp, c), device='cuda')
    x[:, h:, :, 5] = 1e3                       # the band holds the source's maximum: the crop's word must not see it
    x[:, :, w:, 7] = -2e3
    slot = hip.amax_slot(x.device)
    got = hip.crop_nhwc(x, h, w, out_amax=slot)
    want = x[:, :h, :w, :]
    assert torch.equal(got, want)
    assert float(slot) == float(want.abs().max())
    assert hip.crop_nhwc(x, h, w).equal(want)  # (no word asked for)
    g = torch.randn((n, h, w, c), device='cuda')
    gx = hip.crop_bwd_nhwc(g, hp, wp)
    ref = torch.zeros_like(x)
    ref[:, :h, :w, :] = g
    assert torch.equal(gx, ref)


def test_refusals():
    x = torch.randn(2, 3, 5, 64, device='cuda')
    with pytest.raises(MrefsrHipError, match='need a map larger'):
        hip.reflect_pad_nhwc(x, 3, 0)                  # ph >= H (F.pad refuses it too)
    with pytest.raises(MrefsrHipError, match='need a map larger'):
        hip.reflect_pad_nhwc(torch.randn(2, 5, 2, 64, device='cuda'), 0, 2)   # pw >= W
    with pytest.raises(MrefsrHipError, match='pads'):
        hip.reflect_pad_nhwc(x, 4, 0)
    odd = torch.randn(2, 6, 5, 6, device='cuda')      # C % 4 != 0
    with pytest.raises(MrefsrHipError, match='multiple of 4'):
        hip.reflect_pad_nhwc(odd, 1, 1)
    with pytest.raises(MrefsrHipError, match='multiple of 4'):
        hip.reflect_pad_bwd_nhwc(odd, 1, 1)
    with pytest.raises(MrefsrHipError, match='multiple of 4'):
        hip.crop_nhwc(odd, 3, 3)
    with pytest.raises(MrefsrHipError, match='window'):
        hip.crop_nhwc(x, 4, 5)                         # window larger than the map
    with pytest.raises(MrefsrHipError, match='need a map larger'):
        hip.reflect_pad_bwd_nhwc(torch.randn(1, 4, 4, 64, device='cuda'), 2, 0)
