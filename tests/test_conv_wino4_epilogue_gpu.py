"""Output exchange and epilogue of conv_wino4_kernel (csrc/conv_wino4.hip): column fold of both output column parities from one
read of the accumulators, both tile items of a thread in flight together.  Everything is compared BITWISE with
conv_wino_kernel, the eight-wave kernel (MREFSR_WINO_WAVES=8), on the same inputs: the stored tensor (into a channel slice of a wider
one, ld_out > Cout, whose other channels stay untouched), the max |out| word and the range flag.

The shapes are the smallest at which this phase can go wrong: one tile (no previous tile's readers of the exchange buffer), several
tiles per block in a row (289 tiles on at most 256 blocks; 12 tiles x 2 cout blocks), Cin 64 / 128 (the shortest chunk loops: the
next tile's fragments and patch land while the exchange runs), Cout 64 / 128 (a second cout block: non-zero offsets into out, the
bias and the added tensor), every epilogue (plain, residual, pre broadcast over the batch, max-pool) with every activation (none,
slope 0.0, slope 0.1, a PReLU pointer).  All of them are below the size at which the launcher streams the output (256 MiB): they
run the cached store variant; the streamed one is the same source line with another cache policy and is run by
test_kernels_gpu.test_conv_wino4_is_bit_identical_to_the_eight_wave_kernel (30 x 320 x 320) and the benchmark-size tests."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from mrefsr_amd import hip as h
    return h


def _waves(n):
    if n is None:
        os.environ.pop('MREFSR_WINO_WAVES', None)
    else:
        os.environ['MREFSR_WINO_WAVES'] = str(n)


_ACTS = (('none', False, 0.0, False), ('relu', True, 0.0, False), ('leaky', True, 0.1, False), ('prelu', True, 0.0, True))


def _both(hip, x, pk, bias, co, variant, act, slope, prelu, margin):
    """one launch on each kernel -> [(out bits, untouched margin ok, amax bits, range flag)] for 8 and 4 waves"""
    n, h, w, _ = x.shape
    g = torch.Generator(device='cuda').manual_seed(n * 1000 + h + co)
    res = torch.randn(n, h, w, co, device='cuda', generator=g) if variant == 'residual' else None
    pre = torch.randn(1, h, w, co, device='cuda', generator=g) if variant == 'pre' else None   # pre_N = 1: broadcast over the batch
    sp = torch.full((1,), 0.25, device='cuda') if prelu else None
    ep = 1 if variant == 'pool' else 0
    ho, wo = (h // 2, w // 2) if ep else (h, w)
    got = []
    before = os.environ.get('MREFSR_WINO_WAVES')
    try:
        for nw in (8, 4):
            _waves(nw)
            hip.conv_range_tripped()
            wide = torch.full((n, ho, wo, co + 2 * margin), 7.0, device='cuda')
            out = wide[..., margin:margin + co] if margin else wide
            amax = hip.amax_slot(x.device)
            hip.conv_nhwc(x, pk, bias, co, 3, pre=pre, residual=res, act=act, slope=slope, slope_ptr=sp, epilogue=ep, out=out, out_amax=amax)
            flag = hip.conv_range_tripped()
            clean = bool((wide[..., :margin] == 7.0).all() and (wide[..., margin + co:] == 7.0).all()) if margin else True
            got.append((out.contiguous().view(torch.int32).clone(), clean, int(amax.view(torch.int32).item()), flag))
    finally:
        _waves(before)   # (the caller's own setting, if any, holds again)
    return got


def _same(got, what):
    (o8, c8, a8, f8), (o4, c4, a4, f4) = got
    assert c8 and c4, f'{what}: channels beside the slice were written'
    assert f8 == f4, f'{what}: range flag {f4} (four waves) against {f8}'
    if not f8:   # (a flagged launch is re-run by the caller: its values are not used)
        ndiff = int((o8 != o4).sum().item())
        assert ndiff == 0, f'{what}: {ndiff} of {o8.numel()} output words differ'
        assert a8 == a4, f'{what}: max |out| word {a4:#x} against {a8:#x}'
    return f8


def _weights(hip, ci, co, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    wt = torch.randn(co, ci, 3, 3, device='cuda', generator=g) / (3.0 * ci ** 0.5)
    return hip.conv_pack_weight(wt, 17), torch.randn(co, device='cuda', generator=g)


def test_one_tile(hip):
    """N = 1, 16 x 16: one tile per block, each block's only one"""
    for ci, co in ((64, 64), (128, 128)):
        pk, bias = _weights(hip, ci, co, 1)
        x = torch.randn(1, 16, 16, ci, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2))
        for variant in ('plain', 'residual', 'pre', 'pool'):
            for name, act, slope, prelu in _ACTS:
                assert not _same(_both(hip, x, pk, bias, co, variant, act, slope, prelu, 4), (ci, co, variant, name))


def test_more_tiles_than_blocks(hip):
    """N = 1, 272 x 272, 64 -> 64: 289 tiles, so some blocks run two tiles in a row -- the second tile's exchange overwrites the first
    one's while the next fragments land"""
    pk, bias = _weights(hip, 64, 64, 3)
    x = torch.randn(1, 272, 272, 64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(4))
    for variant, (name, act, slope, prelu), margin in (('plain', _ACTS[2], 0), ('residual', _ACTS[2], 4), ('pool', _ACTS[1], 4), ('pre', _ACTS[3], 0)):
        assert not _same(_both(hip, x, pk, bias, 64, variant, act, slope, prelu, margin), (variant, name, margin))


@pytest.mark.parametrize('variant', ['plain', 'residual', 'pre', 'pool'])
def test_channel_counts_and_activations(hip, variant):
    """N = 2, 48 x 32 (12 tiles x 1 or 2 cout blocks on 8 bands): Cin 64 / 128 x Cout 64 / 128 x every activation, dense and into a slice"""
    for ci in (64, 128):
        x = torch.randn(2, 48, 32, ci, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5 + ci))
        for co in (64, 128):
            pk, bias = _weights(hip, ci, co, 6 + ci + co)
            for k, (name, act, slope, prelu) in enumerate(_ACTS):
                assert not _same(_both(hip, x, pk, bias if k != 1 else None, co, variant, act, slope, prelu, 4 * (k & 1)), (ci, co, variant, name))


def test_range_guard(hip):
    """a value that leaves the fp16 range after the input transform raises the flag in both kernels; so do two activations of 4e4 two
    pixels apart on a tile's diagonal, which make ONE transform value (V[0][0] = 8e4) leave it: it enters a single output pixel of a
    pooled 2 x 2, and the maximum would drop its NaN -- the guard reads the tile before the maximum.  A launch inside the range leaves
    the flag down and is bitwise equal."""
    pk, bias = _weights(hip, 64, 64, 9)
    g = torch.Generator(device='cuda').manual_seed(10)
    for variant in ('plain', 'pool'):
        x = torch.randn(2, 48, 32, 64, device='cuda', generator=g).relu_()
        assert not _same(_both(hip, x, pk, bias, 64, variant, True, 0.0, False, 0), (variant, 'in range'))
        big = x.clone()
        big[1, 17, 29, 5] = 7.0e4
        assert _same(_both(hip, big, pk, bias, 64, variant, True, 0.0, False, 0), (variant, 'one value of 7e4'))
        diag = x.clone()
        diag[1, 15, 15, 5] = 4.0e4
        diag[1, 17, 17, 5] = 4.0e4
        assert _same(_both(hip, diag, pk, bias, 64, variant, True, 0.0, False, 0), (variant, 'two values of 4e4 on a diagonal'))
        assert not _same(_both(hip, x, pk, bias, 64, variant, True, 0.0, False, 0), (variant, 'in range again'))
