"""No GPU: val.color_fix -- the option parser, the torch statements of the two operators (mrefsr_amd/color_fix.py) against
independent restatements written here, the valid rectangles, and the C entries' argument checks.

The wavelet operator is checked in float64 against two forms: high_L(x) + low_L(s) with F.pad(mode='replicate') and a dilated
depthwise F.conv2d per stage, and x + A_h (s - x) A_w^T with the composite matrices A_n = S_{2^(L-1)} ... S_2 S_1 of the separable
filter (S_r: 1/4, 1/2, 1/4 at columns clamp(y - r), y, clamp(y + r)); both to 1e-14."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from mrefsr_amd.color_fix import (adain_color_fix_torch, color_fix, parse_color_fix, wavelet_color_fix_torch)

SIZES = [(1, 1), (5, 7), (33, 70), (64, 95)]
LEVELS = (1, 3, 5)
B, C = 2, 3


def _inputs(h, w, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, h, w, generator=g, dtype=torch.float64) * 1.2 - 0.1   # the output: [-0.1, 1.1]
    s = torch.rand(B, C, h, w, generator=g, dtype=torch.float64)               # the colour source: [0, 1]
    return x.to(dtype), s.to(dtype)


# ------------------------------------------------------------------------------------------------ the option
@pytest.mark.parametrize('val_opt', [None, {}, dict(save_img=False), dict(color_fix=None), dict(color_fix=False)])
def test_option_absent_none_or_false_is_off(val_opt):
    assert parse_color_fix(val_opt) is None


@pytest.mark.parametrize('spelling, want', [
    ('wavelet', dict(type='wavelet', levels=5)),
    (dict(type='wavelet'), dict(type='wavelet', levels=5)),
    (dict(type='wavelet', levels=1), dict(type='wavelet', levels=1)),
    (dict(type='wavelet', levels=3), dict(type='wavelet', levels=3)),
    (dict(type='wavelet', levels=5), dict(type='wavelet', levels=5)),
    ('adain', dict(type='adain')),
    (dict(type='adain'), dict(type='adain')),
])
def test_accepted_spellings(spelling, want):
    assert parse_color_fix(dict(color_fix=spelling)) == want


@pytest.mark.parametrize('bad', [
    True, 1, 5, 0.5, ['wavelet'], 'Wavelet', 'histogram', '', dict(), dict(levels=3), dict(type='histogram'), dict(type=None),
    dict(type=['wavelet']), dict(type='wavelet', level=3), dict(type='wavelet', levels=3, clamp=True), dict(type='adain', levels=5),
    dict(type='adain', levels=None), dict(type='wavelet', levels=0), dict(type='wavelet', levels=6), dict(type='wavelet', levels=-1),
    dict(type='wavelet', levels=2.0), dict(type='wavelet', levels='3'), dict(type='wavelet', levels=True),
    dict(type='wavelet', levels=False), dict(type='wavelet', levels=None), dict(type='wavelet', levels=[3]),
], ids=repr)
def test_everything_else_is_refused_by_name(bad):
    with pytest.raises(ValueError, match=r'val\.color_fix'):
        parse_color_fix(dict(color_fix=bad))


def test_the_models_refuse_a_bad_option_at_construction_before_anything_is_built():
    """next to check_self_ensemble: no network is built, no device is asked for"""
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel, RefRestorationModel
    for cls in (MultiRefRestorationModel, RefRestorationModel):
        with pytest.raises(ValueError, match=r'val\.color_fix\.levels'):
            cls(dict(num_gpu=1, is_train=False, val=dict(color_fix=dict(type='wavelet', levels=9))))
        with pytest.raises(ValueError, match=r'val\.color_fix'):
            cls(dict(num_gpu=1, is_train=False, val=dict(color_fix=True)))


def test_feed_data_reads_the_valid_sizes_from_padding_and_original_size():
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    sizes_of = MultiRefRestorationModel._valid_sizes_of
    lq = torch.zeros(2, 3, 4, 5)
    assert sizes_of(dict(img_in_lq=lq)) is None
    assert sizes_of(dict(img_in_lq=lq, original_size=(10, 12))) is None
    assert sizes_of(dict(img_in_lq=lq, padding=False, original_size=(10, 12))) is None
    assert sizes_of(dict(img_in_lq=lq, padding=True, original_size=(10, 12))) == [[10, 12], [10, 12]]
    assert sizes_of(dict(img_in_lq=lq[:1], padding=True, original_size=[10, 12, 3])) == [[10, 12]]
    # what a DataLoader makes of the dataset's `'padding': True, 'original_size': (h, w)`
    collated = dict(img_in_lq=lq, padding=torch.tensor([True, True]), original_size=[torch.tensor([10, 11]), torch.tensor([12, 13])])
    assert sizes_of(collated) == [[10, 12], [11, 13]]
    with pytest.raises(ValueError, match='original_size'):
        sizes_of(dict(img_in_lq=lq, padding=True, original_size=[torch.tensor([10, 11, 12]), torch.tensor([12, 13, 14])]))


# ------------------------------------------------------------------------------------------------ wavelet
def _low_conv(v, levels):
    """low_L by replicate padding and a dilated depthwise convolution per stage"""
    k1 = torch.tensor([1., 2., 1.], dtype=v.dtype)
    k = (k1[:, None] * k1[None, :] / 16.).expand(v.shape[1], 1, 3, 3).contiguous()
    for i in range(levels):
        r = 1 << i
        v = F.conv2d(F.pad(v, (r, r, r, r), mode='replicate'), k, dilation=r, groups=v.shape[1])
    return v


def _stage_matrix(n, r):
    s = torch.zeros(n, n, dtype=torch.float64)
    for y in range(n):
        s[y, max(y - r, 0)] += 0.25
        s[y, y] += 0.5
        s[y, min(y + r, n - 1)] += 0.25
    return s


def _composite(n, levels):
    """A_n = S_{2^(L-1)} ... S_2 S_1"""
    a = torch.eye(n, dtype=torch.float64)
    for i in range(levels):
        a = _stage_matrix(n, 1 << i) @ a
    return a


@pytest.mark.parametrize('levels', LEVELS)
@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_wavelet_equals_both_restatements(size, levels):
    h, w = size
    x, s = _inputs(h, w, seed=17 * h + w)
    got = wavelet_color_fix_torch(x, s, levels=levels)
    assert got.dtype == torch.float64 and got.shape == x.shape
    by_conv = (x - _low_conv(x, levels)) + _low_conv(s, levels)                   # high_L(x) + low_L(s)
    a_h, a_w = _composite(h, levels), _composite(w, levels)
    by_matrix = x + a_h @ (s - x) @ a_w.T
    assert float((got - by_conv).abs().max()) <= 1e-14
    assert float((got - by_matrix).abs().max()) <= 1e-14
    if (h, w) != (1, 1):
        assert float((got - x).abs().max()) > 1e-3, 'the fix would be indistinguishable from x: the test shows nothing'


def test_composite_matrix_facts():
    """every entry of A_n a non-negative multiple of 2^-10 (L = 5), rows summing to exactly 1 and zero outside |j - y| <= 2^L - 1"""
    for n in (5, 33, 70, 95):
        a = _composite(n, 5)
        assert torch.equal(a * 1024, (a * 1024).round()) and bool((a >= 0).all())
        assert torch.equal(a.sum(1), torch.ones(n, dtype=torch.float64))
        j, y = torch.arange(n)[None, :], torch.arange(n)[:, None]
        assert bool((a[(j - y).abs() > 31] == 0).all())
        assert torch.equal(a.float().double(), a)


def test_wavelet_default_levels_is_five_and_bad_levels_are_refused():
    x, s = _inputs(33, 70, seed=3)
    assert torch.equal(wavelet_color_fix_torch(x, s), wavelet_color_fix_torch(x, s, levels=5))
    for bad in (0, 6, True, 2.0, None):
        with pytest.raises(ValueError, match='levels'):
            wavelet_color_fix_torch(x, s, levels=bad)


def test_wavelet_with_the_source_equal_to_x_returns_x():
    x, _ = _inputs(33, 70, seed=4, dtype=torch.float32)
    assert torch.equal(wavelet_color_fix_torch(x, x.clone()), x)


# ------------------------------------------------------------------------------------------------ adain
def _adain_formula(x, s):
    out = torch.empty_like(x)
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            px, ps = x[b, c], s[b, c]
            sig_x = (px.reshape(-1).var(unbiased=True) + 1e-5).sqrt()
            sig_s = (ps.reshape(-1).var(unbiased=True) + 1e-5).sqrt()
            out[b, c] = (px - px.mean()) * (sig_s / sig_x) + ps.mean()
    return out


@pytest.mark.parametrize('size', [(2, 1), (5, 7), (33, 70), (64, 95)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_adain_equals_the_formula(size):
    h, w = size
    x, s = _inputs(h, w, seed=29 * h + w)
    got = adain_color_fix_torch(x, s)
    want = _adain_formula(x, s)
    assert float((got - want).abs().max()) <= 1e-13
    # the statistics of the result are the source's (up to the 1e-5 under the roots)
    assert float((got.mean((2, 3)) - s.mean((2, 3))).abs().max()) <= 1e-12


def test_adain_refuses_a_rectangle_of_one_pixel_by_name():
    x, s = _inputs(1, 1, seed=5)
    with pytest.raises(ValueError, match='1 pixel'):
        adain_color_fix_torch(x, s)
    x, s = _inputs(5, 7, seed=5)
    with pytest.raises(ValueError, match='1 pixel'):
        adain_color_fix_torch(x, s, sizes=[(5, 7), (1, 1)])


# ------------------------------------------------------------------------------------------------ sizes
def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize('kind', ['wavelet', 'adain'])
def test_sizes_restrict_everything_to_the_rectangle(kind):
    fn = (lambda x, s, sizes=None: wavelet_color_fix_torch(x, s, sizes, levels=3)) if kind == 'wavelet' else adain_color_fix_torch
    h, w = 33, 70
    x, s = _inputs(h, w, seed=6)
    x[0, 0, -1, -1] = float('nan')   # outside every rectangle below: it keeps its bits and reaches nothing inside
    sizes = [(30, 65), (7, 70)]
    got = fn(x, s, sizes)
    for b, (hb, wb) in enumerate(sizes):
        inside = torch.zeros(h, w, dtype=torch.bool)
        inside[:hb, :wb] = True
        assert torch.equal(_bits(got[b])[:, ~inside], _bits(x[b])[:, ~inside])
        crop = fn(x[b:b + 1, :, :hb, :wb].contiguous(), s[b:b + 1, :, :hb, :wb].contiguous())
        assert torch.equal(got[b:b + 1, :, :hb, :wb], crop)
        assert bool(torch.isfinite(crop).all()) and float((crop - x[b:b + 1, :, :hb, :wb]).abs().max()) > 1e-3
    full = fn(x[1:], s[1:], [(h, w)])
    assert torch.equal(full, fn(x[1:], s[1:]))
    for bad in ([(30, 65)], [(30, 65), (0, 70)], [(30, 65), (34, 70)], [(30, 65), (7, 71)]):
        with pytest.raises(ValueError, match='sizes'):
            fn(x, s, bad)


def test_dispatcher_takes_cpu_tensors_to_the_torch_forms():
    x, s = _inputs(33, 70, seed=7, dtype=torch.float32)
    assert color_fix(x, s, None) is x
    assert torch.equal(color_fix(x, s, dict(type='wavelet', levels=2)), wavelet_color_fix_torch(x, s, levels=2))
    assert torch.equal(color_fix(x, s, dict(type='adain'), [(30, 65), (7, 70)]), adain_color_fix_torch(x, s, [(30, 65), (7, 70)]))


def test_the_hip_bindings_refuse_cpu_tensors():
    from mrefsr_amd import hip
    x, s = _inputs(5, 7, seed=8, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        hip.color_fix_wavelet(x, s)
    with pytest.raises(NotImplementedError):
        hip.color_fix_adain(x, s)
    with pytest.raises(ValueError, match='levels'):
        hip.color_fix_wavelet(x, s, levels=6)


# ------------------------------------------------------------------------------------------------ the C entries
def test_c_entries_validate_their_arguments_without_a_gpu():
    """error paths return the invalid-argument code and a message before any launch"""
    from mrefsr_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p
    x, s, out, ws, ticket = p(0x1000), p(0x2000), p(0x3000), p(0x4000), p(0x5000)
    invalid = -1   # MREFSR_E_INVALID
    wavelet, adain = lib.mrefsr_color_fix_wavelet_f32, lib.mrefsr_color_fix_adain_f32
    for args in ((None, s, out), (x, None, out), (x, s, None)):
        assert wavelet(*args, 1, 3, 8, 8, None, 5, None) == invalid and b'null' in lib.mrefsr_last_error()
        assert adain(*args, 1, 3, 8, 8, None, ws, 1 << 20, ticket, None) == invalid and b'null' in lib.mrefsr_last_error()
    for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (-1, 3, 8, 8), (1, 3, 8, -8)):
        assert wavelet(x, s, out, *dims, None, 5, None) == invalid and b'positive' in lib.mrefsr_last_error()
        assert adain(x, s, out, *dims, None, ws, 1 << 20, ticket, None) == invalid and b'positive' in lib.mrefsr_last_error()
        assert lib.mrefsr_color_fix_adain_workspace_bytes(*dims) == -1
    for levels in (0, 6, -1, 63):
        assert wavelet(x, s, out, 1, 3, 8, 8, None, levels, None) == invalid and b'levels' in lib.mrefsr_last_error()
    need = lib.mrefsr_color_fix_adain_workspace_bytes(2, 3, 125, 40)
    assert need > 0 and need % 8 == 0
    assert adain(x, s, out, 2, 3, 125, 40, None, None, need, ticket, None) == invalid and b'null' in lib.mrefsr_last_error()
    assert adain(x, s, out, 2, 3, 125, 40, None, ws, need, None, None) == invalid and b'null' in lib.mrefsr_last_error()
    assert adain(x, s, out, 2, 3, 125, 40, None, ws, need - 8, ticket, None) == invalid and b'workspace' in lib.mrefsr_last_error()
    assert adain(x, s, out, 1, 3, 1, 1, None, ws, 1 << 20, ticket, None) == invalid and b'one pixel' in lib.mrefsr_last_error()
    assert wavelet(x, s, x, 1, 3, 8, 8, None, 5, None) == invalid   # out aliasing an input
