"""GPU: the kernels of val.color_fix (csrc/color_fix.hip) against the float64 torch statements of mrefsr_amd/color_fix.py.

Shapes: B = 2, C = 3; (1, 1) for the wavelet alone (a rectangle of one pixel has no unbiased variance), (2, 1), (5, 7), (31, 33),
(64, 95), (125, 40) and (130, 67): below, astride and beyond one halo of 31 pixels, beyond one 64 x 64 tile on each axis, rows of
W % 4 != 0 that take the 4-byte form ((125, 40) takes the 16-byte one), and a view one word off a 16-byte boundary.  sizes: None, a
cropped (H - 3, W - 5) and, for the wavelet, the mixed table [(H, W), (1, 1)].  x in [-0.1, 1.1], s in [0, 1], seeded.

Bounds, both derived and not measured.
  wavelet:  |out - ref| <= R 2^-24 max |s - x| + 2^-24 |ref|,  R = 4 L + 1: the fp32 roundings on the longest path of the kernel in
            front of its last add (the subtraction s - x, then per stage and axis the add of the two neighbours and the add of the
            centre term; the products by 0.25 and 0.5 are exact), each of a value no larger than max |s - x| because every stage is
            a convex combination with weights that are exact in fp32; the second term is the rounding of the last add.  The header
            of color_fix.hip states the same R.
  adain:    |out - ref| <= 2^-23 |ref| + 2^-36 (a |x - mu_x| + |mu_s|),  a = sigma_s / sigma_x: one rounding to fp32 (with a factor 2
            of slack), and double accumulation over at most 10^4 pixels."""
import pytest
import torch

from mrefsr_amd.color_fix import adain_color_fix_torch, wavelet_color_fix_torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
B, C = 2, 3
SIZES = [(1, 1), (2, 1), (5, 7), (31, 33), (64, 95), (125, 40), (130, 67)]
LEVELS = 5


def R(levels):
    """fp32 roundings in front of the kernel's last add: s - x, then two per pass, two passes per stage"""
    return 4 * levels + 1


def _inputs(h, w, seed, offset=0):
    """(x, s) on the GPU, fp32, contiguous; offset: words off a 16-byte boundary"""
    g = torch.Generator().manual_seed(seed)
    n = B * C * h * w
    x = (torch.rand(n, generator=g, dtype=torch.float64) * 1.2 - 0.1).float()
    s = torch.rand(n, generator=g, dtype=torch.float64).float()

    def place(t):
        buf = torch.empty(n + 8, device=DEV, dtype=torch.float32)
        assert buf.data_ptr() % 16 == 0
        v = buf[offset:offset + n].view(B, C, h, w)
        v.copy_(t.view(B, C, h, w))
        assert v.is_contiguous() and v.data_ptr() % 16 == 4 * offset
        return v
    return place(x), place(s)


def _size_cases(h, w, wavelet):
    cases = {'whole': None}
    if h > 3 and w > 5:
        cases['cropped'] = [(h - 3, w - 5)] * B
    if wavelet and (h, w) != (1, 1):
        cases['mixed'] = [(h, w), (1, 1)]
    return cases


def _bits(t):
    return t.contiguous().view(torch.int32)


def _outside(h, w, sizes):
    """[B,1,H,W] bool: the pixels outside the valid rectangles"""
    m = torch.ones(B, 1, h, w, dtype=torch.bool, device=DEV)
    for b, (hb, wb) in enumerate(sizes):
        m[b, :, :hb, :wb] = False
    return m.expand(B, C, h, w)


_refs = {}


def _case(kind, h, w, offset=0):
    """inputs and the float64 references of every sizes case, computed once and left unchanged"""
    key = (kind, h, w, offset)
    if key not in _refs:
        x, s = _inputs(h, w, seed=1000 * h + 10 * w + (1 if kind == 'adain' else 0), offset=offset)
        fn = (lambda a, b, sz: wavelet_color_fix_torch(a, b, sz, levels=LEVELS)) if kind == 'wavelet' else adain_color_fix_torch
        refs = {name: fn(x.double(), s.double(), sz) for name, sz in _size_cases(h, w, kind == 'wavelet').items()}
        _refs[key] = (x, s, refs)
    return _refs[key]


def _check_wavelet(out, ref, x, s, sizes, levels=LEVELS):
    assert out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous()
    bound = R(levels) * 2.0 ** -24 * float((s.double() - x.double()).abs().max()) + 2.0 ** -24 * ref.abs()
    err = (out.double() - ref).abs()
    print(f'wavelet {tuple(x.shape)} sizes={sizes}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all()), float((err / bound).max())
    if sizes is not None:
        m = _outside(*x.shape[2:], sizes)
        assert torch.equal(_bits(out)[m], _bits(x)[m])


def _check_adain(out, ref, x, s, sizes):
    assert out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous()
    h, w = x.shape[2:]
    rects = sizes if sizes is not None else [(h, w)] * B
    bound = torch.zeros_like(ref)
    for b, (hb, wb) in enumerate(rects):
        xd, sd = x[b, :, :hb, :wb].double(), s[b, :, :hb, :wb].double()
        mu_x, mu_s = xd.mean((1, 2), keepdim=True), sd.mean((1, 2), keepdim=True)
        a = ((sd.var((1, 2), unbiased=True, keepdim=True) + 1e-5) / (xd.var((1, 2), unbiased=True, keepdim=True) + 1e-5)).sqrt()
        bound[b, :, :hb, :wb] = 2.0 ** -23 * ref[b, :, :hb, :wb].abs() + 2.0 ** -36 * (a * (xd - mu_x).abs() + mu_s.abs())
    err = (out.double() - ref).abs()
    inside = ~_outside(h, w, rects)
    print(f'adain {tuple(x.shape)} sizes={sizes}: max err {float(err.max()):.3e}, max err / bound '
          f'{float((err[inside] / bound[inside]).max()):.3f}')
    assert bool((err[inside] <= bound[inside]).all()), float((err[inside] / bound[inside]).max())
    m = ~inside
    assert torch.equal(_bits(out)[m], _bits(x)[m])


@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_wavelet_against_float64(size):
    from mrefsr_amd import hip
    h, w = size
    x, s, refs = _case('wavelet', h, w)
    x0, s0 = x.clone(), s.clone()
    for name, sizes in _size_cases(h, w, True).items():
        out = hip.color_fix_wavelet(x, s, sizes)            # (levels: the default, 5)
        _check_wavelet(out, refs[name], x, s, sizes)
        assert torch.equal(_bits(hip.color_fix_wavelet(x, s, sizes, levels=LEVELS)), _bits(out)), 'two calls differ'
    assert torch.equal(_bits(x), _bits(x0)) and torch.equal(_bits(s), _bits(s0)), 'an input was written'


@pytest.mark.parametrize('size', SIZES[1:], ids=lambda s: f'{s[0]}x{s[1]}')
def test_adain_against_float64(size):
    from mrefsr_amd import hip
    h, w = size
    x, s, refs = _case('adain', h, w)
    x0, s0 = x.clone(), s.clone()
    for name, sizes in _size_cases(h, w, False).items():
        out = hip.color_fix_adain(x, s, sizes)
        _check_adain(out, refs[name], x, s, sizes)
        assert torch.equal(_bits(hip.color_fix_adain(x, s, sizes)), _bits(out)), 'two calls differ'
    assert torch.equal(_bits(x), _bits(x0)) and torch.equal(_bits(s), _bits(s0)), 'an input was written'


@pytest.mark.parametrize('size', [(64, 96), (125, 40)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_a_view_one_word_off_a_16_byte_boundary_takes_the_4_byte_form_with_the_same_bits(size):
    """W % 4 == 0: the aligned tensors take the 16-byte form, the same values one word off the boundary the 4-byte one"""
    from mrefsr_amd import hip
    h, w = size
    xa, sa = _inputs(h, w, seed=77)
    xo, so = _inputs(h, w, seed=77, offset=1)
    assert torch.equal(xa, xo) and xa.data_ptr() % 16 == 0 and xo.data_ptr() % 16 == 4
    for sizes in (None, [(h - 3, w - 5), (h, w - 1)]):
        ref = wavelet_color_fix_torch(xa.double(), sa.double(), sizes)
        out = hip.color_fix_wavelet(xo, so, sizes)
        _check_wavelet(out, ref, xo, so, sizes)
        assert torch.equal(_bits(out), _bits(hip.color_fix_wavelet(xa, sa, sizes)))
        ref = adain_color_fix_torch(xa.double(), sa.double(), sizes)
        out = hip.color_fix_adain(xo, so, sizes)
        _check_adain(out, ref, xo, so, sizes)
        assert torch.equal(_bits(out), _bits(hip.color_fix_adain(xa, sa, sizes)))


@pytest.mark.parametrize('levels', [1, 2, 3, 4])
def test_wavelet_levels_below_the_default(levels):
    from mrefsr_amd import hip
    for h, w in ((31, 33), (64, 96)):
        x, s = _inputs(h, w, seed=levels)
        sizes = [(h, w), (h - 3, w - 5)]
        ref = wavelet_color_fix_torch(x.double(), s.double(), sizes, levels=levels)
        _check_wavelet(hip.color_fix_wavelet(x, s, sizes, levels=levels), ref, x, s, sizes, levels=levels)


@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_wavelet_with_the_source_bit_equal_to_x_returns_the_bits_of_x(size):
    from mrefsr_amd import hip
    h, w = size
    x, _ = _inputs(h, w, seed=5)
    x.view(-1)[0] = -0.0
    for sizes in (None, [(h, w), (1, 1)]):
        out = hip.color_fix_wavelet(x, x.clone(), sizes)
        assert torch.equal(_bits(out), _bits(x))


def test_the_fix_moves_the_low_frequencies_to_the_source():
    """what the operators are for: a constant colour cast on x is gone afterwards"""
    from mrefsr_amd import hip
    h, w = 64, 95
    _, s = _inputs(h, w, seed=9)
    cast = torch.tensor([0.2, -0.1, 0.05], device=DEV).view(1, C, 1, 1)
    x = (s + cast).contiguous()
    out = hip.color_fix_wavelet(x, s)
    assert float((out - s).abs().max()) <= 1e-5 and float((x - s).abs().max()) >= 0.19   # low_L of a constant is the constant
    out = hip.color_fix_adain(x, s)
    assert float((out - s).abs().max()) <= 1e-5


def test_refusals_come_before_any_launch(monkeypatch):
    from mrefsr_amd import _lib, hip
    x, s = _inputs(5, 7, seed=11)

    def refuse(name, *a):
        raise AssertionError(f'{name} was called')

    monkeypatch.setattr(_lib, 'call', refuse)
    for fn in (hip.color_fix_wavelet, hip.color_fix_adain):
        with pytest.raises(NotImplementedError):
            fn(x.cpu(), s.cpu())
        with pytest.raises(NotImplementedError):
            fn(x, s.cpu())
        with pytest.raises(ValueError):
            fn(x, s[:, :, :4].contiguous())                    # mismatched shapes
        with pytest.raises(ValueError):
            fn(x[0], s[0])                                     # not [B,C,H,W]
        with pytest.raises(ValueError):
            fn(x.transpose(2, 3), s.transpose(2, 3))           # not contiguous
        with pytest.raises(TypeError):
            fn(x.bfloat16(), s.bfloat16())                     # fp32 only
        for bad in ([(5, 7)], [(5, 7), (0, 7)], [(5, 7), (6, 7)], [(5, 7), (5, 8)]):
            with pytest.raises(ValueError, match='sizes'):
                fn(x, s, bad)
    with pytest.raises(ValueError, match='levels'):
        hip.color_fix_wavelet(x, s, levels=0)
    with pytest.raises(ValueError, match='levels'):
        hip.color_fix_wavelet(x, s, levels=True)
    with pytest.raises(ValueError, match='1 pixel'):
        hip.color_fix_adain(x, s, [(5, 7), (1, 1)])
    x1, s1 = _inputs(1, 1, seed=12)
    with pytest.raises(ValueError, match='1 pixel'):
        hip.color_fix_adain(x1, s1)


def test_dispatcher_sends_gpu_fp32_to_the_kernels_and_the_rest_to_torch():
    from mrefsr_amd import hip
    from mrefsr_amd.color_fix import color_fix
    x, s = _inputs(31, 33, seed=13)
    sizes = [(31, 33), (20, 30)]
    assert torch.equal(_bits(color_fix(x, s, dict(type='wavelet', levels=3), sizes)), _bits(hip.color_fix_wavelet(x, s, sizes, levels=3)))
    assert torch.equal(_bits(color_fix(x, s, dict(type='adain'), sizes)), _bits(hip.color_fix_adain(x, s, sizes)))
    out = color_fix(x.double(), s.double(), dict(type='adain'), sizes)
    assert out.dtype == torch.float64 and torch.equal(out, adain_color_fix_torch(x.double(), s.double(), sizes))
