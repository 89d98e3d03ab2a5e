"""GPU: the two kernels of the x8 geometric self-ensemble (csrc/selfens.hip) against their torch statements, bit for bit.

Sizes below, astride and on the edges of the 32-word tile; (32, 64) and (40, 72) take the 16-byte form in both groups, (5, 7),
(31, 33) and (1, 1) the 4-byte one, and a view one word off a 16-byte boundary takes the 4-byte form at an aligned size."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SIZES = [(1, 1), (5, 7), (31, 33), (32, 64), (40, 72)]
C = 3


def _copy(src, j, tr):
    """the torch statement of copy j"""
    s = src
    if j & 1:
        s = s.flip(-1)
    if j & 2:
        s = s.flip(-2)
    if tr:
        s = s.transpose(-1, -2)
    return s


def _inverse(out, j, tr):
    o = out
    if tr:
        o = o.transpose(-1, -2)
    if j & 2:
        o = o.flip(-2)
    if j & 1:
        o = o.flip(-1)
    return o


def _expand(src, tr, outer):
    """[outer * inner, C, H, W] -> [outer][4][inner] copies, in torch"""
    inner = src.shape[0] // outer
    s = src.view(outer, inner, *src.shape[1:])
    return torch.stack([_copy(s, j, tr) for j in range(4)], dim=1).reshape(outer * 4 * inner, *_copy(s, 0, tr).shape[2:]).contiguous()


def _chain(a, b):
    """a [4, N, C, H, W], b [4, N, C, W, H]: the inverse transforms, seven adds in the stated order, one multiply"""
    acc = _inverse(a[0], 0, 0)
    for j in (1, 2, 3):
        acc = acc + _inverse(a[j], j, 0)
    for j in range(4):
        acc = acc + _inverse(b[j], j, 1)
    return acc * 0.125


def _bits(t):
    return t.contiguous().view(torch.int32)


def _random(shape, seed, specials=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-20, 20, shape, generator=g).float())
    if specials:
        flat = x.view(-1)
        vals = torch.tensor([float('nan'), float('inf'), float('-inf'), -0.0, 0.0], dtype=torch.float32)
        pos = torch.randperm(flat.numel(), generator=g)[:min(10, flat.numel())]
        flat[pos] = vals[torch.arange(pos.numel()) % 5]
        if flat.numel() > 10:   # a NaN with a payload and its sign bit set
            flat.view(torch.int32)[torch.randperm(flat.numel(), generator=g)[0]] = -0x00345679
    return x.to(DEV)


def _misaligned(t):
    """the same values in storage one word behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize('tr', [0, 1])
@pytest.mark.parametrize('outer,inner', [(1, 1), (2, 3), (5, 2)])
@pytest.mark.parametrize('hw', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_expand_is_the_torch_statement_bit_for_bit(hw, outer, inner, tr):
    from mrefsr_amd import hip
    h, w = hw
    src = _random((outer * inner, C, h, w), seed=h * 1000 + w * 10 + outer, specials=True)
    want = _expand(src, tr, outer)
    got = hip.dihedral_expand(src, tr, outer=outer)
    assert got.shape == want.shape == (outer * 4 * inner, C, *((w, h) if tr else (h, w))) and got.is_contiguous()
    assert torch.equal(_bits(got), _bits(want))
    # the [outer][4][inner] order, spelt out for one row: copy 3 of the last source row
    o, i = outer - 1, inner - 1
    assert torch.equal(_bits(got[(o * 4 + 3) * inner + i]), _bits(_copy(src[o * inner + i], 3, tr)))
    # a source off the 16-byte grid: the 4-byte form, the same bits
    assert torch.equal(_bits(hip.dihedral_expand(_misaligned(src), tr, outer=outer)), _bits(want))


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('hw', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_merge_is_the_torch_chain_bit_for_bit(hw, n):
    from mrefsr_amd import hip
    h, w = hw
    a = _random((4 * n, C, h, w), seed=h * 77 + w + n)
    b = _random((4 * n, C, w, h), seed=h * 79 + w + n)
    want = _chain(a.view(4, n, C, h, w), b.view(4, n, C, w, h))
    got = hip.dihedral_merge(a, b)
    assert got.shape == (n, C, h, w) and got.is_contiguous()
    assert torch.isfinite(want).all()
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(hip.dihedral_merge(_misaligned(a), b)), _bits(want))
    assert torch.equal(_bits(hip.dihedral_merge(a, _misaligned(b))), _bits(want))


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('hw', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_merging_the_expansion_returns_the_image(hw, n):
    """eight copies of one image through identity "networks" (|x| < 1e30: no overflow).  The round trip returns x bit for bit
    where the seven adds of the stated order are exact: the partial sums 3 x, 5 x, 6 x and 7 x need up to three more mantissa
    bits than x, so the images here have their last three mantissa bits clear.  For a full 24-bit mantissa those sums round -- in
    torch's chain too: ((((((x + x) + x) + x) + x) + x) + x) + x) * 0.125 != x for about 43 % of random fp32 values -- and the
    round trip is that chain of x, which the second half asserts, bit for bit again."""
    from mrefsr_amd import hip
    h, w = hw
    full = _random((n, C, h, w), seed=h + 31 * w + n)
    x = (full.view(torch.int32) & ~7).view(torch.float32)
    assert float(x.abs().max()) < 1e30 and torch.isfinite(x).all()
    got = hip.dihedral_merge(hip.dihedral_expand(x, 0), hip.dihedral_expand(x, 1))
    assert torch.equal(_bits(got), _bits(x))
    chain = full
    for _ in range(7):
        chain = chain + full
    got = hip.dihedral_merge(hip.dihedral_expand(full, 0), hip.dihedral_expand(full, 1))
    assert torch.equal(_bits(got), _bits(chain * 0.125))


def test_wrappers_refuse_what_the_kernels_do_not_take():
    from mrefsr_amd import hip
    x = torch.zeros(6, 3, 5, 7, device=DEV)
    with pytest.raises(ValueError):
        hip.dihedral_expand(x, 2)
    with pytest.raises(ValueError):
        hip.dihedral_expand(x, 0, outer=4)                       # 6 rows are no multiple of 4
    with pytest.raises(ValueError):
        hip.dihedral_expand(x[:, :, :, ::2], 0)                  # not contiguous
    with pytest.raises(TypeError):
        hip.dihedral_expand(x.half(), 0)
    with pytest.raises(ValueError):
        hip.dihedral_merge(torch.zeros(4, 3, 5, 7, device=DEV), torch.zeros(4, 3, 5, 7, device=DEV))   # b is not [.., W, H]
    with pytest.raises(ValueError):
        hip.dihedral_merge(torch.zeros(6, 3, 5, 7, device=DEV), torch.zeros(6, 3, 7, 5, device=DEV))   # 6 rows are not 4 N
