"""GPU: the two kernels of csrc/warp.hip through their torch bindings.

hip.warp_perspective: the bit-exact cases that follow from weights of exactly [0, 1, 0, 0] at a fraction of 0, and the accuracy against
the float64 oracle -- torch.nn.functional.grid_sample on the CPU in double (padding_mode='zeros', align_corners=True, grid 2 s /
(size - 1) - 1), which states the same cubic convolution (A = -0.75) and the same constant border.  The bounds are the ones DESIGN
3.24 counts from the kernel's evaluation order, |y - exact| <= c * 2^-24 * max |x|:  bicubic c = 70 (2.1 + 17.3 per axis for the
rounded fraction and the weights, times the other axis' sum of |w| <= 1.375, plus 15.2 for the two sums), bilinear c = 7 (1 + 0.5
per axis, the sum of |w| is 1, plus 4 for the two sums of length 2).  Measured on an MI355X at the
shape below: 3.32 of those 70 units (bicubic, clamped or not) and 1.89 (bilinear); 3.3 % (bicubic) and 9.6 % (bilinear) of the oracle's
outputs there are border zeros, and the cubic's values span [-0.141, 1.128].

hip.match_stats: against a numpy float64 restatement; counts and threshold hits exactly, the error sums to 1e-12 relative."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mrefsr_amd import views

pytestmark = pytest.mark.gpu

BOUND_C = {'bicubic': 70.0, 'bilinear': 7.0}   # DESIGN 3.24, each counted from its own chain of operations
INTERPS = ('bicubic', 'bilinear')


def _dev(t):
    return t.cuda().contiguous()


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _coords(s, ho, wo):
    """the source coordinates (sx, sy, t) [N,Ho,Wo] of every destination pixel, in double"""
    ys, xs = torch.meshgrid(torch.arange(ho, dtype=torch.float64), torch.arange(wo, dtype=torch.float64), indexing='ij')
    p = torch.stack([xs, ys, torch.ones_like(xs)], dim=-1)   # [Ho,Wo,3]
    q = torch.einsum('nij,hwj->nhwi', s, p)
    return q[..., 0] / q[..., 2], q[..., 1] / q[..., 2], q[..., 2]


def _oracle(x, s, ho, wo, interp, clamp):
    n, _, h, w = x.shape
    sx, sy, t = _coords(s, ho, wo)
    grid = torch.stack([2 * sx / (w - 1) - 1, 2 * sy / (h - 1) - 1], dim=-1)
    out = F.grid_sample(x.double(), grid, mode=interp, padding_mode='zeros', align_corners=True)
    out = torch.where((t > 0)[:, None], out, torch.zeros((), dtype=torch.float64))
    return out.clamp(0, 1) if clamp else out


@pytest.mark.parametrize('interp', INTERPS)
def test_the_identity_returns_the_inputs_bits(interp):
    from mrefsr_amd import hip
    x = _dev(_rand((2, 3, 7, 9), 0) * 4 - 2)   # (outside [0, 1] too: nothing is clamped unless asked)
    for s in (torch.eye(3, dtype=torch.float64), torch.eye(3, dtype=torch.float64).repeat(2, 1, 1), torch.eye(3).reshape(1, 9).repeat(2, 1)):
        out = hip.warp_perspective(x, s, interp=interp)
        assert out.shape == x.shape and out.dtype == torch.float32 and torch.equal(_bits(out), _bits(x))
    out = hip.warp_perspective(x, 3 * torch.eye(3, dtype=torch.float64), interp=interp)   # a homography has no scale
    assert torch.equal(_bits(out), _bits(x))
    assert torch.equal(hip.warp_perspective(x, torch.eye(3), interp=interp, clamp=True), x.clamp(0, 1))


@pytest.mark.parametrize('interp', INTERPS)
def test_an_integer_translation_returns_shifted_bits_and_exact_zeros(interp):
    from mrefsr_amd import hip
    n, c, h, w, ho, wo = 2, 3, 7, 9, 10, 40   # (Wo > 32: two tiles across; Ho > 8: two tiles down)
    x = _rand((n, c, h, w), 1) + 0.5
    shifts = [(3, -2), (-4, 5)]   # out(xo, yo) = x(xo + dx, yo + dy)
    s = torch.stack([torch.tensor([[1.0, 0, dx], [0, 1.0, dy], [0, 0, 1.0]], dtype=torch.float64) for dx, dy in shifts])
    want = torch.zeros(n, c, ho, wo)
    for i, (dx, dy) in enumerate(shifts):
        for yo in range(ho):
            for xo in range(wo):
                if 0 <= yo + dy < h and 0 <= xo + dx < w:
                    want[i, :, yo, xo] = x[i, :, yo + dy, xo + dx]
    out = hip.warp_perspective(_dev(x), s, out_size=(ho, wo), interp=interp).cpu()
    assert out.shape == (n, c, ho, wo)
    assert torch.equal(_bits(out), _bits(want))   # (+0 where the source is outside: the same bits as the zeros above)
    assert 0 < int((want == 0).sum()) < want.numel()


@pytest.mark.parametrize('interp', INTERPS)
def test_a_zero_image_stays_zero_under_a_random_homography(interp):
    from mrefsr_amd import hip
    s = views.sample_corner_homographies(3, 13, 17, [1, 3], generator=torch.Generator().manual_seed(5))
    out = hip.warp_perspective(torch.zeros(3, 3, 13, 17, device='cuda'), s, out_size=(11, 19), interp=interp)
    assert torch.equal(_bits(out), torch.zeros_like(_bits(out)))


@pytest.mark.parametrize('interp', INTERPS)
def test_where_the_third_coordinate_is_not_positive_the_output_is_zero(interp):
    from mrefsr_amd import hip
    x = _dev(_rand((1, 3, 7, 9), 2) + 1.0)
    s = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [-0.25, 0, 1.0]], dtype=torch.float64)   # t = 1 - xo / 4: 0 at xo = 4, negative behind
    out = hip.warp_perspective(x, s, interp=interp).cpu()
    assert torch.equal(_bits(out[..., 4:]), torch.zeros_like(_bits(out[..., 4:])))
    assert torch.equal(_bits(out[..., 0]), _bits(x.cpu()[..., 0])) and bool((out[..., :2] != 0).any())
    # not finite: a matrix of NaN, and one whose coordinates overflow
    for bad in (torch.full((3, 3), float('nan'), dtype=torch.float64),
                torch.tensor([[1e308, 1e308, 1e308], [0, 1.0, 0], [0, 0, 1e-308]], dtype=torch.float64)):
        out = hip.warp_perspective(x, bad, interp=interp)
        assert torch.equal(_bits(out), torch.zeros_like(_bits(out)))


@pytest.fixture(scope='module')
def accuracy_case():
    """N = 3, C = 3, 13 x 17 -> 11 x 19, values in [0, 1], random corner homographies; the float64 oracle, computed once"""
    x = _rand((3, 3, 13, 17), 3)
    s = views.sample_corner_homographies(3, 13, 17, [1, 3], generator=torch.Generator().manual_seed(4))
    want = {(interp, clamp): _oracle(x, s, 11, 19, interp, clamp) for interp in INTERPS for clamp in (False, True)}
    for v in want.values():
        v.requires_grad_(False)
    return x, s, want


@pytest.mark.parametrize('clamp', [False, True])
@pytest.mark.parametrize('interp', INTERPS)
def test_random_homographies_agree_with_the_float64_oracle_within_the_derived_bound(accuracy_case, interp, clamp):
    from mrefsr_amd import hip
    x, s, want = accuracy_case
    ref = want[(interp, clamp)]
    plain = want[(interp, False)]
    border = float((plain == 0).double().mean())
    assert 0.005 < border < 0.5, border   # some outputs lie where no tap is inside the image, most do not
    if interp == 'bicubic':
        assert float(plain.min()) < 0 and float(plain.max()) > 1   # the cubic overshoots: clamp has something to do
    out = hip.warp_perspective(_dev(x), s, out_size=(11, 19), interp=interp, clamp=clamp).cpu()
    err = float((out.double() - ref).abs().max())
    c = BOUND_C[interp]
    bound = c * 2.0 ** -24 * float(x.abs().max())
    print(f'warp {interp} clamp={clamp}: max |y - oracle| = {err:.3e} = {err / bound * c:.2f} of c = {c:g} units; '
          f'border zeros {border:.3f}; range [{float(plain.min()):.3f}, {float(plain.max()):.3f}]')
    assert err <= bound
    assert torch.equal(_bits(out)[plain == 0], torch.zeros_like(_bits(out)[plain == 0]))   # the border zeros are exact
    if clamp:
        assert float(out.min()) >= 0 and float(out.max()) <= 1
    assert torch.equal(hip.warp_perspective(_dev(x), s, out_size=(11, 19), interp=interp, clamp=clamp).cpu(), out)   # the same bits again


def _stats_numpy(idx, m, thr, h, w, y_hi, x_hi, margin):
    n, pw = idx.shape[0], w - 2
    out = np.zeros((n, 2 + len(thr)), np.float64)
    errs = [[] for _ in range(n)]
    for i in range(n):
        for qy in range(h - 2):
            for qx in range(pw):
                cx, cy = np.float64(qx + 1), np.float64(qy + 1)
                u = (m[i, 0] * cx + m[i, 1] * cy) + m[i, 2]
                v = (m[i, 3] * cx + m[i, 4] * cy) + m[i, 5]
                z = (m[i, 6] * cx + m[i, 7] * cy) + m[i, 8]
                if not z > 0:
                    continue
                tx, ty = u / z - 1.0, v / z - 1.0
                if not (margin <= qx <= x_hi - margin and margin <= qy <= y_hi - margin and margin <= tx <= x_hi - margin
                        and margin <= ty <= y_hi - margin):
                    continue
                ex, ey = np.float64(idx[i, qy, qx] % pw) - tx, np.float64(idx[i, qy, qx] // pw) - ty
                e = np.sqrt(ex * ex + ey * ey)
                out[i, 0] += 1
                errs[i].append(e)
                for k, t in enumerate(thr):
                    out[i, 2 + k] += e <= t
        out[i, 1] = np.sum(np.array(errs[i], np.float64)) if errs[i] else 0.0
    return out


@pytest.mark.parametrize('margin, valid_hw', [(0, None), (1, None), (1, (8, 9))])
def test_match_stats_equals_its_float64_restatement(margin, valid_hw):
    from mrefsr_amd import hip
    n, h, w = 3, 9, 11
    ph, pw = h - 2, w - 2
    # feature-space homographies near the identity: two from HR corner views, one whose third coordinate turns negative on a part
    s = views.sample_corner_homographies(2, 4 * h, 4 * w, [1, 5], generator=torch.Generator().manual_seed(6))
    m = torch.cat([views.to_feature_coords(s), torch.tensor([[[1.0, 0, 0.5], [0, 1.0, -0.25], [-0.125, 0, 1.0]]], dtype=torch.float64)])
    rng = np.random.default_rng(7)
    mn = m.reshape(n, 9).numpy()
    idx = np.zeros((n, ph, pw), np.int64)
    for i in range(n):
        for qy in range(ph):
            for qx in range(pw):
                z = mn[i, 6] * (qx + 1) + mn[i, 7] * (qy + 1) + mn[i, 8]
                tx = (mn[i, 0] * (qx + 1) + mn[i, 1] * (qy + 1) + mn[i, 2]) / z - 1 if z > 0 else 0.0
                ty = (mn[i, 3] * (qx + 1) + mn[i, 4] * (qy + 1) + mn[i, 5]) / z - 1 if z > 0 else 0.0
                mx = int(np.clip(np.rint(tx) + rng.integers(-2, 3) * (rng.random() < 0.5), 0, pw - 1))
                my = int(np.clip(np.rint(ty) + rng.integers(-2, 3) * (rng.random() < 0.5), 0, ph - 1))
                idx[i, qy, qx] = my * pw + mx
    thr = (0.5, 1.0, 2.0)
    vh, vw = (h, w) if valid_hw is None else valid_hw
    want = _stats_numpy(idx, mn, thr, h, w, vh - 3, vw - 3, margin)
    got = hip.match_stats(torch.from_numpy(idx).cuda(), m, thr, margin, valid_hw)
    assert got.shape == (n, 5) and got.dtype == torch.float64 and got.is_cuda
    got = got.cpu().numpy()
    print('match_stats', margin, valid_hw, got.tolist())
    assert (want[:, 0] > 0).all() and (want[:, 2] < want[:, 0]).any() and want[2, 0] < want[0, 0]
    assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 2:], want[:, 2:])
    assert np.all(np.abs(got[:, 1] - want[:, 1]) <= 1e-12 * np.abs(want[:, 1]))
    # one matrix for all pairs, no thresholds
    one = hip.match_stats(torch.from_numpy(idx).cuda(), m[0], (), margin, valid_hw).cpu().numpy()
    assert one.shape == (n, 2) and np.array_equal(one[0], got[0, :2])


def test_the_bindings_refuse_what_the_kernels_do_not_take():
    from mrefsr_amd import hip
    x = torch.zeros(2, 3, 5, 6, device='cuda')
    eye = torch.eye(3, dtype=torch.float64)
    with pytest.raises(ValueError, match='interp'):
        hip.warp_perspective(x, eye, interp='nearest')
    with pytest.raises(ValueError, match='clamp'):
        hip.warp_perspective(x, eye, clamp=1)
    with pytest.raises(ValueError, match='out_size'):
        hip.warp_perspective(x, eye, out_size=(0, 4))
    with pytest.raises(ValueError, match='3 x 3'):
        hip.warp_perspective(x, eye.repeat(3, 1, 1))
    with pytest.raises(TypeError):
        hip.warp_perspective(x.double(), eye)
    with pytest.raises(ValueError, match='contiguous'):
        hip.warp_perspective(x.transpose(2, 3), eye)
    idx = torch.zeros(2, 7, 9, dtype=torch.int64, device='cuda')
    with pytest.raises(ValueError, match='thresholds'):
        hip.match_stats(idx, eye, (1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match='margin'):
        hip.match_stats(idx, eye, (1,), margin=-1)
    with pytest.raises(ValueError, match='valid_hw'):
        hip.match_stats(idx, eye, (1,), valid_hw=(10, 11))
    with pytest.raises(TypeError):
        hip.match_stats(idx.int(), eye)
