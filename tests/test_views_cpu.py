"""No GPU: the host side of the homography views (mrefsr_amd/views.py) -- the matrices in float64, the three options' parsers, the
argument checks of the two C entry points of csrc/warp.hip and of their torch bindings."""
import ctypes

import pytest
import torch

from mrefsr_amd import views


def _apply(m, pts):
    p = torch.cat([pts, torch.ones_like(pts[..., :1])], dim=-1) @ m.transpose(-1, -2)
    return p[..., :2] / p[..., 2:]


def test_the_dlt_maps_its_four_points():
    g = torch.Generator().manual_seed(1)
    src = torch.tensor([[0.0, 0.0], [16.0, 0.0], [16.0, 12.0], [0.0, 12.0]], dtype=torch.float64).repeat(5, 1, 1)
    dst = src + 3 * (torch.rand(5, 4, 2, generator=g, dtype=torch.float64) - 0.5)
    h = views.homography_from_points(src, dst)
    assert h.shape == (5, 3, 3) and h.dtype == torch.float64 and bool((h[:, 2, 2] == 1).all())
    assert float((_apply(h, src) - dst).abs().max()) <= 1e-9
    # a single pair of point sets, given as lists
    one = views.homography_from_points(src[0].tolist(), dst[0].tolist())
    assert one.shape == (3, 3) and float((_apply(one, src[0]) - dst[0]).abs().max()) <= 1e-9
    with pytest.raises(ValueError, match='homography_from_points'):
        views.homography_from_points(src[:, :3], dst[:, :3])


def test_the_sampler_is_a_pure_function_of_the_seed():
    def draw(seed, **kw):
        return views.sample_corner_homographies(4, 40, 56, [2, 9], generator=torch.Generator().manual_seed(seed), **kw)

    a, b, c = draw(7), draw(7), draw(8)
    assert a.shape == (4, 3, 3) and a.dtype == torch.float64
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert not torch.equal(a[0], a[1])
    # the documented order of draws: one randint of magnitudes, one of signs, corners tl, tr, br, bl, x before y
    g = torch.Generator().manual_seed(7)
    mag, neg = torch.randint(2, 9, (4, 4, 2), generator=g), torch.randint(0, 2, (4, 4, 2), generator=g)
    cx, cy, r = 55 / 2, 39 / 2, 39 / 2
    square = torch.tensor([[cx - r, cy - r], [cx + r, cy - r], [cx + r, cy + r], [cx - r, cy + r]], dtype=torch.float64)
    quad = square + (mag * (1 - 2 * neg)).double()
    assert float((_apply(a, square.expand(4, 4, 2)) - quad).abs().max()) <= 1e-9   # S maps the square onto the quadrilateral
    # a smaller window
    sq16 = torch.tensor([[cx - 7.5, cy - 7.5], [cx + 7.5, cy - 7.5], [cx + 7.5, cy + 7.5], [cx - 7.5, cy + 7.5]], dtype=torch.float64)
    with pytest.raises(ValueError, match=r'window / 4'):   # (hi = 9 > 16 / 4)
        draw(7, window=16)
    g = torch.Generator().manual_seed(7)
    w16 = views.sample_corner_homographies(4, 40, 56, [1, 4], window=16, generator=g)
    g = torch.Generator().manual_seed(7)
    mag, neg = torch.randint(1, 4, (4, 4, 2), generator=g), torch.randint(0, 2, (4, 4, 2), generator=g)
    assert float((_apply(w16, sq16.expand(4, 4, 2)) - (sq16 + (mag * (1 - 2 * neg)).double())).abs().max()) <= 1e-9


def test_the_sampler_returns_identities_for_no_perturbation_and_refuses_a_concave_range():
    g = torch.Generator().manual_seed(3)
    before = g.get_state()
    eye = views.sample_corner_homographies(3, 20, 30, 0, generator=g)
    assert torch.equal(eye, torch.eye(3, dtype=torch.float64).repeat(3, 1, 1))
    assert torch.equal(g.get_state(), before)   # nothing was drawn
    views.sample_corner_homographies(1, 20, 30, [0, 5], generator=g)   # hi = window / 4: allowed
    with pytest.raises(ValueError, match=r'window / 4'):
        views.sample_corner_homographies(1, 20, 30, [0, 6], generator=g)
    with pytest.raises(ValueError, match=r'window / 4'):
        views.sample_corner_homographies(1, 64, 64, [2, 5], window=16, generator=g)
    for bad in ([5], [5, 5], [-1, 4], [1.0, 4], 'x', True, [3, 2]):
        with pytest.raises(ValueError, match='perturb'):
            views.sample_corner_homographies(1, 20, 30, bad, generator=g)
    with pytest.raises(ValueError, match='window'):
        views.sample_corner_homographies(1, 20, 30, [1, 3], window=21, generator=g)


def test_the_indexed_views_depend_on_seed_and_index_only():
    a = views.indexed_corner_homographies(0, 5, 2, 64, 80, (5, 16))
    assert a.shape == (2, 3, 3) and torch.equal(a, views.indexed_corner_homographies(0, 5, 2, 64, 80, (5, 16)))
    assert not torch.equal(a, views.indexed_corner_homographies(0, 6, 2, 64, 80, (5, 16)))
    assert not torch.equal(a, views.indexed_corner_homographies(1, 5, 2, 64, 80, (5, 16)))


def test_similarity_is_exact_at_multiples_of_90_degrees():
    h, w = 7, 10
    assert torch.equal(views.similarity(h, w, 1.0, 0), torch.eye(3, dtype=torch.float64))
    assert torch.equal(views.similarity(h, w, 1.0, 180), torch.tensor([[-1.0, 0, w - 1], [0, -1.0, h - 1], [0, 0, 1]], dtype=torch.float64))
    assert torch.equal(views.similarity(h, w, 1.0, 360), torch.eye(3, dtype=torch.float64))
    cx, cy = (w - 1) / 2, (h - 1) / 2
    assert torch.equal(views.similarity(h, w, 1.0, 90), torch.tensor([[0, -1.0, cx + cy], [1.0, 0, cy - cx], [0, 0, 1]], dtype=torch.float64))
    assert torch.equal(views.similarity(h, w, 1.0, -90), views.similarity(h, w, 1.0, 270))
    # the centre is the fixed point; a magnification by 2 samples at half the distance from it
    s = views.similarity(h, w, 2.0, 30)
    c = torch.tensor([[cx, cy]], dtype=torch.float64)
    assert float((_apply(s, c) - c).abs().max()) <= 1e-12
    p = torch.tensor([[cx + 4.0, cy]], dtype=torch.float64)
    assert abs(float((_apply(s, p) - c).norm()) - 2.0) <= 1e-12
    for bad in (0, -1.0, float('inf')):
        with pytest.raises(ValueError, match='similarity'):
            views.similarity(h, w, bad, 0)


def test_a_translation_by_multiples_of_four_is_the_opposite_translation_of_the_feature_maps():
    for a, b in ((1, -2), (3, 0), (-5, 7)):
        s = torch.tensor([[1.0, 0, 4 * a], [0, 1.0, 4 * b], [0, 0, 1.0]], dtype=torch.float64)
        assert torch.equal(views.to_feature_coords(s), torch.tensor([[1.0, 0, -a], [0, 1.0, -b], [0, 0, 1.0]], dtype=torch.float64))
    # a cell's centre goes where its HR pixel goes: A M c = S^-1 A c
    s = views.sample_corner_homographies(2, 64, 80, [3, 12], generator=torch.Generator().manual_seed(0))
    m = views.to_feature_coords(s)
    cells = torch.tensor([[2.0, 3.0], [10.0, 7.0]], dtype=torch.float64)
    hr = 4 * cells + 1.5
    for i in range(2):
        back = _apply(s[i], 4 * _apply(m[i], cells) + 1.5)
        assert float((back - hr).abs().max()) <= 1e-9
    with pytest.raises(ValueError, match='singular'):
        views.to_feature_coords(torch.zeros(3, 3, dtype=torch.float64))


def test_sample_ref_augment_draws_in_its_documented_order():
    cfg = views.parse_ref_augment(dict(ref_augment=dict(p=0.5, perturb=[2, 8])))
    s = views.sample_ref_augment(8, 40, 48, cfg, torch.Generator().manual_seed(11))
    g = torch.Generator().manual_seed(11)
    chosen = torch.rand(8, generator=g) < 0.5
    full = views.sample_corner_homographies(8, 40, 48, (2, 8), None, g)
    assert 0 < int(chosen.sum()) < 8
    assert torch.equal(s, torch.where(chosen[:, None, None], full, torch.eye(3, dtype=torch.float64)))
    assert views.sample_ref_augment(8, 40, 48, dict(cfg, p=0.0), torch.Generator().manual_seed(11)) is None


def test_a_parsed_perturb_of_zero_goes_through_the_samplers_as_identities():
    """what the parsers keep for ``perturb: 0`` is what the samplers are handed at the first batch"""
    eye = torch.eye(3, dtype=torch.float64)
    aug = views.parse_ref_augment(dict(ref_augment=dict(p=1, perturb=0)))
    assert aug['perturb'] == (0, 0)
    g = torch.Generator().manual_seed(5)
    assert views.sample_ref_augment(4, 40, 48, aug, g) is None   # every view is the image itself: nothing to launch
    g2 = torch.Generator().manual_seed(5)
    torch.rand(4, generator=g2)
    assert torch.equal(g.get_state(), g2.get_state())   # (the one torch.rand was drawn, nothing else)
    for parse, key in ((views.parse_match_probe, 'match_probe'), (views.parse_ref_perturb, 'ref_perturb')):
        cfg = parse({key: dict(perturb=0)})
        assert cfg['perturb'] == (0, 0)
        got = views.indexed_corner_homographies(cfg['seed'], 3, 2, 40, 48, cfg['perturb'], cfg['window'])
        assert torch.equal(got, eye.repeat(2, 1, 1))
    for zero in (0, (0, 0), [0, 0]):
        assert torch.equal(views.sample_corner_homographies(2, 40, 48, zero), eye.repeat(2, 1, 1))
    assert torch.equal(views.to_feature_coords(eye), eye)


GOOD_AUGMENT = [dict(), dict(p=0), dict(p=1, perturb=[0, 3], window=16, interp='bilinear'), dict(perturb=0)]
BAD_AUGMENT = [
    (True, r'train\.ref_augment'), ('on', r'train\.ref_augment'), (dict(q=1), r"train\.ref_augment: unknown key\(s\) \['q'\]"),
    (dict(p=1.5), r'train\.ref_augment\.p'), (dict(p=True), r'train\.ref_augment\.p'), (dict(p='0.5'), r'train\.ref_augment\.p'),
    (dict(perturb=[5]), r'train\.ref_augment\.perturb'), (dict(perturb=[20, 5]), r'train\.ref_augment\.perturb'),
    (dict(perturb=[0.5, 2]), r'train\.ref_augment\.perturb'), (dict(window=1), r'train\.ref_augment\.window'),
    (dict(window=2.5), r'train\.ref_augment\.window'), (dict(window=40, perturb=[5, 20]), r'train\.ref_augment\.perturb'),
    (dict(interp='nearest'), r'train\.ref_augment\.interp'), (dict(interp=1), r'train\.ref_augment\.interp')]
GOOD_PERTURB = [dict(scale=0.5), dict(rotate=-30), dict(scale=2, rotate=90, interp='bilinear'), dict(perturb=[5, 20]),
                dict(perturb=[1, 4], seed=3, window=32)]
BAD_PERTURB = [
    (True, r'val\.ref_perturb'), (dict(), r'val\.ref_perturb'), (dict(angle=3), r"val\.ref_perturb: unknown key\(s\) \['angle'\]"),
    (dict(scale=0), r'val\.ref_perturb\.scale'), (dict(scale='2'), r'val\.ref_perturb\.scale'), (dict(rotate=float('nan')), r'val\.ref_perturb\.rotate'),
    (dict(rotate=True), r'val\.ref_perturb\.rotate'), (dict(scale=1, perturb=[1, 2]), r'val\.ref_perturb: .*two forms'),
    (dict(rotate=0, seed=1), r'val\.ref_perturb: .*two forms'), (dict(seed=1), r'val\.ref_perturb'),
    (dict(perturb=[2, 2]), r'val\.ref_perturb\.perturb'), (dict(perturb=[1, 3], seed=-1), r'val\.ref_perturb\.seed'),
    (dict(perturb=[1, 3], seed=1.0), r'val\.ref_perturb\.seed'), (dict(perturb=[1, 9], window=16), r'val\.ref_perturb\.perturb'),
    (dict(scale=1, interp='cubic'), r'val\.ref_perturb\.interp')]
GOOD_PROBE = [True, dict(), dict(source='lq_up', margin=0, thresholds=[0.5, 1, 2, 4], seed=9), dict(perturb=0, window=8)]
BAD_PROBE = [
    ('gt', r'val\.match_probe'), (3, r'val\.match_probe'), (dict(threshold=[1]), r"val\.match_probe: unknown key\(s\) \['threshold'\]"),
    (dict(thresholds=[]), r'val\.match_probe\.thresholds'), (dict(thresholds=[1, 2, 3, 4, 5]), r'val\.match_probe\.thresholds'),
    (dict(thresholds=2), r'val\.match_probe\.thresholds'), (dict(thresholds=[0]), r'val\.match_probe\.thresholds'),
    (dict(thresholds=['1']), r'val\.match_probe\.thresholds'), (dict(margin=-1), r'val\.match_probe\.margin'),
    (dict(margin=1.5), r'val\.match_probe\.margin'), (dict(margin=True), r'val\.match_probe\.margin'),
    (dict(source='ref'), r'val\.match_probe\.source'), (dict(seed='0'), r'val\.match_probe\.seed'),
    (dict(perturb=[4, 1]), r'val\.match_probe\.perturb'), (dict(window=0), r'val\.match_probe\.window'),
    (dict(interp=None), r'val\.match_probe\.interp')]


def test_well_formed_options_parse_to_their_checked_form():
    assert views.parse_ref_augment(None) is None and views.parse_ref_augment(dict(ref_augment=None)) is None
    assert views.parse_ref_augment(dict(ref_augment=False)) is None
    assert views.parse_ref_augment(dict(ref_augment={})) == dict(p=0.5, perturb=(5, 20), window=None, interp='bicubic')
    for good in GOOD_AUGMENT:
        assert views.parse_ref_augment(dict(ref_augment=good)) is not None
    assert views.parse_ref_perturb({}) is None and views.parse_ref_perturb(dict(ref_perturb=False)) is None
    assert views.parse_ref_perturb(dict(ref_perturb=dict(rotate=180))) == dict(kind='similarity', scale=1.0, rotate=180.0, interp='bicubic')
    assert views.parse_ref_perturb(dict(ref_perturb=dict(perturb=[5, 20]))) == dict(kind='corners', perturb=(5, 20), window=None, seed=0,
                                                                                     interp='bicubic')
    for good in GOOD_PERTURB:
        assert views.parse_ref_perturb(dict(ref_perturb=good)) is not None
    assert views.parse_match_probe(dict(match_probe=None)) is None
    assert views.parse_match_probe(dict(match_probe=True)) == dict(perturb=(5, 20), window=None, thresholds=(1.0, 2.0), margin=3, source='gt',
                                                                   seed=0, interp='bicubic')
    for good in GOOD_PROBE:
        assert views.parse_match_probe(dict(match_probe=good)) is not None
    assert views.probe_result_keys((1.0, 2.0, 2.5)) == ['match_epe', 'match_pck1', 'match_pck2', 'match_pck2.5']
    assert views.probe_numbers([4.0, 2.0, 3.0, 4.0], (1.0, 2.0)) == dict(count=4, match_epe=0.5, match_pck1=0.75, match_pck2=1.0)


@pytest.mark.parametrize('which, key, cases', [('train', 'ref_augment', BAD_AUGMENT), ('val', 'ref_perturb', BAD_PERTURB),
                                               ('val', 'match_probe', BAD_PROBE)])
def test_every_malformed_option_is_refused_by_name_at_construction(which, key, cases):
    """by the parser and by both model classes, before a network is built or a device asked for"""
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel, RefRestorationModel
    parse = getattr(views, 'parse_' + key)
    for bad, pattern in cases:
        with pytest.raises(ValueError, match=pattern):
            parse({key: bad})
        for cls in (MultiRefRestorationModel, RefRestorationModel):
            for is_train in (True, False):   # (train.ref_augment is refused in a test-only configuration too)
                with pytest.raises(ValueError, match=pattern):
                    cls({'num_gpu': 1, 'is_train': is_train, which: {key: bad}})


def test_the_c_entries_validate_their_arguments_without_a_gpu():
    """error paths return the invalid-argument code and a message before any launch"""
    from mrefsr_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p
    x, s, y, st = p(0x1000), p(0x2000), p(0x3000), p(0x4000)
    invalid = -1   # MREFSR_E_INVALID
    warp, stats = lib.mrefsr_warp_persp_f32, lib.mrefsr_match_stats_f64
    for args in ((None, s, y), (x, None, y), (x, s, None), (x, s, x)):
        assert warp(*args, 1, 3, 8, 8, 8, 8, 1, 0, None) == invalid and b'null' in lib.mrefsr_last_error()
    for dims in ((0, 3, 8, 8, 8, 8), (1, 0, 8, 8, 8, 8), (1, 3, -1, 8, 8, 8), (1, 3, 8, 0, 8, 8), (1, 3, 8, 8, 0, 8), (1, 3, 8, 8, 8, -4)):
        assert warp(x, s, y, *dims, 1, 0, None) == invalid and b'positive' in lib.mrefsr_last_error()
    for interp in (-1, 2, 7):
        assert warp(x, s, y, 1, 3, 8, 8, 8, 8, interp, 0, None) == invalid and b'interp' in lib.mrefsr_last_error()
    assert warp(x, s, y, 1, 3, 8, 8, 8, 8, 1, 2, None) == invalid and b'clamp' in lib.mrefsr_last_error()
    assert warp(x, s, y, 1, 3, 1 << 16, 1 << 16, 8, 8, 1, 0, None) == invalid and b'2^30' in lib.mrefsr_last_error()
    assert warp(x, s, y, 65536, 3, 8, 8, 8, 8, 1, 0, None) == invalid and b'65535' in lib.mrefsr_last_error()
    assert warp(x, s, y, 1, 3, 8, 8, 524288, 1, 1, 0, None) == invalid and b'524280' in lib.mrefsr_last_error()
    thr = (ctypes.c_double * 2)(1.0, 2.0)
    for args in ((None, s, thr, st), (x, None, thr, st), (x, s, None, st), (x, s, thr, None)):
        assert stats(*args, 1, 9, 11, 6, 8, 0, 2, None) == invalid and b'null' in lib.mrefsr_last_error()
    for n, h, w in ((0, 9, 11), (1, 2, 11), (1, 9, 2), (-3, 9, 11)):
        assert stats(x, s, thr, st, n, h, w, 0, 0, 0, 2, None) == invalid and b'match_stats: N=' in lib.mrefsr_last_error()
    for t in (-1, 5):
        assert stats(x, s, thr, st, 1, 9, 11, 6, 8, 0, t, None) == invalid and b'thresholds' in lib.mrefsr_last_error()
    for y_hi, x_hi, margin in ((7, 8, 0), (6, 9, 0), (-1, 8, 0), (6, 8, -1)):
        assert stats(x, s, thr, st, 1, 9, 11, y_hi, x_hi, margin, 2, None) == invalid and b'margin' in lib.mrefsr_last_error()


def test_the_bindings_have_no_cpu_path_and_check_before_a_launch():
    from mrefsr_amd import hip
    with pytest.raises(NotImplementedError, match='no CPU path'):
        hip.warp_perspective(torch.zeros(1, 3, 4, 4), torch.eye(3, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match='no CPU path'):
        hip.match_stats(torch.zeros(1, 3, 3, dtype=torch.int64), torch.eye(3, dtype=torch.float64))
    for bad in (torch.eye(4), torch.zeros(3, 3, 3), torch.zeros(2, 8)):
        with pytest.raises(ValueError, match='3 x 3'):
            hip._homographies('warp_perspective', bad, 2, torch.device('cpu'))
    m = hip._homographies('warp_perspective', [[1, 0, 2], [0, 1, 3], [0, 0, 1]], 2, torch.device('cpu'))
    assert m.shape == (2, 9) and m.dtype == torch.float64 and m.is_contiguous() and m[1].tolist() == [1, 0, 2, 0, 1, 3, 0, 0, 1]
