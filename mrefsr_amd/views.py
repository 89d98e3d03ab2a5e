"""Homography views of reference images: the matrices (here, on the host, in float64, no GPU needed) and the three options of the
models that use them on the kernels of csrc/warp.hip (hip.warp_perspective, hip.match_stats).

The reference makes its views on the host: image_pair_generation_perspective of basicsr/data/ref_cufed_dataset.py:190-272 and
ref_megadepth_dataset.py:161-243 moves the four corners of a square window by random integers, fits the homography H square ->
quadrilateral through them and calls cv2.warpPerspective(img, inv(H), INTER_CUBIC) -- so the view samples the image at H p:
out(p) = img(H p).  Every matrix below is such a SAMPLING matrix S (destination -> source) in integer pixel coordinates, pixel
(x, y) at (x, y); the reference's call has S = H.  Bit parity with OpenCV is not claimed, and the uint8 round trip of the
reference's view is not reproduced (clamp: true saturates where it does).

    train.ref_augment   each (sample, reference) image of a training batch is replaced, with probability p, by a random view
    val.ref_perturb     the references of every validation / test batch are scaled and rotated, or viewed through a corner
                        homography that depends on (seed, image index) only: the robustness protocol of C2-Matching (Jiang et al.,
                        CVPR 2021, section 4.4: scale and rotation)
    val.match_probe     the extractor + matcher pair is scored against a known answer: a view of the input itself

No claim about image or matching quality is made anywhere: only random-init weights were available when this was written.
"""
import math

import torch

INTERPS = ('bicubic', 'bilinear')
REF_AUGMENT_KEYS = ('p', 'perturb', 'window', 'interp')
REF_PERTURB_KEYS = ('scale', 'rotate', 'perturb', 'window', 'seed', 'interp')
MATCH_PROBE_KEYS = ('perturb', 'window', 'thresholds', 'margin', 'source', 'seed', 'interp')
PROBE_SOURCES = ('gt', 'lq_up')
MAX_THRESHOLDS = 4
# a conv3_1 cell (i, j) of the extractor is centred on HR pixel (4 i + 1.5, 4 j + 1.5) behind the two 2 x 2 pools
FEATURE_STRIDE, FEATURE_OFFSET = 4.0, 1.5


# ------------------------------------------------------------------ matrices
def homography_from_points(src, dst):
    """the homography H with H (src_i, 1) ~ (dst_i, 1) for four point pairs: src, dst [..., 4, 2] -> [..., 3, 3] float64, H[2][2] = 1
    (the four-point direct linear transform: eight equations, solved in double; cv2.getPerspectiveTransform's system)"""
    src, dst = torch.as_tensor(src, dtype=torch.float64), torch.as_tensor(dst, dtype=torch.float64)
    if src.shape != dst.shape or src.shape[-2:] != (4, 2):
        raise ValueError(f'homography_from_points: two [..., 4, 2] point sets of one shape expected, got {tuple(src.shape)} and {tuple(dst.shape)}')
    x, y, u, v = src[..., 0], src[..., 1], dst[..., 0], dst[..., 1]
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    rows_u = torch.stack([x, y, one, zero, zero, zero, -u * x, -u * y], dim=-1)
    rows_v = torch.stack([zero, zero, zero, x, y, one, -v * x, -v * y], dim=-1)
    a = torch.cat([rows_u, rows_v], dim=-2)
    b = torch.cat([u, v], dim=-1).unsqueeze(-1)
    sol = torch.linalg.solve(a, b).squeeze(-1)
    return torch.cat([sol, torch.ones_like(sol[..., :1])], dim=-1).reshape(*src.shape[:-2], 3, 3)


def check_perturb(name, perturb):
    """perturb: 0 (no perturbation) or [lo, hi] with ints 0 <= lo < hi -> (lo, hi), (0, 0) for 0; the checked pair (0, 0) -- what the
    parsers keep for 0 -- is taken as it is"""
    if isinstance(perturb, int) and not isinstance(perturb, bool) and perturb == 0:
        return 0, 0
    if isinstance(perturb, (list, tuple)) and len(perturb) == 2 and all(isinstance(v, int) and not isinstance(v, bool) and v == 0 for v in perturb):
        return 0, 0
    ok = isinstance(perturb, (list, tuple)) and len(perturb) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in perturb)
    if not ok or not 0 <= perturb[0] < perturb[1]:
        raise ValueError(f'{name}: {perturb!r} is not 0 or [lo, hi] with ints 0 <= lo < hi (each corner moves by an int in [lo, hi))')
    return int(perturb[0]), int(perturb[1])


def check_window(name, window, h=None, w=None):
    if window is None:
        return None
    if isinstance(window, bool) or not isinstance(window, int) or window < 2:
        raise ValueError(f'{name}: {window!r} is not null or an int of at least 2 (the side of the centred square in pixels)')
    if h is not None and window > min(h, w):
        raise ValueError(f'{name}: {window} is larger than the {h} x {w} image')
    return window


def sample_corner_homographies(n, h, w, perturb, window=None, generator=None):
    """n random sampling matrices [n,3,3] float64 for h x w images, the reference's recipe made reproducible: the corners tl, tr, br,
    bl of the centred square of ``window`` pixels a side (default min(h, w); the square spans window - 1 between its corner
    pixels, centred on ((w - 1) / 2, (h - 1) / 2)) each move in x and in y by a uniform int in [lo, hi) times a random sign, and S
    is the homography square -> quadrilateral (the reference's H: the view shows the quadrilateral's content in the square).
    perturb: [lo, hi] or 0.  hi > window / 4 is a ValueError: every corner then stays in its own quadrant of the square and the
    quadrilateral convex.  perturb 0 returns identities and draws nothing.
    The draws, from ``generator`` (a host torch.Generator; None: torch's global one), in this order: ONE
    torch.randint(lo, hi, (n, 4, 2)) -- image-major, corners tl, tr, br, bl, x before y -- then ONE torch.randint(0, 2, (n, 4, 2)),
    1 meaning a negative sign.  A pure function of the generator's state."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1 or h < 2 or w < 2:
        raise ValueError(f'sample_corner_homographies: n={n!r} images of {h} x {w} (n >= 1, h, w >= 2)')
    lo, hi = check_perturb('sample_corner_homographies: perturb', perturb)
    window = check_window('sample_corner_homographies: window', window, h, w) or min(h, w)
    if hi == 0:
        return torch.eye(3, dtype=torch.float64).repeat(n, 1, 1)
    if hi > window / 4:
        raise ValueError(f'sample_corner_homographies: perturb [{lo}, {hi}): hi > window / 4 = {window / 4} (the quadrilateral would not '
                         'stay convex)')
    mag = torch.randint(lo, hi, (n, 4, 2), generator=generator)
    neg = torch.randint(0, 2, (n, 4, 2), generator=generator)
    cx, cy, r = (w - 1) / 2, (h - 1) / 2, (window - 1) / 2
    square = torch.tensor([[cx - r, cy - r], [cx + r, cy - r], [cx + r, cy + r], [cx - r, cy + r]], dtype=torch.float64)
    quad = square + (mag * (1 - 2 * neg)).to(torch.float64)
    return homography_from_points(square.expand(n, 4, 2), quad)


def similarity(h, w, scale=1.0, rotate_deg=0.0):
    """the sampling matrix [3,3] float64 of the view that shows an h x w image magnified by ``scale`` and turned by ``rotate_deg``
    about its centre c = ((w - 1) / 2, (h - 1) / 2): out(p) = img(c + R(rotate_deg) (p - c) / scale) with R = [[cos, -sin], [sin,
    cos]].  Multiples of 90 degrees use exact 0 and +-1: scale 1 at 0 is the identity, at 180 the double flip (w - 1 - x,
    h - 1 - y), both exact"""
    scale, rotate_deg = float(scale), float(rotate_deg)
    if not (scale > 0 and math.isfinite(scale) and math.isfinite(rotate_deg)):
        raise ValueError(f'similarity: scale {scale!r} (positive) / rotate {rotate_deg!r} (finite degrees)')
    if rotate_deg % 90 == 0:
        cos, sin = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(rotate_deg // 90) % 4]
    else:
        cos, sin = math.cos(math.radians(rotate_deg)), math.sin(math.radians(rotate_deg))
    a, b = cos / scale, sin / scale
    cx, cy = (w - 1) / 2, (h - 1) / 2
    return torch.tensor([[a, -b, (cx - a * cx) + b * cy], [b, a, (cy - b * cx) - a * cy], [0.0, 0.0, 1.0]], dtype=torch.float64)


def _inverse3(m):
    """[..., 3, 3] float64 -> its inverse by the adjugate (exact for the translations and 90-degree turns the tests feed)"""
    a, b, c, d, e, f, g, h, i = (m[..., r, k] for r in range(3) for k in range(3))
    co = [e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d]
    det = a * co[0] + b * co[3] + c * co[6]
    if bool((det == 0).any()) or not bool(torch.isfinite(det).all()):
        raise ValueError('a singular matrix is no homography')
    return torch.stack([v / det for v in co], dim=-1).reshape(*m.shape[:-2], 3, 3)


def to_feature_coords(S):
    """sampling matrices S [..., 3, 3] of HR views -> M = A^-1 S^-1 A float64: M maps a position of the extractor's conv3_1 map of
    the ORIGINAL image to the position of the same content in the map of the VIEW (the view shows the content of p at S^-1 p), A =
    [[4, 0, 1.5], [0, 4, 1.5], [0, 0, 1]] taking cell (i, j) to its centre on the HR grid.  A translation by (4 a, 4 b) becomes the
    translation by (-a, -b), exactly"""
    s = torch.as_tensor(S, dtype=torch.float64)
    if s.shape[-2:] != (3, 3):
        raise ValueError(f'to_feature_coords: [..., 3, 3] matrices expected, got {tuple(s.shape)}')
    k, o = FEATURE_STRIDE, FEATURE_OFFSET
    a = torch.tensor([[k, 0.0, o], [0.0, k, o], [0.0, 0.0, 1.0]], dtype=torch.float64)
    a_inv = torch.tensor([[1 / k, 0.0, -o / k], [0.0, 1 / k, -o / k], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return a_inv @ _inverse3(s) @ a


def indexed_corner_homographies(seed, index, k, h, w, perturb, window=None):
    """the k corner homographies [k,3,3] of validation image ``index``: a pure function of (seed, index, k) and the image size, so
    that checkpoints are compared on the same views (sample_corner_homographies(k, ...) on a fresh generator seeded with
    seed * 1000003 + index)"""
    gen = torch.Generator().manual_seed((int(seed) * 1000003 + int(index)) % (2 ** 63))
    return sample_corner_homographies(k, h, w, perturb, window, gen)


def sample_ref_augment(n, h, w, cfg, generator):
    """train.ref_augment for a stack of n images of h x w: -> [n,3,3] sampling matrices, the identity for the images left alone, or
    None when none was chosen (nothing is launched then).  The draws, in this order: ONE torch.rand(n) -- image i is replaced by
    its view where the value is < p --, then, unless p or perturb is 0, the draws of sample_corner_homographies(n, ...) for ALL n images (the
    generator's state after a batch does not depend on which images were chosen)"""
    chosen = torch.rand(n, generator=generator) < cfg['p']
    if cfg['p'] == 0 or cfg['perturb'][1] == 0:   # (perturb 0: every view is the image itself)
        return None
    sampling = sample_corner_homographies(n, h, w, cfg['perturb'], cfg['window'], generator)
    if not bool(chosen.any()):
        return None
    return torch.where(chosen[:, None, None], sampling, torch.eye(3, dtype=torch.float64))


# ------------------------------------------------------------------ the options
def _mapping(name, v, keys):
    if not isinstance(v, dict):
        raise ValueError(f'{name}: {v!r} is not a mapping of {", ".join(keys)}')
    unknown = sorted(set(v) - set(keys), key=str)
    if unknown:
        raise ValueError(f'{name}: unknown key(s) {unknown} ({", ".join(keys)} are the options)')


def _interp(name, v):
    if not isinstance(v, str) or v not in INTERPS:
        raise ValueError(f'{name}.interp: {v!r} is not one of {", ".join(INTERPS)}')
    return v


def _seed(name, v):
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise ValueError(f'{name}.seed: {v!r} is not a non-negative int')
    return v


def _number(name, v, positive=False):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (positive and not v > 0):
        raise ValueError(f'{name}: {v!r} is not a {"positive" if positive else "finite"} number')
    return float(v)


def parse_ref_augment(train_opt):
    """opt['train'] -> None (ref_augment absent, None or False) or {p, perturb: (lo, hi), window, interp}.  Accepted: a dict
    {p: 0.5, perturb: [5, 20], window: null, interp: bicubic} (the defaults).  Refused by name (ValueError): anything else that is
    not a dict, unknown keys, a p outside [0, 1], a perturb that is not 0 or [lo, hi] with ints 0 <= lo < hi, a window that is not
    null or an int >= 2 (hi > window / 4 is refused here when window is given, else at the first batch, whose size sets it), an
    interp that is not bicubic or bilinear.  The models parse it whether they train or not; only a training model acts on it."""
    v = (train_opt or {}).get('ref_augment')
    if v is None or v is False:
        return None
    name = 'train.ref_augment'
    _mapping(name, v, REF_AUGMENT_KEYS)
    p = v.get('p', 0.5)
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0 <= p <= 1:
        raise ValueError(f'{name}.p: {p!r} is not a probability in [0, 1]')
    lo, hi = check_perturb(f'{name}.perturb', v.get('perturb', [5, 20]))
    window = check_window(f'{name}.window', v.get('window'))
    if window is not None and hi > window / 4:
        raise ValueError(f'{name}.perturb: hi = {hi} > window / 4 = {window / 4} (the quadrilateral would not stay convex)')
    return dict(p=float(p), perturb=(lo, hi), window=window, interp=_interp(name, v.get('interp', 'bicubic')))


def parse_ref_perturb(val_opt):
    """opt['val'] -> None (ref_perturb absent, None or False) or one of two forms: {kind: 'similarity', scale, rotate, interp} from
    {scale: 1.0, rotate: 0} (degrees; either may be left out), or {kind: 'corners', perturb: (lo, hi), window, seed, interp} from
    {perturb: [lo, hi], seed: 0, window: null}.  Refused by name (ValueError): anything else that is not a dict, unknown keys, both
    forms at once (scale / rotate next to perturb / window / seed), an empty dict, a scale that is not a positive number, a rotate
    that is not a finite number, and what parse_ref_augment refuses of perturb, window and interp; a seed that is not an int >= 0."""
    v = (val_opt or {}).get('ref_perturb')
    if v is None or v is False:
        return None
    name = 'val.ref_perturb'
    _mapping(name, v, REF_PERTURB_KEYS)
    sim, cor = [k for k in ('scale', 'rotate') if k in v], [k for k in ('perturb', 'window', 'seed') if k in v]
    if sim and cor:
        raise ValueError(f'{name}: {sim} and {cor} are two forms of the option; use one ({{scale, rotate}} or {{perturb, window, seed}})')
    interp = _interp(name, v.get('interp', 'bicubic'))
    if sim:
        return dict(kind='similarity', scale=_number(f'{name}.scale', v.get('scale', 1.0), positive=True),
                    rotate=_number(f'{name}.rotate', v.get('rotate', 0)), interp=interp)
    if 'perturb' not in v:
        raise ValueError(f'{name}: neither scale / rotate nor perturb is given')
    lo, hi = check_perturb(f'{name}.perturb', v['perturb'])
    window = check_window(f'{name}.window', v.get('window'))
    if window is not None and hi > window / 4:
        raise ValueError(f'{name}.perturb: hi = {hi} > window / 4 = {window / 4} (the quadrilateral would not stay convex)')
    return dict(kind='corners', perturb=(lo, hi), window=window, seed=_seed(name, v.get('seed', 0)), interp=interp)


def parse_match_probe(val_opt):
    """opt['val'] -> None (match_probe absent, None or False) or {perturb: (lo, hi), window, thresholds: (...), margin, source, seed,
    interp}.  Accepted: True (every default) or a dict {perturb: [5, 20], window: null, thresholds: [1, 2], margin: 3, source: gt |
    lq_up, seed: 0, interp: bicubic}.  Refused by name (ValueError): anything else, unknown keys, thresholds that are not a list of
    1 to 4 positive numbers, a margin that is not an int >= 0, an unknown source, a seed that is not an int >= 0, and what
    parse_ref_augment refuses of perturb, window and interp."""
    v = (val_opt or {}).get('match_probe')
    if v is None or v is False:
        return None
    name = 'val.match_probe'
    if v is True:
        v = {}
    _mapping(name, v, MATCH_PROBE_KEYS)
    lo, hi = check_perturb(f'{name}.perturb', v.get('perturb', [5, 20]))
    window = check_window(f'{name}.window', v.get('window'))
    if window is not None and hi > window / 4:
        raise ValueError(f'{name}.perturb: hi = {hi} > window / 4 = {window / 4} (the quadrilateral would not stay convex)')
    thr = v.get('thresholds', [1, 2])
    if not isinstance(thr, (list, tuple)) or not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError(f'{name}.thresholds: {thr!r} is not a list of 1 to {MAX_THRESHOLDS} positive numbers (feature pixels)')
    thr = tuple(_number(f'{name}.thresholds', t, positive=True) for t in thr)
    margin = v.get('margin', 3)
    if isinstance(margin, bool) or not isinstance(margin, int) or margin < 0:
        raise ValueError(f'{name}.margin: {margin!r} is not a non-negative int (feature pixels)')
    source = v.get('source', 'gt')
    if not isinstance(source, str) or source not in PROBE_SOURCES:
        raise ValueError(f'{name}.source: {source!r} is not one of {", ".join(PROBE_SOURCES)}')
    return dict(perturb=(lo, hi), window=window, thresholds=thr, margin=margin, source=source, seed=_seed(name, v.get('seed', 0)),
                interp=_interp(name, v.get('interp', 'bicubic')))


def probe_result_keys(thresholds):
    """the names the probe's numbers are logged and returned under: match_epe, then match_pck<t> per threshold (1 -> match_pck1,
    2.5 -> match_pck2.5)"""
    return ['match_epe'] + [f'match_pck{t:g}' for t in thresholds]


def probe_numbers(stats, thresholds):
    """the summed stats row (count, sum of errors, hits per threshold; host floats) -> {count, match_epe, match_pck...}: the mean
    end-point error in feature pixels and the fraction of counted queries within each threshold; NaN when nothing was counted"""
    count = float(stats[0])
    out = {'count': int(count)}
    for key, v in zip(probe_result_keys(thresholds), stats[1:]):
        out[key] = float(v) / count if count > 0 else float('nan')
    return out
