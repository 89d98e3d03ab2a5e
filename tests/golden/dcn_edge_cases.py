"""Deterministic hostile offset / mask fields for the deformable convolution (plain numpy).

A DCN sample position is  base + tap + offset  with  base = ho * stride - pad  and  tap = i * dilation  (integers), formed in fp32
in that order by every kernel and by oracle/mrefsr_oracle.c.  The position-exact fields below choose a TARGET position per
(b, deformable group, tap, ho, wo) and set  offset = target - (base + tap):  every target is a multiple of 1/8 of small magnitude,
so the offset and the fp32 sum are exact and the sample lands on the target bit for bit -- on the window boundary (-1 and L, the
first positions outside), on integers, inside the two half-open border bands (-1, 0) and (L-1, L), or far outside.

    fields:  lattice, zero, shift, outside, mostly_outside, heavy_tail, mask_zero       (see field())

Each field comes with the targets and the class indices that produced it, so that a test can assert what its inputs cover
(coverage()) and pick out the entries an assertion is about (outside_window()).
"""
from collections import namedtuple

import numpy as np

Field = namedtuple('Field', 'name offset mask ty tx cy cx')
# offset [B, dg*18, Ho, Wo] fp32 ([g][tap][y, x] as the reference lays it out), mask [B, dg*9, Ho, Wo] fp32 or None (DCNv1),
# ty / tx [B, dg, 9, Ho, Wo] fp32 target positions (None for fields that are not position-exact),
# cy / cx [B, dg, 9, Ho, Wo] class index into edge_values() (lattice only)

N_CLASSES = 16
N_PAIRS = N_CLASSES * N_CLASSES
LATTICE_STEP = 101          # coprime to N_PAIRS = 256 (odd), to 9 taps, and no divisor of 32 / 64: pairs drift across taps, groups, tiles
MASK_CYCLE = (1.0, 0.0, 0.25, 1.0, 0.8125, 0.5, 0.0)    # exact 0, exact 1, values in (0, 1); period 7 is coprime to 256
MOSTLY_OUTSIDE_EVERY = 37
FIELDS = ('lattice', 'zero', 'shift', 'outside', 'mostly_outside', 'heavy_tail', 'mask_zero')


def out_size(h, w, stride=1, pad=1, dil=1, k=3):
    return (h + 2 * pad - (dil * (k - 1) + 1)) // stride + 1, (w + 2 * pad - (dil * (k - 1) + 1)) // stride + 1


def edge_values(length):
    """the 16 target positions of one axis of length L, by class index"""
    k = (length - 1) // 2      # an interior integer (0 on a one-pixel axis)
    L = float(length)
    return np.array([-1.125, -1.0, -0.875, -0.5, -0.125, 0.0, 0.125, k, k + 0.5, L - 1.125, L - 1.0, L - 0.875, L - 0.5, L - 0.125, L, L + 0.5],
                    np.float32)


EDGE_NAMES = ('-1.125', '-1', '-0.875', '-0.5', '-0.125', '0', '0.125', 'k', 'k+0.5', 'L-1.125', 'L-1', 'L-0.875', 'L-0.5', 'L-0.125', 'L', 'L+0.5')


def base_positions(b, dg, h, w, stride=1, pad=1, dil=1):
    """integer base + tap of every sample: (by, bx), int64 [1, 1, 9, Ho, Wo] broadcastable to [B, dg, 9, Ho, Wo]"""
    ho, wo = out_size(h, w, stride, pad, dil)
    tap = np.arange(9)
    by = (np.arange(ho) * stride - pad)[None, :, None] + (tap // 3 * dil)[:, None, None]
    bx = (np.arange(wo) * stride - pad)[None, None, :] + (tap % 3 * dil)[:, None, None]
    return (np.broadcast_to(by, (9, ho, wo))[None, None].astype(np.int64), np.broadcast_to(bx, (9, ho, wo))[None, None].astype(np.int64))


def _flat_index(b, dg, ho, wo):
    return np.arange(b * dg * 9 * ho * wo, dtype=np.int64).reshape(b, dg, 9, ho, wo)


def _offsets(ty, tx, by, bx):
    b, dg, _, ho, wo = ty.shape
    off = np.stack([ty - by.astype(np.float32), tx - bx.astype(np.float32)], axis=3)   # [B, dg, 9, 2, Ho, Wo]
    return np.ascontiguousarray(off.reshape(b, dg * 18, ho, wo), dtype=np.float32)


def _mask_cycle(n, b, dg, ho, wo):
    return np.ascontiguousarray(np.array(MASK_CYCLE, np.float32)[n % len(MASK_CYCLE)].reshape(b, dg * 9, ho, wo))


def _outside_targets(n, h, w):
    """targets at least 1.5 pixels beyond the map on one axis or both; the other axis anywhere (inside, on an edge, beyond)"""
    beyond = np.array([1.5, 2.0, 3.25, 17.0, 300.5, 1.0e4, 1.625, 64.0], np.float32)
    free_y = np.concatenate([edge_values(h), [-7.5, h + 40.0]]).astype(np.float32)
    free_x = np.concatenate([edge_values(w), [-7.5, w + 40.0]]).astype(np.float32)
    d = beyond[(n // 4) % len(beyond)]
    kind = n % 4           # 0: above / left of the map on y, 1: below on y, 2: left on x, 3: right on x; every 5th: both axes
    ty = np.where(kind == 0, -d, np.where(kind == 1, (h - 1) + d, free_y[(n // 3) % len(free_y)]))
    tx = np.where(kind == 2, -d, np.where(kind == 3, (w - 1) + d, free_x[(n // 5) % len(free_x)]))
    both = n % 5 == 0
    d2 = beyond[(n // 7) % len(beyond)]
    ty = np.where(both & (kind >= 2), np.where(n % 2 == 0, -d2, (h - 1) + d2), ty)
    tx = np.where(both & (kind < 2), np.where(n % 3 == 0, -d2, (w - 1) + d2), tx)
    return ty.astype(np.float32), tx.astype(np.float32)


def field(name, b, dg, h, w, stride=1, pad=1, dil=1, with_mask=True, shift=(0, 0), seed=0):
    """one field for a 3 x 3 DCN on a [b, *, h, w] map; with_mask=False: DCNv1 (mask None)"""
    ho, wo = out_size(h, w, stride, pad, dil)
    by, bx = base_positions(b, dg, h, w, stride, pad, dil)
    n = _flat_index(b, dg, ho, wo)
    shape5 = (b, dg, 9, ho, wo)
    ones = np.ones((b, dg * 9, ho, wo), np.float32) if with_mask else None
    if name == 'lattice':
        pair = (n * LATTICE_STEP) % N_PAIRS
        cy, cx = pair // N_CLASSES, pair % N_CLASSES
        ty, tx = edge_values(h)[cy], edge_values(w)[cx]
        return Field(name, _offsets(ty, tx, by, bx), _mask_cycle(n, b, dg, ho, wo) if with_mask else None, ty, tx, cy, cx)
    if name == 'zero':
        ty, tx = np.broadcast_to(by, shape5).astype(np.float32), np.broadcast_to(bx, shape5).astype(np.float32)
        return Field(name, np.zeros((b, dg * 18, ho, wo), np.float32), ones, ty, tx, None, None)
    if name == 'shift':
        ty = np.broadcast_to(by + int(shift[0]), shape5).astype(np.float32)
        tx = np.broadcast_to(bx + int(shift[1]), shape5).astype(np.float32)
        return Field(f'shift{tuple(shift)}', _offsets(ty, tx, by, bx), ones, ty, tx, None, None)
    if name in ('outside', 'mostly_outside'):
        ty, tx = _outside_targets(n, h, w)
        if name == 'mostly_outside':
            back = n % MOSTLY_OUTSIDE_EVERY == 0
            frac = np.array([0.125, 0.5, 0.875, 0.25], np.float32)
            ty = np.where(back, (h - 1) // 2 + frac[(n // MOSTLY_OUTSIDE_EVERY) % 4], ty).astype(np.float32)
            tx = np.where(back, (w - 1) // 2 + frac[(n // (4 * MOSTLY_OUTSIDE_EVERY)) % 4], tx).astype(np.float32)
        mask = None
        if with_mask:
            mask = _mask_cycle(n, b, dg, ho, wo) if name == 'outside' else ones
        return Field(name, _offsets(ty, tx, by, bx), mask, ty, tx, None, None)
    rng = np.random.default_rng(1000 + seed)
    if name == 'heavy_tail':
        off = rng.standard_normal((b, dg * 18, ho, wo)) * 2.0
        off = np.where(rng.random(off.shape) < 0.03, off * 40.0, off).astype(np.float32)
        mask = rng.random((b, dg * 9, ho, wo)).astype(np.float32) if with_mask else None
        return Field(name, off, mask, None, None, None, None)
    if name == 'mask_zero':
        off = (rng.standard_normal((b, dg * 18, ho, wo)) * 3.0).astype(np.float32)
        return Field(name, off, np.zeros((b, dg * 9, ho, wo), np.float32), None, None, None, None)
    raise ValueError(name)


def positions_fp32(f, h, w, stride=1, pad=1, dil=1):
    """the sample positions as the kernels form them: fp32(base + tap) + fp32 offset -> (py, px) [B, dg, 9, Ho, Wo] fp32"""
    b = f.offset.shape[0]
    dg = f.offset.shape[1] // 18
    ho, wo = f.offset.shape[2:]
    by, bx = base_positions(b, dg, h, w, stride, pad, dil)
    off = f.offset.reshape(b, dg, 9, 2, ho, wo)
    return by.astype(np.float32) + off[:, :, :, 0], bx.astype(np.float32) + off[:, :, :, 1]


def outside_window(ty, tx, h, w):
    """True where the reference takes the sample for empty: not inside (-1, H) x (-1, W)   (deform_conv_cuda_kernel.cu:531, :618)"""
    return (ty <= -1) | (ty >= h) | (tx <= -1) | (tx >= w)


def coverage(f):
    """which (y-class, x-class) pairs of a lattice field landed where: {'tap': [9 sets], 'group': [dg sets], 'tile64': set, 'tile32': set,
    'unmasked': set} -- the pairs under each tap, in each deformable group, in the last (ragged or only) 64- and 32-pixel tile of
    every image, and with a nonzero mask anywhere"""
    b, dg, _, ho, wo = f.cy.shape
    pair = (f.cy * N_CLASSES + f.cx).reshape(b, dg, 9, ho * wo)
    hw = ho * wo
    rep = {'tap': [set(np.unique(pair[:, :, t]).tolist()) for t in range(9)],
           'group': [set(np.unique(pair[:, g]).tolist()) for g in range(dg)],
           'tile64': set(np.unique(pair[..., (hw - 1) // 64 * 64:]).tolist()),
           'tile32': set(np.unique(pair[..., (hw - 1) // 32 * 32:]).tolist())}
    if f.mask is None:
        rep['unmasked'] = set(np.unique(pair).tolist())
    else:
        rep['unmasked'] = set(np.unique(pair[f.mask.reshape(b, dg, 9, hw) != 0]).tolist())
    return rep


def missing_pairs(f):
    """[(where, [pair names])] for every place coverage() found short of all 256 pairs; empty when the field covers everything"""
    rep, full, out = coverage(f), set(range(N_PAIRS)), []

    def names(s):
        return [f'(y {EDGE_NAMES[p // N_CLASSES]}, x {EDGE_NAMES[p % N_CLASSES]})' for p in sorted(s)]
    for t, s in enumerate(rep['tap']):
        if s != full:
            out.append((f'tap {t}', names(full - s)))
    for g, s in enumerate(rep['group']):
        if s != full:
            out.append((f'deformable group {g}', names(full - s)))
    for key in ('tile64', 'tile32', 'unmasked'):
        if rep[key] != full:
            out.append((key, names(full - rep[key])))
    return out


def covering_batch(b, dg, h, w, stride=1, pad=1, dil=1, with_mask=True, limit=64):
    """the smallest batch >= b at which the lattice field of this geometry covers every pair in every place coverage() looks at:
    a map too small to hold 256 pairs under each tap or in its last 32-pixel tile gets more images, never a weaker assertion"""
    for bb in range(b, limit + 1):
        if not missing_pairs(field('lattice', bb, dg, h, w, stride, pad, dil, with_mask)):
            return bb
    raise ValueError(f'no batch <= {limit} covers every pair for dg={dg}, {h}x{w}, stride {stride}, pad {pad}, dilation {dil}')


# ---------------------------------------------------------------------------------------------------------------------------------
# The geometries the edge tests run (tests/test_dcn_edges_cpu.py asserts the coverage of every one, tests/test_dcn_edges_gpu.py
# runs the kernels on them).  Maps: H != W, W no multiple of 4; 9 x 11 = 99 pixels (one tile group at T = 2, ragged at T = 4, ragged
# 32-pixel tile), 13 x 21 = 273 pixels (five 64-pixel tiles: the last tile group is partial), and two thin maps on which both clamped
# corners of an axis coincide.
MAPS = ((2, 9, 11), (2, 13, 21), (1, 1, 70), (1, 5, 1))      # (default batch, H, W)

# (C, Co, dg, groups, stride, pad, dil, with_mask): the channel / geometry settings behind the kernel paths
GEOMETRIES = {
    'c64': (64, 64, 8, 1, 1, 1, 1, True),
    'c128': (128, 128, 8, 1, 1, 1, 1, True),
    'c128_64': (128, 64, 8, 1, 1, 1, 1, True),
    'c256': (256, 256, 8, 1, 1, 1, 1, True),
    'c64_dg1_v1': (64, 64, 1, 1, 1, 1, 1, False),
    'c64_dg2_v1': (64, 64, 2, 1, 1, 1, 1, False),
    'g8_dg4': (8, 8, 4, 1, 1, 1, 1, True),
    'g8_4_dg2_groups2_stride2': (8, 4, 2, 2, 2, 1, 1, True),
    'g12_20_dg3_dil2': (12, 20, 3, 1, 1, 2, 2, True),
}
# the maps each geometry is run on: the two default maps everywhere, the thin maps where they are cheap and reach another kernel
GEOMETRY_MAPS = {
    'c64': MAPS, 'c128': MAPS[:2], 'c128_64': MAPS[:2], 'c256': MAPS[:2], 'c64_dg1_v1': MAPS[:2], 'c64_dg2_v1': MAPS[:2],
    'g8_dg4': MAPS, 'g8_4_dg2_groups2_stride2': MAPS[:2], 'g12_20_dg3_dil2': MAPS[:2],
}


def cases():
    """[(geometry name, (B, H, W))]"""
    return [(name, m) for name in GEOMETRIES for m in GEOMETRY_MAPS[name]]


_batch_cache = {}


def lattice_batch(geometry, bhw):
    """the batch the lattice field of (geometry, map) is run at: the map's default batch, or the next larger one that covers"""
    key = (geometry, tuple(bhw))
    if key not in _batch_cache:
        _, _, dg, _, stride, pad, dil, with_mask = GEOMETRIES[geometry]
        b, h, w = bhw
        _batch_cache[key] = covering_batch(b, dg, h, w, stride, pad, dil, with_mask)
    return _batch_cache[key]


def inputs(geometry, b, h, w):
    """(x [b, C, h, w], weight [Co, C / groups, 3, 3], bias [Co]) fp32, seeded by the geometry and the map: no value is zero, so a
    corner that wrongly takes part shows"""
    c, co, _, groups = GEOMETRIES[geometry][:4]
    rng = np.random.default_rng([c, co, groups, b, h, w])
    x = rng.standard_normal((b, c, h, w)).astype(np.float32)
    weight = (rng.standard_normal((co, c // groups, 3, 3)) * (2.0 / (c * 9)) ** 0.5).astype(np.float32)
    bias = rng.standard_normal(co).astype(np.float32)
    return x, weight, bias


def shifted_conv2d(x, weight, bias, stride, pad, dil, groups, shift=(0, 0)):
    """the closed form of a DCN whose every offset is the whole-pixel shift (dy, dx) and whose mask is 1: the plain convolution of
    the map translated with zero fill (torch tensors of one dtype in, differentiable; shift (0, 0): F.conv2d itself).  The padding
    ring is translated with the map -- position -1 + 2 reads row 1 -- so the translated window is cut from a zero canvas and
    convolved without padding."""
    import torch.nn.functional as F
    dy, dx = int(shift[0]), int(shift[1])
    h, w = x.shape[2:]
    m = pad + max(abs(dy), abs(dx))
    canvas = F.pad(x, (m, m, m, m))
    win = canvas[:, :, m - pad + dy:m - pad + dy + h + 2 * pad, m - pad + dx:m - pad + dx + w + 2 * pad]
    return F.conv2d(win, weight, bias, stride, 0, dil, groups)
