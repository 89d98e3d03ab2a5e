#!/usr/bin/env python3
"""Bits of kernels for a fixed, seeded case list (--list, default split16).  An output above BIG bytes is kept as its SHA-256
(equal digests = equal bits).

  split16     the kernels that rest on csrc/split16.h: one case per kernel template that calls the header's scale, splits or MFMA
              wrappers, at the smallest shapes the launchers send there.  Inputs come from a CPU generator and mix magnitudes from
              1e-6 to 1e3 (low terms in the fp16 subnormals); every scaled case also runs with amax = 0 (the guard's unscaled path).
  dcn_sample  the DCN kernel paths that sample through csrc/dcn_sample.h and the split16 list does not reach, on the lattice and
              heavy_tail fields of tests/golden/dcn_edge_cases.py (first map of each geometry).  grad_x of dcn_col2im and of
              dcn_bwd_data, a float-atomic scatter, is not part of the list: the tolerance tests hold it.
  gram        the Gram kernels of the style term and the texture loss (csrc/percep.hip, csrc/texture.hip, whose backward bodies are
              csrc/gram.h): gram_nhwc, gram_raw_nhwc and both backwards, fresh and accumulated onto a seeded base (texture also with
              norm == 0), at N = 2 on C = 64, 3 x 3 (one block, 9 of 16 lanes) and C = 128, 9 x 9 (two column blocks, a pixel block
              with a one-pixel wave and two empty ones, the forward's mirrored tile and split-K).  No float atomic: nothing is left out.
  blend_conv  mrattn_blend_conv_kernel (csrc/mrattn_conv.hip) at C = 64, 128 and 256, N = 2, on maps of 4 x 4 (smaller than any
              tile), 12 x 20 (ragged both ways) and 19 x 70 (several tile rows and columns, a tile count that is no multiple of 8):
              T = 5 without a mask, T = 5 with valid_bits that leave two references to sample 0 and none to sample 1, and at C = 64
              T = 7 (reference groups of 5 + 2).  References of mixed magnitudes; every case as plain / amax / amax0.  Nothing is left out.

    python tools/kernel_bits.py --pin tests/golden/split16_bits.npz                         # regenerate a fixture (tools/README.md)
    python tools/kernel_bits.py --list dcn_sample --pin tests/golden/dcn_sample_bits.npz [--note 'which library recorded it']
    python tools/kernel_bits.py --list gram --pin tests/golden/gram_bits.npz --note 'which library recorded it'
    python tools/kernel_bits.py --list blend_conv --pin tests/golden/blend_conv_bits.npz --note 'which library recorded it'
    python tools/kernel_bits.py [--list NAME] out.npz                                       # one run of the list

--pin runs every case twice; an output that does not repeat is left out and named under the key `excluded` with the reason (at
most two outputs of the split16 list, none of the dcn_sample, gram and blend_conv lists); --note TEXT is stored under the key `note`.
tests/test_split16_bits_gpu.py, tests/test_dcn_sample_bits_gpu.py, tests/test_gram_bits_gpu.py and tests/test_blend_conv_bits_gpu.py run the lists on the tree's library
and compare per output."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
BIG = 16 << 10
MAX_EXCLUDED = 2


def mixed(rng, shape, scale=1.0):
    """normal values times 10^u, u uniform in [-6, 3]"""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-6.0, 3.0, shape) * scale).astype(np.float32)


def cases():
    """-> {case name: [outputs as numpy arrays]} (insertion order fixed)"""
    import torch
    from mrefsr_amd import hip
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    out = {}

    def amax_variants(name, x_abs_max, run, scaled_only=False):
        """run(in_amax) for in_amax = None (where the wrapper takes it), max |x| and 0"""
        variants = [] if scaled_only else [('plain', None)]
        variants += [('amax', dev(np.array([x_abs_max], np.float32))), ('amax0', dev(np.zeros(1, np.float32)))]
        for tag, am in variants:
            res = run(am)
            res = res if isinstance(res, (list, tuple)) else [res]
            out[f'{name}.{tag}'] = [r.detach().cpu().numpy() for r in res if r is not None]

    def conv(name, seed, h, w, ci, co, k, terms):
        rng = np.random.default_rng(seed)
        x = mixed(rng, (1, h, w, ci))
        wt = dev((rng.standard_normal((co, ci, k, k)) * (2.0 / (ci * k * k)) ** 0.5).astype(np.float32))
        bias, res = dev(rng.standard_normal(co).astype(np.float32)), dev(mixed(rng, (1, h, w, co)))
        pk, xd = hip.conv_pack_weight(wt, terms), dev(x)
        amax_variants(name, np.abs(x).max(), lambda am: hip.conv_nhwc(xd, pk, bias, co, k, residual=res, act=True, slope=0.1, in_amax=am))

    # ---- conv_nhwc.hip: the direct kernel (4-row tiles at this size), the eight-wave kernel (>= 256 pairs of cout blocks), the 1x1 kernel
    # (> 128 blocks of 16-row tiles); conv_wino.hip (a side that is no multiple of 16) and conv_wino4.hip (whole 16 x 16 tiles)
    conv('conv3x3_t16', 1, 17, 33, 16, 64, 3, 16)
    conv('conv8_t16', 2, 241, 481, 16, 128, 3, 16)
    conv('conv1x1_t16', 3, 129, 225, 16, 128, 1, 16)
    conv('conv_wino_t17', 4, 17, 17, 48, 64, 3, 17)
    conv('conv_wino4_t17', 5, 16, 32, 48, 64, 3, 17)

    # ---- the input-gradient convolution with its statistics (fixed-order sums: deterministic mode)
    rng = np.random.default_rng(6)
    g = mixed(rng, (1, 17, 33, 16), 1e-6)
    wt = (rng.standard_normal((16, 16, 3, 3)) * 0.05).astype(np.float32)
    pk = hip.conv_pack_view(dev(wt), None, 16, dgrad=True, wscale=2.0 ** (13 - int(np.floor(np.log2(np.abs(wt).max())))))
    gd, t = dev(g), dev(rng.standard_normal((1, 17, 33, 16)).astype(np.float32))
    with hip.deterministic(True):
        amax_variants('conv_nhwc_bwd', np.abs(g).max(), lambda am: hip.conv_nhwc_bwd(gd, pk, 16, 3, residual=t, residual_is_mask=True, in_amax=am),
                      scaled_only=True)

    # ---- dcn.hip: H W = 65 pixels of the 64-pixel tile; C = 32 stays on the one-tile kernel, C = 64 goes to the two-tile kernel;
    # terms 16 by default, the bf16 three-term split (terms 6) with range_free
    for name, c, dg in (('dcn_fwd_1tile', 32, 4), ('dcn_fwd_2tile', 64, 8)):
        rng = np.random.default_rng(10 + c)
        x, off = dev(mixed(rng, (1, 5, 13, c))), dev((rng.standard_normal((1, dg * 18, 5, 13)) * 3).astype(np.float32))
        msk = dev(rng.random((1, dg * 9, 5, 13)).astype(np.float32))
        wgt = dev((rng.standard_normal((64, c, 3, 3)) * (2.0 / (c * 9)) ** 0.5).astype(np.float32))
        bias = dev(rng.standard_normal(64).astype(np.float32))
        for tag, rf in (('t16', False), ('t6', True)):
            out[f'{name}.{tag}'] = [hip.dcn_fwd(x, off, msk, wgt, bias, 1, 1, 1, 1, dg, 0.1, channels_last=True, range_free=rf).cpu().numpy()]

    # ---- dcn_bwd.hip: the two fused backward kernels and the 1x1 weight gradient (with their reduce kernels)
    rng = np.random.default_rng(20)
    c, co, dg = 32, 64, 4
    x, off = dev(mixed(rng, (1, 5, 13, c))), dev((rng.standard_normal((1, dg * 18, 5, 13)) * 3).astype(np.float32))
    msk = dev(rng.random((1, dg * 9, 5, 13)).astype(np.float32))
    wt = (rng.standard_normal((co, c, 3, 3)) * (2.0 / (c * 9)) ** 0.5).astype(np.float32)
    g = mixed(rng, (1, 5, 13, co), 1e-6)
    gd = dev(g)
    pkT = hip.conv_pack_view(dev(wt), None, 16, dgrad='T', wscale=2.0 ** (13 - int(np.floor(np.log2(np.abs(wt).max())))))
    with hip.deterministic(False):   # (the input gradient is a float-atomic scatter: pinned only if it repeats)
        amax_variants('dcn_bwd_data', np.abs(g).max(), lambda am: hip.dcn_bwd_data(gd, x, off, msk, pkT, dg, g_amax=am), scaled_only=True)
    amax_variants('dcn_bwd_weight', np.abs(g).max(), lambda am: hip.dcn_bwd_weight(gd, x, off, msk, co, dg, g_amax=am), scaled_only=True)
    rng = np.random.default_rng(21)
    x1, g1 = dev(mixed(rng, (1, 5, 13, 16))), mixed(rng, (1, 5, 13, 16), 1e-6)
    g1d = dev(g1)
    amax_variants('conv_wgrad1x1', np.abs(g1).max(), lambda am: hip.conv_wgrad1x1(x1, g1d, 16, 16, am), scaled_only=True)

    # ---- wgrad.hip
    rng = np.random.default_rng(22)
    x3, g3 = dev(mixed(rng, (1, 17, 33, 16))), mixed(rng, (1, 17, 33, 16), 1e-6)
    g3d = dev(g3)
    amax_variants('conv_wgrad3x3', np.abs(g3).max(), lambda am: hip.conv_wgrad3x3(x3, g3d, 16, 16, am), scaled_only=True)

    # ---- mrattn_conv.hip: t = 2 references of 64 channels
    rng = np.random.default_rng(23)
    c, t_ = 64, 2
    refs = mixed(rng, (t_, 17, 33, c))
    q, emb = dev(rng.standard_normal((1, 17, 33, c)).astype(np.float32)), dev(rng.standard_normal((t_, 17, 33, c)).astype(np.float32))
    pkb = hip.conv_pack_weight(dev((rng.standard_normal((2 * c, c, 3, 3)) / (9 * c) ** 0.5).astype(np.float32)), 16)
    bias, refs_d = dev(rng.standard_normal(2 * c).astype(np.float32)), dev(refs)
    prob = hip.mrattn_prob_nhwc(q, emb, t_, None, q_scale=c ** -0.5)
    amax_variants('mrattn_blend_conv', np.abs(refs).max(), lambda am: hip.mrattn_blend_conv(refs_d, prob, pkb, bias, t_, None, in_amax=am))
    hip.conv_range_tripped(reset=True)   # (values of 1e3 are far inside the fp16 range; the flag is not part of the bits)
    return out


def dcn_sample_cases():
    """-> {case name: [outputs as numpy arrays]} (insertion order fixed)"""
    import torch
    from mrefsr_amd import hip
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import dcn_edge_cases as E
    dev = lambda a, dt=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dt or torch.float32)   # noqa: E731
    nhwc = lambda a, dt=None: dev(a, dt).permute(0, 2, 3, 1).contiguous()   # noqa: E731
    out = {}

    def fields(geometry, with_mask=None):
        """(tag, Field, x, weight, bias) for the lattice and the heavy_tail field on the geometry's first map"""
        c, co, dg, groups, stride, pad, dil, wm = E.GEOMETRIES[geometry]
        wm = wm if with_mask is None else with_mask
        bhw = E.GEOMETRY_MAPS[geometry][0]
        for name in ('lattice', 'heavy_tail'):
            b = E.covering_batch(bhw[0], dg, bhw[1], bhw[2], stride, pad, dil, wm) if name == 'lattice' else bhw[0]
            yield (name, E.field(name, b, dg, bhw[1], bhw[2], stride, pad, dil, wm)) + E.inputs(geometry, b, bhw[1], bhw[2])

    def fwd(case, geometry, pt='1', t='2', dt=None, x_dt=None, **kw):
        c, co, dg, groups, stride, pad, dil, _ = E.GEOMETRIES[geometry]
        cl = kw.get('channels_last', False)
        os.environ['MREFSR_DCN_PT'], os.environ['MREFSR_DCN_T'] = pt, t     # (read per call by the launcher)
        for tag, f, x, wgt, bias in fields(geometry):
            y = hip.dcn_fwd(nhwc(x, x_dt or dt) if cl else dev(x, x_dt or dt), dev(f.offset, dt), dev(f.mask, dt), dev(wgt, dt), dev(bias, dt), stride, pad, dil,
                            groups, dg, 0.1, **kw)
            out[f'{case}.{tag}'] = [y.view(torch.int16).cpu().numpy() if y.dtype == torch.bfloat16 else y.cpu().numpy()]

    def columns(case, geometry, with_mask, dt=None):
        """dcn_im2col, then dcn_col2im of a seeded column gradient: columns, grad_offset, grad_mask"""
        c, co, dg, groups, stride, pad, dil, _ = E.GEOMETRIES[geometry]
        for tag, f, x, wgt, bias in fields(geometry, with_mask):
            dx, doff, dm = dev(x, dt), dev(f.offset, dt), dev(f.mask, dt)
            col = hip.dcn_im2col(dx, doff, dm, wgt.shape, stride, pad, dil, groups, dg)
            gcol = dev(np.random.default_rng(3).standard_normal(tuple(col.shape)), dt)
            _, goff, gm = hip.dcn_col2im(gcol, dx, doff, dm, wgt.shape, stride, pad, dil, groups, dg)
            out[f'{case}.{tag}'] = [a.cpu().numpy() for a in (col, goff, gm) if a is not None]

    def fused_bwd(case, geometry):
        c, co, dg = E.GEOMETRIES[geometry][:3]
        for tag, f, x, wgt, bias in fields(geometry):
            g = (np.random.default_rng(4).standard_normal((x.shape[0], co) + f.offset.shape[2:]) * 1e-6).astype(np.float32)
            pk = hip.conv_pack_view(dev(wgt), None, 16, dgrad='T', wscale=2.0 ** (13 - int(np.floor(np.log2(np.abs(wgt).max())))))
            _, goff, gm = hip.dcn_bwd_data(nhwc(g), nhwc(x), dev(f.offset), dev(f.mask), pk, dg, g_amax=dev(np.array([np.abs(g).max()])))
            out[f'{case}.{tag}'] = [goff.cpu().numpy(), gm.cpu().numpy()]

    keep = {k: os.environ.get(k) for k in ('MREFSR_DCN_PT', 'MREFSR_DCN_T')}
    try:
        with hip.deterministic(False):   # (the scatter runs; its output is not kept)
            for geometry in ('g8_dg4', 'g8_4_dg2_groups2_stride2', 'g12_20_dg3_dil2'):     # the portable fp32 forward
                fwd(f'fwd_portable_{geometry}', geometry)
            columns('columns_f32_mask', 'g8_dg4', True)
            columns('columns_f32_nomask', 'g8_dg4', False)
            fwd('fwd_mfma_nchw_gather', 'c64_dg1_v1', nhwc_gather=False)                   # dcn_fwd_mfma_kernel, DCNv1
            fwd('fwd_one_tile_c256', 'c256', channels_last=True)                           # dcn_fwd_bf16_kernel
            fwd('fwd_pt_paired_c128', 'c128', channels_last=True)                          # dcn_fwd_pt_kernel, paired gather
            fwd('fwd_pt_map8_c128_64', 'c128_64', channels_last=True)                      # ... eight-channel mapping
            fwd('fwd_bf16_arith_f32_storage', 'c64', channels_last=True, bf16_arith=True)
            fwd('fwd_bf16_arith_bf16_storage', 'c64', x_dt=torch.bfloat16, channels_last=True, bf16_arith=True)
            fused_bwd('bwd_data_cpg16', 'c128')
            fused_bwd('bwd_data_cpg32', 'c256')
            for tag, dt in (('f64', torch.float64), ('f16', torch.float16)):               # csrc/dcn_any.hip's other dtypes
                fwd(f'fwd_{tag}', 'g8_dg4', dt=dt)
                columns(f'columns_{tag}', 'g8_dg4', True, dt=dt)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return out


GRAM_SHAPES = ((64, 3, 3), (128, 9, 9))   # (C, h, w), N = 2
GRAM_OUTPUTS = ('gram', 'gram_raw', 'bwd_fresh', 'bwd_acc', 'texture_bwd_fresh', 'texture_bwd_acc', 'texture_bwd_norm0')


def gram_cases():
    """-> {case name: [outputs as numpy arrays]} (insertion order fixed).  The backwards give [df, max |df|]; texture_bwd_norm0 gives
    [df, max |df|, the base it accumulated onto] (df has the base's bits)."""
    import torch
    from mrefsr_amd import hip
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    out = {}
    for c, h, w in GRAM_SHAPES:
        rng = np.random.default_rng(100 + c)
        f, f2 = dev(mixed(rng, (2, h, w, c))), dev(mixed(rng, (2, h, w, c)))
        base = mixed(rng, (2, h, w, c))
        coeff, norm = dev(rng.random((2, h, w)).astype(np.float32)), dev(np.array([7.5], np.float32))
        gup, zero = dev(np.array([0.37], np.float32)), dev(np.zeros(1, np.float32))
        gx, gg = hip.gram_nhwc(f), hip.gram_nhwc(f2)          # two different maps: both signs, exact zeros on no diagonal
        rx, rm = hip.gram_raw_nhwc(f), hip.gram_raw_nhwc(f2)

        def bwd(run, acc):
            df = dev(base) if acc else torch.empty_like(f)
            amax = run(df, gup if acc else None, acc)
            return [df.cpu().numpy(), amax.cpu().numpy()]

        style = lambda df, up, acc: hip.gram_bwd_nhwc(f, gx, gg, df, 0.8, 1.5, gup=up, accumulate=acc)   # noqa: E731
        tex = lambda nrm: lambda df, up, acc: hip.texture_gram_bwd_nhwc(f, rx, rm, coeff, nrm, df, 1e-3, gup=up, accumulate=acc)   # noqa: E731
        res = [[gx.cpu().numpy()], [rx.cpu().numpy()], bwd(style, False), bwd(style, True), bwd(tex(norm), False), bwd(tex(norm), True),
               bwd(tex(zero), True) + [base]]
        for name, r in zip(GRAM_OUTPUTS, res):
            out[f'{name}.c{c}_{h}x{w}'] = r
    return out


BLEND_MAPS = ((4, 4), (12, 20), (19, 70))   # (h, w), N = 2
BLEND_MASK = (0b10010, 0)                   # valid_bits of the masked cases: references 1 and 4 for sample 0, none for sample 1


def blend_inputs(seed, c, t, h, w, n=2):
    """seeded CPU inputs of one blend_conv case: refs [t*n,h,w,c] of mixed magnitudes and weights prob [n,h,w,t] >= 0 whose sum
    over t stays below 1 (adds and one division per element: the same bits from every numpy)"""
    rng = np.random.default_rng(seed)
    refs = mixed(rng, (t * n, h, w, c))
    r = rng.random((n, h, w, t), dtype=np.float32) + np.float32(0.01)
    tot = np.zeros((n, h, w), np.float32)
    for k in range(t):
        tot = tot + r[..., k]
    return refs, (r / (tot * np.float32(1.01))[..., None]).astype(np.float32)


def blend_weights(c):
    """seeded conv_ass weight [2c,c,3,3] and bias [2c] of the blend_conv list"""
    rng = np.random.default_rng(300 + c)
    return (rng.standard_normal((2 * c, c, 3, 3)) / (9 * c) ** 0.5).astype(np.float32), rng.standard_normal(2 * c).astype(np.float32)


def blend_conv_cases():
    """-> {case name: [output]} (insertion order fixed).  A masked case multiplies prob by the mask (an absent reference's weight is
    exactly 0, as mrattn_prob_nhwc leaves it); its sample 1 has no reference at all."""
    import torch
    from mrefsr_amd import hip
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    out = {}
    for c in (64, 128, 256):
        wt, bias = blend_weights(c)
        pk, bias_d = hip.conv_pack_weight(dev(wt), 16), dev(bias)
        for h, w in BLEND_MAPS:
            for tag, t, masked in (('t5', 5, False), ('t5_masked', 5, True)) + ((('t7', 7, False),) if c == 64 else ()):
                refs, prob = blend_inputs(1000 * c + 10 * h + t + masked, c, t, h, w)
                vb = None
                if masked:
                    present = np.array([[(m >> k) & 1 for k in range(t)] for m in BLEND_MASK], np.float32)
                    prob = prob * present[:, None, None, :]
                    vb = dev(np.array(BLEND_MASK, np.int32))
                refs_d, prob_d = dev(refs), dev(prob)
                for var, am in (('plain', None), ('amax', dev(np.array([np.abs(refs).max()], np.float32))), ('amax0', dev(np.zeros(1, np.float32)))):
                    y = hip.mrattn_blend_conv(refs_d, prob_d, pk, bias_d, t, vb, in_amax=am)
                    out[f'c{c}_{h}x{w}_{tag}.{var}'] = [y.cpu().numpy()]
    hip.conv_range_tripped(reset=True)   # (values of 1e3 are far inside the fp16 range; the flag is not part of the bits)
    return out


# name: (case list, outputs --pin may leave out)
LISTS = {'split16': (cases, MAX_EXCLUDED), 'dcn_sample': (dcn_sample_cases, 0), 'gram': (gram_cases, 0), 'blend_conv': (blend_conv_cases, 0)}


def flatten(res):
    """{case: [arrays]} -> {'case/i': array, or its SHA-256 as uint8[32] above BIG bytes}"""
    flat = {}
    for name, arrs in res.items():
        for i, a in enumerate(arrs):
            a = np.ascontiguousarray(a)
            flat[f'{name}/{i}'] = a if a.nbytes <= BIG else np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8).copy()
    return flat


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()   # (bits: a NaN equals itself)


def main(argv):
    argv, opt = list(argv), {'--list': 'split16', '--note': ''}
    for name in opt:
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    pin = '--pin' in argv
    paths = [a for a in argv if not a.startswith('--')]
    if len(paths) != 1 or opt['--list'] not in LISTS:
        sys.exit(__doc__)
    run, most = LISTS[opt['--list']]
    first = flatten(run())
    excluded = []
    if pin:
        second = flatten(run())
        excluded = [k for k in first if not same(first[k], second[k])]
        if len(excluded) > most:
            sys.exit(f'{len(excluded)} outputs do not repeat (at most {most} may be left out): {excluded}')
        for k in excluded:
            del first[k]
    if opt['--note']:
        first['note'] = np.array([opt['--note']], dtype='U512')
    np.savez_compressed(paths[0], excluded=np.array([f'{k}: did not repeat in two runs of the pinning library' for k in excluded], dtype='U128'),
                        **first)
    first.pop('note', None)
    print(f'list {opt["--list"]}: {len(first)} outputs of {len(set(k.split("/")[0] for k in first))} cases -> {paths[0]} ({os.path.getsize(paths[0])} bytes); excluded: {excluded}')


if __name__ == '__main__':
    main(sys.argv[1:])
