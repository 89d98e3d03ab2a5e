#!/usr/bin/env python3
"""Bits of the kernels that rest on csrc/split16.h, for a fixed, seeded case list: one case per kernel template that calls the
header's scale, splits or MFMA wrappers, at the smallest shapes the launchers send there.  Inputs come from a CPU generator and
mix magnitudes from 1e-6 to 1e3 (low terms in the fp16 subnormals); every scaled case also runs with amax = 0 (the guard's
unscaled path).  An output above BIG bytes is kept as its SHA-256 (equal digests = equal bits).

    python tools/kernel_bits.py --pin tests/golden/split16_bits.npz     # regenerate the fixture (tools/README.md)
    python tools/kernel_bits.py out.npz                                 # one run of the list

--pin runs every case twice; an output that does not repeat is left out and named under the key `excluded` with the reason.
tests/test_split16_bits_gpu.py runs the list on the tree's library and compares per output."""
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
    pin = '--pin' in argv
    paths = [a for a in argv if not a.startswith('--')]
    if len(paths) != 1:
        sys.exit(__doc__)
    first = flatten(cases())
    excluded = []
    if pin:
        second = flatten(cases())
        excluded = [k for k in first if not same(first[k], second[k])]
        if len(excluded) > MAX_EXCLUDED:
            sys.exit(f'{len(excluded)} outputs do not repeat (at most {MAX_EXCLUDED} may be left out): {excluded}')
        for k in excluded:
            del first[k]
    np.savez_compressed(paths[0], excluded=np.array([f'{k}: did not repeat in two runs of the pinning library' for k in excluded], dtype='U128'),
                        **first)
    print(f'{len(first)} outputs of {len(set(k.split("/")[0] for k in first))} cases -> {paths[0]} ({os.path.getsize(paths[0])} bytes); excluded: {excluded}')


if __name__ == '__main__':
    main(sys.argv[1:])
