#!/usr/bin/env python3
"""Times of the DCN paths tools/kbench.py does not reach: the portable fp32 hip.dcn_im2col + hip.dcn_col2im, the portable forward,
and the fused backward (hip.dcn_bwd_data / hip.dcn_bwd_weight at 8, 16 and 32 channels per group).  HIP events, median (minimum).
    [MREFSR_HIP_LIB=another build] [DCN_TIME_ITERS=300: the two portable lines only, that many calls] python tools/dcn_time.py TAG"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
from mrefsr_amd import hip
import dcn_edge_cases as E

ITERS = int(os.environ.get('DCN_TIME_ITERS', '0'))
def timeit(fn, warm=5, iters=40):
    iters = ITERS or iters
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3

tag = sys.argv[1]
torch.manual_seed(0)
def portable(name, b, c, co, dg, h, w):
    x = torch.randn(b, c, h, w, device='cuda'); off = torch.randn(b, dg * 18, h, w, device='cuda') * 3
    msk = torch.rand(b, dg * 9, h, w, device='cuda'); gcol = torch.randn(b, c * 9, h * w, device='cuda')
    ws = (co, c, 3, 3)
    with hip.deterministic(False):
        def both():
            hip.dcn_im2col(x, off, msk, ws, 1, 1, 1, 1, dg)
            hip.dcn_col2im(gcol, x, off, msk, ws, 1, 1, 1, 1, dg)
        m, lo = timeit(both)
        m1, lo1 = timeit(lambda: hip.dcn_im2col(x, off, msk, ws, 1, 1, 1, 1, dg))
        m2, lo2 = timeit(lambda: hip.dcn_col2im(gcol, x, off, msk, ws, 1, 1, 1, 1, dg))
    print(f'{tag} portable im2col+col2im {name}: median {m:9.1f} us (min {lo:9.1f});  im2col {m1:8.1f} ({lo1:8.1f})  col2im {m2:8.1f} ({lo2:8.1f})', flush=True)
def fwd_portable(name, b, c, co, dg, h, w, groups, stride, pad, dil):
    x = torch.randn(b, c, h, w, device='cuda')
    ho, wo = E.out_size(h, w, stride, pad, dil)
    off = torch.randn(b, dg * 18, ho, wo, device='cuda') * 3; msk = torch.rand(b, dg * 9, ho, wo, device='cuda')
    wgt = torch.randn(co, c // groups, 3, 3, device='cuda') * 0.05; bias = torch.randn(co, device='cuda')
    m, lo = timeit(lambda: hip.dcn_fwd(x, off, msk, wgt, bias, stride, pad, dil, groups, dg, 0.1))
    print(f'{tag} portable forward {name}: median {m:9.1f} us (min {lo:9.1f})', flush=True)
def fused(name, b, c, dg, hw):
    x = torch.randn(b, hw, hw, c, device='cuda'); off = torch.randn(b, dg * 18, hw, hw, device='cuda') * 3
    msk = torch.rand(b, dg * 9, hw, hw, device='cuda'); g = torch.randn(b, hw, hw, c, device='cuda') * 1e-6
    wgt = torch.randn(c, c, 3, 3, device='cuda') * 0.02
    pk = hip.conv_pack_view(wgt, None, 16, dgrad='T', wscale=2.0 ** (13 - int(np.floor(np.log2(float(wgt.abs().max()))))))
    amax = g.abs().max().reshape(1)
    with hip.deterministic(False):
        m, lo = timeit(lambda: hip.dcn_bwd_data(g, x, off, msk, pk, dg, g_amax=amax), iters=20)
        m2, lo2 = timeit(lambda: hip.dcn_bwd_weight(g, x, off, msk, c, dg, g_amax=amax), iters=20)
    print(f'{tag} fused backward {name}: data median {m:9.1f} us (min {lo:9.1f})   weight median {m2:9.1f} us (min {lo2:9.1f})', flush=True)
portable('g8_dg4 2x8x13x21', 2, 8, 8, 4, 13, 21)
portable('64ch dg8 4x64x40x40', 4, 64, 64, 8, 40, 40)
if ITERS: sys.exit(0)
fwd_portable('g12_20_dg3_dil2 8x12x40x40', 8, 12, 20, 3, 40, 40, 1, 1, 2, 2)
fused('C=64 cpg8 B=4 160x160', 4, 64, 8, 160)
fused('C=128 cpg16 B=4 80x80', 4, 128, 8, 80)
fused('C=256 cpg32 B=4 40x40', 4, 256, 8, 40)
