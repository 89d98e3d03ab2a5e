#!/usr/bin/env python3
"""What the MS-SSIM loss costs.

  python tools/msssim_loss_time.py [--steps 10] [--warmup 3] [--reps 20] [--batch 4] [--refs 5] [--lr 40] [--out FILE.json]

(1) the launches of csrc/msssim.hip at --batch samples, GT 160 x 160 with four levels and GT 256 x 256 with five, channel 'y' (and
'rgb' at 160): HIP events around --reps back-to-back calls, divided by their number (the launch-to-launch time on a busy stream,
with the host running ahead), and the shader clock sampled while they run; for comparison the same loss as torch autograd on the
GPU (losses.msssim_loss_torch, forward and backward, fp32) in the same session;
(2) MultiRefRestorationModel.optimize_parameters at LR --lr (16 residual blocks, synthetic weights): L1 alone and L1 with
train.msssim_opt, two models in one process, steps alternating, ms per step (median of --steps after --warmup).  Without the
option the step launches what it launched before the option existed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ssim_loss_time import _median_ms, _opt  # noqa: E402

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _kernel_rows(b, steps, warmup, reps):
    import bench
    from mrefsr_amd import hip
    from mrefsr_amd.losses import msssim_loss_torch
    up = torch.ones((), device='cuda')
    rows = []
    with bench.ClockSampler(0) as clock:
        for size, levels, channel in ((160, 4, 'y'), (160, 4, 'rgb'), (256, 5, 'y')):
            g = torch.Generator().manual_seed(0)
            target = torch.rand(b, 3, size, size, generator=g).cuda()
            pred = (0.5 * target + 0.5 * torch.rand(b, 3, size, size, generator=g).cuda()).contiguous()
            weights, rgb = WEIGHTS[:levels], channel == 'rgb'
            _, saved, _ = hip.msssim_loss_fwd(pred, target, weights, rgb, 1.0, want_grad=True)
            case = f'B={b} GT {size} M={levels} {channel}'
            for name, fn in ((f'msssim_loss_fwd {case} (loss only, 3 launches)', lambda: hip.msssim_loss_fwd(pred, target, weights, rgb, 1.0)),
                             (f'msssim_loss_fwd {case} (+ coefficient maps, 3 launches)',
                              lambda: hip.msssim_loss_fwd(pred, target, weights, rgb, 1.0, want_grad=True)),
                             (f'msssim_loss_bwd {case} (2 launches)', lambda: hip.msssim_loss_bwd(saved, up, pred.shape, rgb, 1.0))):
                rows.append(dict(launch=name, us=1e3 * _median_ms(fn, steps, warmup, reps)))

            def torch_fwd():
                with torch.no_grad():
                    msssim_loss_torch(pred, target, channel, weights)

            def torch_step():
                p = pred.detach().requires_grad_(True)
                msssim_loss_torch(p, target, channel, weights).backward()
            rows.append(dict(launch=f'torch {case} (forward, no grad)', us=1e3 * _median_ms(torch_fwd, steps, warmup, max(1, reps // 4))))
            rows.append(dict(launch=f'torch autograd {case} (forward + backward)', us=1e3 * _median_ms(torch_step, steps, warmup, max(1, reps // 4))))
    return rows, clock.summary()


def _step_times(b, k, lr, steps, warmup):
    import bench
    import synth
    from mrefsr_amd.models import build_model
    models = {}
    for name in ('l1', 'l1_msssim'):
        opt = _opt(False)
        if name == 'l1_msssim':
            opt['train']['msssim_opt'] = dict(loss_weight=0.1, channel='y', weights=list(WEIGHTS[:4]))
        m = build_model(opt)
        for net in (m.get_bare_model(getattr(m, n)) for n in ('net_g', 'net_extractor', 'net_map')):
            spec = [(key, tuple(v.shape)) for key, v in net.state_dict().items()]
            net.load_state_dict({key: torch.from_numpy(v) for key, v in synth.state_dict(spec).items()})
        models[name] = m
    samples = [synth.sr_sample(f'msssim_loss_time/s{i}', k, lr, lr) for i in range(b)]
    data = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    times = {n: [] for n in models}
    with bench.ClockSampler(0) as clock:
        for it in range(1, warmup + steps + 1):
            for name, m in models.items():   # (alternating: both see the same clock and the same neighbours)
                m.feed_data(data)
                torch.cuda.synchronize()
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                m.optimize_parameters(it)
                e.record()
                torch.cuda.synchronize()
                if it > warmup:
                    times[name].append(a.elapsed_time(e))
    out = {n: dict(ms=statistics.median(t), min_ms=min(t), max_ms=max(t)) for n, t in times.items()}
    out['l_g_msssim'] = float(models['l1_msssim'].get_current_log()['l_g_msssim'])
    out['range_fallbacks'] = {n: m.range_fallbacks for n, m in models.items()}
    out['clock_mhz'] = clock.summary()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--refs', type=int, default=5)
    ap.add_argument('--lr', type=int, default=40)
    ap.add_argument('--no-step', action='store_true', help='the launches only')
    ap.add_argument('--out')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'msssim_loss_time.py measures on a GPU'
    rows, clock = _kernel_rows(a.batch, a.steps, a.warmup, a.reps)
    res = dict(batch=a.batch, refs=a.refs, lr=a.lr, launches=rows, launches_clock_mhz=clock)
    for r in rows:
        print(f"{r['launch']:72s} {r['us']:8.1f} us")
    print('shader clock while the launches ran:', json.dumps(clock))
    if not a.no_step:
        res['step'] = _step_times(a.batch, a.refs, a.lr, a.steps, a.warmup)
        print(json.dumps(res['step']))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
