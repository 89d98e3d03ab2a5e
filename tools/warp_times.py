#!/usr/bin/env python3
"""What the homography views cost: hip.warp_perspective, train.ref_augment and val.match_probe.

  python tools/warp_times.py [--steps 10] [--warmup 3] [--reps 20] [--out profiles/warp_times.txt]

Runs its parts one after the other, each in a process of its own under its own time limit, stops at the first one that fails, and
writes what they print to --out:
  kernels  hip.warp_perspective (bicubic and bilinear, clamp on) under random corner homographies at the training shape N = 20
           (B = 4, K = 5), 3 x 160 x 160 and at the validation shape N = 5, 3 x 500 x 500: the device time of the kernel from the
           profiler (median over --reps calls), HIP events around --reps back-to-back calls divided by their number, the shader
           clock sampled meanwhile; beside each torch.nn.functional.grid_sample in fp32 on the same GPU (mode bicubic / bilinear,
           zeros padding, align_corners; the grid made once, outside the timed region), the two alternating in one session
  step     feed_data + optimize_parameters at B = 4, K = 5, LR 40 x 40 (L1) without train.ref_augment and with {p: 1}: one model,
           the option switched between steps, the variants alternating, ms per step (median of --steps after --warmup)
  test     feed_data + test() [+ the probe] at the CUFED validation size (B = 1, K = 5, LR 125 x 125) without val.match_probe and
           with it, alternating likewise; the probe's statistics stay on the device, as in validation
No bar is set for any of these times: the file reports what was measured."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

PARTS = (('kernels', 300), ('step', 420), ('test', 420))   # (name, time limit in seconds)


def _median_ms(fn, steps, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return statistics.median(ts)


def _kernel_us(fn, reps):
    """{kernel name: median device time in us} over reps profiled calls"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    times = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            m = re.search(r'(\w+_kernel(<[^>]*>)?)', e.name)
            times.setdefault(m.group(1) if m else e.name[:40], []).append(e.device_time)
    return {k: statistics.median(v) for k, v in times.items()}


def part_kernels(a):
    import bench
    import torch
    import torch.nn.functional as F
    from mrefsr_amd import hip, views
    with bench.ClockSampler(0) as clock:
        for n, size in ((20, 160), (5, 500)):
            g = torch.Generator().manual_seed(size)
            x = torch.rand(n, 3, size, size, generator=g).cuda()
            s = views.sample_corner_homographies(n, size, size, [5, 20], generator=g)
            sd = s.reshape(n, 9).cuda()
            ys, xs = torch.meshgrid(torch.arange(size, dtype=torch.float64), torch.arange(size, dtype=torch.float64), indexing='ij')
            q = torch.einsum('nij,hwj->nhwi', s, torch.stack([xs, ys, torch.ones_like(xs)], dim=-1))
            grid = (2 * q[..., :2] / q[..., 2:] / (size - 1) - 1).float().cuda()
            print(f'N = {n}, 3 x {size} x {size} ({4.0 * x.numel() / 1e6:.2f} MB in, as much out)')
            for interp in ('bicubic', 'bilinear'):
                def fn():
                    return hip.warp_perspective(x, sd, interp=interp, clamp=True)

                def ref():
                    return F.grid_sample(x, grid, mode=interp, padding_mode='zeros', align_corners=True).clamp_(0, 1)
                for _ in range(2):   # (alternating)
                    for kernel, us in _kernel_us(fn, a.reps).items():
                        print(f'  {interp:9s} {kernel:52s} {us:8.2f} us device time per launch')
                    print(f'  {interp:9s} {"hip.warp_perspective, call to call, back to back":52s} {1e3 * _median_ms(fn, a.steps, a.warmup, a.reps):8.2f} us')
                    for kernel, us in _kernel_us(ref, a.reps).items():
                        print(f'  {interp:9s} torch: {kernel[:45]:45s} {us:8.2f} us device time per launch')
                    print(f'  {interp:9s} {"grid_sample + clamp_ (fp32), call to call":52s} {1e3 * _median_ms(ref, a.steps, a.warmup, a.reps):8.2f} us')
    print('shader clock while the launches ran (MHz):', json.dumps(clock.summary()))


def _alternate(a, variants, switch, body, what):
    import bench
    import torch
    times = {n: [] for n in variants}
    with bench.ClockSampler(0) as clock:
        for it in range(1, a.warmup + a.steps + 1):
            for name, spec in variants.items():   # (alternating: all see the same clock and the same neighbours)
                switch(spec)
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                body(it)
                e.record()
                torch.cuda.synchronize()
                if it > a.warmup:
                    times[name].append(s.elapsed_time(e))
    print(what)
    names = list(variants)
    for name, t in times.items():
        print(f'  {name:44s} median {statistics.median(t):7.2f}  min {min(t):7.2f}  max {max(t):7.2f}  ({len(t)} calls)')
    for name in names[1:]:
        print(f'  {name}: difference of the medians {statistics.median(times[name]) - statistics.median(times[names[0]]):+.3f} ms')
    print('shader clock meanwhile (MHz):', json.dumps(clock.summary()))


def part_step(a):
    import bench
    model = bench.build(argparse.Namespace(mode='train'), False)
    bench.seeded_weights(model)
    data = bench.synth_batch(4, 5, 40, seed=0)

    def switch(spec):
        model.opt['train']['ref_augment'] = spec
        model._setup_ref_views(model.opt)

    def body(it):
        model.feed_data(data)
        model.optimize_parameters(it)
    _alternate(a, {'without train.ref_augment (baseline)': None, 'ref_augment {p: 1, perturb: [5, 20]}': dict(p=1)}, switch, body,
               'feed_data + optimize_parameters at B = 4, K = 5, LR 40 x 40 (references 20 x 3 x 160 x 160), L1, ms per step:')
    print('  range fallbacks:', model.range_fallbacks)


def part_test(a):
    import bench
    model = bench.build(argparse.Namespace(mode='infer'), False)
    bench.seeded_weights(model)
    data = bench.synth_batch(1, 5, 125, seed=0)

    def switch(spec):
        model.opt['val'] = dict(match_probe=spec)
        model._setup_ref_views(model.opt)

    def body(it):
        model.feed_data(data)
        model.test()
        if model.match_probe_cfg is not None:
            model._match_probe_stats(model.match_probe_cfg)
    _alternate(a, {'without val.match_probe (baseline)': None, 'match_probe: true': True}, switch, body,
               'feed_data + test() [+ probe] at B = 1, K = 5, LR 125 x 125 (output 500 x 500), ms per image:')
    print('  range fallbacks:', model.range_fallbacks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'warp_times.txt'))
    ap.add_argument('--part', choices=[p for p, _ in PARTS], help='(internal) run one part in this process')
    a = ap.parse_args()
    if a.part:
        import torch
        assert torch.cuda.is_available(), 'warp_times.py measures on a GPU'
        torch.cuda.set_device(0)
        {'kernels': part_kernels, 'step': part_step, 'test': part_test}[a.part](a)
        return 0
    text = ['# tools/warp_times.py' + ''.join(f' --{k} {getattr(a, k)}' for k in ('steps', 'warmup', 'reps'))]
    rc = 0
    for part, limit in PARTS:
        cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--steps', str(a.steps), '--warmup', str(a.warmup), '--reps', str(a.reps)]
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            rc, out, err = run.returncode, run.stdout, run.stderr
        except subprocess.TimeoutExpired as e:
            rc, out, err = 124, e.stdout or '', f'time limit of {limit} s reached'
            out = out.decode() if isinstance(out, bytes) else out
        text += [f'\n## {part}', out.rstrip()]
        print(text[-2], text[-1], sep='\n', flush=True)
        if rc != 0:
            text.append(f'FAILED with exit status {rc}; the parts behind it were not run\n{str(err)[-2000:]}')
            print(text[-1], flush=True)
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(text) + '\n')
    return rc


if __name__ == '__main__':
    sys.exit(main())
