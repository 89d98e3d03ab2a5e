#!/usr/bin/env python3
"""What val.color_fix costs.

  python tools/color_fix_times.py [--steps 10] [--warmup 3] [--reps 20] [--out profiles/color_fix_times.txt]

Runs its parts one after the other, each in a process of its own under its own time limit, stops at the first one that fails, and
writes what they print to --out:
  kernels  hip.color_fix_wavelet (levels 5) and hip.color_fix_adain at B = 1, 500 x 500 with sizes (300, 500) -- a padded CUFED
           validation image -- and at B = 4, 160 x 160 and 640 x 640: the device time of each kernel from the profiler (median over
           --reps calls), HIP events around --reps back-to-back calls divided by their number (the launch-to-launch time on a busy
           stream), the shader clock sampled meanwhile; beside each the torch form of the same expression (color_fix.*_torch, fp32)
           on the same GPU, and a float4 copy of the same bytes (torch's copy of x, s and out: 12 bytes per element)
  test     MultiRefRestorationModel.test() at the CUFED validation size (B = 1, K = 5, LR 125 x 125) without the option and with
           each type: one model, the option switched between calls, the variants alternating, ms per call (median of --steps after
           --warmup); the run without the option is the baseline
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

PARTS = (('kernels', 300), ('test', 420))   # (name, time limit in seconds)


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
    from mrefsr_amd import color_fix as cf
    from mrefsr_amd import hip
    with bench.ClockSampler(0) as clock:
        for b, size, sizes in ((1, 500, [(300, 500)]), (4, 160, None), (4, 640, None)):
            g = torch.Generator().manual_seed(size)
            x = (torch.rand(b, 3, size, size, generator=g) * 1.2 - 0.1).cuda()
            s = torch.rand(b, 3, size, size, generator=g).cuda()
            out = torch.empty_like(x)
            print(f'B = {b}, {size} x {size} ({4.0 * x.numel() / 1e6:.2f} MB per tensor), sizes = {sizes}')
            for name, fn, ref in (('color_fix_wavelet', lambda: hip.color_fix_wavelet(x, s, sizes, levels=5),
                                   lambda: cf.wavelet_color_fix_torch(x, s, sizes, levels=5)),
                                  ('color_fix_adain', lambda: hip.color_fix_adain(x, s, sizes), lambda: cf.adain_color_fix_torch(x, s, sizes))):
                for kernel, us in _kernel_us(fn, a.reps).items():
                    print(f'  {name:18s} {kernel:48s} {us:8.2f} us device time per launch')
                print(f'  {name:18s} {"call to call, back to back":48s} {1e3 * _median_ms(fn, a.steps, a.warmup, a.reps):8.2f} us')
                n = len(_kernel_us(ref, 1))
                print(f'  {name:18s} {"the torch form of the same expression (fp32)":48s} '
                      f'{1e3 * _median_ms(ref, a.steps, a.warmup, max(1, a.reps // 4)):8.2f} us  ({n} distinct kernels)')

            def copies():   # the bytes of one call: x and s read, out written
                out.copy_(x)
                out.copy_(s)
            print(f'  {"float4 copy of the same bytes (two torch copies: 16 bytes per element)":67s} '
                  f'{1e3 * _median_ms(copies, a.steps, a.warmup, a.reps):8.2f} us')
    print('shader clock while the launches ran (MHz):', json.dumps(clock.summary()))


def part_test(a):
    import bench
    import torch
    from mrefsr_amd.color_fix import parse_color_fix
    args = argparse.Namespace(mode='infer')
    model = bench.build(args, False)
    bench.seeded_weights(model)
    model.feed_data(bench.synth_batch(1, 5, 125, seed=0))
    variants = {'without val.color_fix (baseline)': None, 'color_fix: wavelet': 'wavelet', 'color_fix: adain': 'adain'}
    times = {n: [] for n in variants}
    with bench.ClockSampler(0) as clock:
        for it in range(a.warmup + a.steps):
            for name, spec in variants.items():   # (alternating: all see the same clock and the same neighbours)
                model.opt['val'] = dict(color_fix=spec)
                model.color_fix_cfg = parse_color_fix(model.opt['val'])
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                model.test()
                e.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[name].append(s.elapsed_time(e))
    print('test() at B = 1, K = 5, LR 125 x 125 (output 500 x 500), ms per call:')
    for name, t in times.items():
        print(f'  {name:36s} median {statistics.median(t):7.2f}  min {min(t):7.2f}  max {max(t):7.2f}  ({len(t)} calls)')
    base = statistics.median(times['without val.color_fix (baseline)'])
    for name in list(variants)[1:]:
        print(f'  {name}: difference of the medians {statistics.median(times[name]) - base:+.3f} ms')
    print('  range fallbacks:', model.range_fallbacks)
    print('shader clock while the calls ran (MHz):', json.dumps(clock.summary()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'color_fix_times.txt'))
    ap.add_argument('--part', choices=[p for p, _ in PARTS], help='(internal) run one part in this process')
    a = ap.parse_args()
    if a.part:
        import torch
        assert torch.cuda.is_available(), 'color_fix_times.py measures on a GPU'
        torch.cuda.set_device(0)
        {'kernels': part_kernels, 'test': part_test}[a.part](a)
        return 0
    text = ['# tools/color_fix_times.py' + ''.join(f' --{k} {getattr(a, k)}' for k in ('steps', 'warmup', 'reps'))]
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
