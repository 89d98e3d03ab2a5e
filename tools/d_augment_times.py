#!/usr/bin/env python3
"""What the discriminator augmentation costs.

  python tools/d_augment_times.py [--steps 10] [--warmup 3] [--reps 20] [--out profiles/d_augment_times.txt]

Runs its parts one after the other, each in a process of its own under its own time limit, stops at the first one that fails, and
writes what they print to --out:
  kernels  the launches of csrc/disc_augment.hip at B = 4, 160 x 160 and 256 x 256 on one set of tables (policy color, translation,
           cutout, flip; p = 1): the device time of each kernel from the profiler (median over --reps calls), HIP events around
           --reps back-to-back calls divided by their number (the launch-to-launch time on a busy stream), the shader clock
           sampled meanwhile; d_augment_torch forward + backward under torch autograd on the same GPU and the same tables; the
           host time of one sampler call with its upload
  step     MultiRefRestorationModel.optimize_parameters at B = 4, K = 5, LR 40 x 40 with VGGStyleDiscriminator(160) and WGAN-GP,
           without and with d_augment {policy: [color, translation, cutout], p: 1}: two models in one process, steps alternating,
           ms per step (median of --steps after --warmup); the option-absent model is the baseline
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
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

PARTS = (('kernels', 300), ('step', 600))   # (name, time limit in seconds)


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
    from mrefsr_amd import hip
    from mrefsr_amd.archs import d_augment as da
    cfg = da.parse_d_augment(dict(policy=['color', 'translation', 'cutout', 'flip']))
    with bench.ClockSampler(0) as clock:
        for size in (160, 256):
            g = torch.Generator().manual_seed(size)
            x = torch.rand(4, 3, size, size, generator=g).cuda()
            gy = torch.randn(4, 3, size, size, generator=g).cuda()
            par = da.sample_d_augment(4, size, size, cfg, 1.0, g)
            pd = par.to('cuda')
            print(f'B = 4, {size} x {size} ({4.0 * x.numel() / 1e6:.2f} MB per tensor), contrast on: two launches per call')
            for name, fn in (('disc_augment', lambda: hip.disc_augment(x, pd)), ('disc_augment_adj', lambda: hip.disc_augment_adj(gy, pd))):
                for kernel, us in _kernel_us(fn, a.reps).items():
                    print(f'  {name:18s} {kernel:40s} {us:8.2f} us device time per launch')
                print(f'  {name:18s} {"call to call, back to back":40s} {1e3 * _median_ms(fn, a.steps, a.warmup, a.reps):8.2f} us')

            def pair():
                xx = x.detach().requires_grad_(True)
                da.d_augment(xx, pd).backward(gy)
            print(f'  {"HIP forward + backward through autograd":59s} {1e3 * _median_ms(pair, a.steps, a.warmup, a.reps):8.2f} us')

            def torch_pair():
                xx = x.detach().requires_grad_(True)
                da.d_augment_torch(xx, pd).backward(gy)
            n = len(_kernel_us(torch_pair, 1))
            print(f'  {"d_augment_torch forward + backward, torch autograd":59s} {1e3 * _median_ms(torch_pair, a.steps, a.warmup, max(1, a.reps // 4)):8.2f} us'
                  f'  ({n} distinct kernels)')
    import time
    g = torch.Generator().manual_seed(0)
    t0 = time.perf_counter()
    for _ in range(200):
        da.sample_d_augment(4, 160, 160, cfg, 1.0, g).to('cuda')
    torch.cuda.synchronize()
    print(f'sample_d_augment + upload, B = 4, host time per call: {(time.perf_counter() - t0) / 200 * 1e6:.1f} us')
    print('shader clock while the launches ran (MHz):', json.dumps(clock.summary()))


def part_step(a):
    import bench
    import gan_step_time as G
    import torch
    G.GAN['plain'] = dict(G.GAN['wgan_gp'])
    G.GAN['augmented'] = dict(G.GAN['wgan_gp'], d_augment=dict(policy=['color', 'translation', 'cutout'], p=1.0))
    models = {name: G._model(name, 'VGGStyleDiscriminator', 40) for name in ('plain', 'augmented')}
    times = {n: [] for n in models}
    with bench.ClockSampler(0) as clock:
        for it in range(1, a.warmup + a.steps + 1):
            for name, m in models.items():   # (alternating: both see the same clock and the same neighbours)
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                m.optimize_parameters(it)
                e.record()
                torch.cuda.synchronize()
                if it > a.warmup:
                    times[name].append(s.elapsed_time(e))
    print('B = 4, K = 5, LR 40 x 40, VGGStyleDiscriminator(160), WGAN-GP (gan_weight 1e-3, grad_penalty_weight 10), ms per step:')
    for name, t in times.items():
        what = 'without train.d_augment (baseline)' if name == 'plain' else 'd_augment {policy: [color, translation, cutout], p: 1}'
        print(f'  {what:58s} median {statistics.median(t):7.2f}  min {min(t):7.2f}  max {max(t):7.2f}  ({len(t)} steps)')
    print(f'  difference of the medians: {statistics.median(times["augmented"]) - statistics.median(times["plain"]):+.2f} ms')
    print('  range fallbacks:', json.dumps({n: m.range_fallbacks for n, m in models.items()}))
    print('shader clock while the steps ran (MHz):', json.dumps(clock.summary()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'd_augment_times.txt'))
    ap.add_argument('--part', choices=[p for p, _ in PARTS], help='(internal) run one part in this process')
    a = ap.parse_args()
    if a.part:
        import torch
        assert torch.cuda.is_available(), 'd_augment_times.py measures on a GPU'
        torch.cuda.set_device(0)
        {'kernels': part_kernels, 'step': part_step}[a.part](a)
        return 0
    text = ['# tools/d_augment_times.py' + ''.join(f' --{k} {getattr(a, k)}' for k in ('steps', 'warmup', 'reps'))]
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
