#!/usr/bin/env python3
"""What the frequency-domain losses cost.

  python tools/freq_loss_time.py [--steps 10] [--warmup 3] [--reps 20] [--batch 4] [--refs 5] [--lr 40] [--out FILE.json]

(1) the forward (two launches for FFTLoss, three for FocalFrequencyLoss) and the backward (two launches) of csrc/freq_loss.hip at
the GT size of a training step of --batch samples and LR --lr x --lr (GT 4 lr): HIP events around --reps back-to-back calls,
divided by their number (the call-to-call time on a busy stream, with the host running ahead), the FLOPs of the dense transform
over that time, and the shader clock sampled while they run; for comparison the same definitions as torch autograd on the GPU
through torch.fft (rocFFT; losses.fft_loss_torch / focal_frequency_loss_torch, forward and backward, fp32).  The per-kernel times
come from running this file with --no-step under a kernel trace;
(2) MultiRefRestorationModel.optimize_parameters at that size (16 residual blocks, synthetic weights): L1 alone, L1 with FFTLoss
and L1 with FocalFrequencyLoss, three models in one process, steps alternating, ms per step (median of --steps after --warmup)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _median_ms(fn, steps, warmup, reps):
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


def _kernel_rows(b, lr, steps, warmup, reps):
    import bench
    from mrefsr_amd import hip
    from mrefsr_amd.losses import fft_loss_torch, focal_frequency_loss_torch
    h = w = 4 * lr
    wh, planes = w // 2 + 1, 3 * b
    g = torch.Generator().manual_seed(0)
    target = torch.rand(b, 3, h, w, generator=g).cuda()
    pred = (target + 0.05 * torch.randn(b, 3, h, w, generator=g).cuda()).contiguous()
    up = torch.ones((), device='cuda')
    fwd_flop = 2.0 * planes * h * w * 2 * wh + 8.0 * planes * h * h * wh      # real x complex rows, complex x complex columns
    bwd_flop = 8.0 * planes * h * h * wh + 4.0 * planes * h * w * wh
    rows = []
    with bench.ClockSampler(0) as clock:
        for name, kw, torch_fn in (('fft', dict(norm='backward'), lambda p: fft_loss_torch(p, target)),
                                   ('focal', dict(focal=True, alpha=1.0), lambda p: focal_frequency_loss_torch(p, target))):
            _, gmap = hip.freq_loss_fwd(pred, target, want_grad=True, **kw)
            for label, fn, flop in (
                    (f'freq_loss_fwd {name} (loss only)', lambda: hip.freq_loss_fwd(pred, target, **kw), fwd_flop),
                    (f'freq_loss_fwd {name} (+ gradient map)', lambda: hip.freq_loss_fwd(pred, target, want_grad=True, **kw), fwd_flop),
                    (f'freq_loss_bwd {name}', lambda: hip.freq_loss_bwd(gmap, up, pred.shape, 1.0), bwd_flop)):
                ms = _median_ms(fn, steps, warmup, reps)
                rows.append(dict(launch=label, us=1e3 * ms, mflop=flop / 1e6, tflops=flop / ms / 1e9))

            def torch_step():
                p = pred.detach().requires_grad_(True)
                torch_fn(p).backward()
            ms = _median_ms(torch_step, steps, warmup, max(1, reps // 4))
            rows.append(dict(launch=f'torch autograd through torch.fft {name} (forward + backward)', us=1e3 * ms))
            with torch.no_grad():
                ms = _median_ms(lambda: torch_fn(pred), steps, warmup, max(1, reps // 4))
            rows.append(dict(launch=f'torch.fft {name} (forward only)', us=1e3 * ms))
    return rows, clock.summary()


def _opt(freq):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), net_g_pretrain_steps=0,
                 pixel_criterion='L1Loss', pixel_weight=1.0)
    if freq:
        train['freq_opt'] = dict(freq)
    return dict(name='freq_loss_time', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, is_train=True, dist=False,
                network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8),
                network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                                 vgg_type='vgg19'),
                network_extractor=dict(type='ContrasMultiExtractorSep'), path={}, train=train)


def _step_times(b, k, lr, steps, warmup):
    import bench
    import synth
    from mrefsr_amd.models import build_model
    models = {}
    for name, freq in (('l1', None), ('l1_fft', dict(type='FFTLoss', loss_weight=0.05)),
                       ('l1_focal', dict(type='FocalFrequencyLoss', loss_weight=1.0))):
        m = build_model(_opt(freq))
        for net in (m.get_bare_model(getattr(m, n)) for n in ('net_g', 'net_extractor', 'net_map')):
            spec = [(key, tuple(v.shape)) for key, v in net.state_dict().items()]
            net.load_state_dict({key: torch.from_numpy(v) for key, v in synth.state_dict(spec).items()})
        models[name] = m
    samples = [synth.sr_sample(f'freq_loss_time/s{i}', k, lr, lr) for i in range(b)]
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
    out['l_g_freq'] = {n: float(m.get_current_log()['l_g_freq']) for n, m in models.items() if m.cri_freq is not None}
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
    assert torch.cuda.is_available(), 'freq_loss_time.py measures on a GPU'
    rows, clock = _kernel_rows(a.batch, a.lr, a.steps, a.warmup, a.reps)
    res = dict(batch=a.batch, refs=a.refs, lr=a.lr, launches=rows, launches_clock_mhz=clock)
    for r in rows:
        extra = f"  {r['mflop']:7.1f} MFLOP  {r['tflops']:5.2f} TFLOP/s" if 'tflops' in r else ''
        print(f"{r['launch']:64s} {r['us']:8.1f} us{extra}")
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
