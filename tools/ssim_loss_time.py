#!/usr/bin/env python3
"""What the SSIM loss costs.

  python tools/ssim_loss_time.py [--steps 10] [--warmup 3] [--reps 20] [--batch 4] [--refs 5] [--lr 40] [--out FILE.json]

(1) the two launches of csrc/ssim_loss.hip at the GT size of a training step of --batch samples and LR --lr x --lr (GT 4 lr), both
channel modes: HIP events around --reps back-to-back launches, divided by their number (at 1.2 MB of input a launch is a few
microseconds: this is the launch-to-launch time on a busy stream, with the host running ahead), the bytes each must move over
that time, and the shader clock sampled while they run; for comparison the same loss as torch autograd on the GPU through F.conv2d
(losses.ssim_loss_torch, forward and backward, fp32);
(2) MultiRefRestorationModel.optimize_parameters at that size (16 residual blocks, synthetic weights): L1 alone and L1 with
train.ssim_opt, two models in one process, steps alternating, ms per step (median of --steps after --warmup)."""
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
    from mrefsr_amd.losses import ssim_loss_torch
    h = w = 4 * lr
    g = torch.Generator().manual_seed(0)
    target = torch.rand(b, 3, h, w, generator=g).cuda()
    pred = (target + 0.05 * torch.randn(b, 3, h, w, generator=g).cuda()).contiguous()
    up = torch.ones((), device='cuda')
    rows = []
    with bench.ClockSampler(0) as clock:
        for channel in ('y', 'rgb'):
            rgb = channel == 'rgb'
            planes = (3 if rgb else 1) * b
            img_b, map_b = 4.0 * pred.numel(), 4.0 * planes * (h - 10) * (w - 10)
            _, maps = hip.ssim_loss_fwd(pred, target, rgb, 1.0, want_grad=True)
            for name, fn, nbytes in (
                    (f'ssim_loss_fwd {channel} (loss only)', lambda: hip.ssim_loss_fwd(pred, target, rgb, 1.0), 2 * img_b),
                    (f'ssim_loss_fwd {channel} (+ coefficient maps)', lambda: hip.ssim_loss_fwd(pred, target, rgb, 1.0, want_grad=True), 2 * img_b + 3 * map_b),
                    (f'ssim_loss_bwd {channel}', lambda: hip.ssim_loss_bwd(pred, target, maps, up, rgb, 1.0), 3 * img_b + 3 * map_b)):
                ms = _median_ms(fn, steps, warmup, reps)
                rows.append(dict(launch=name, us=1e3 * ms, mbytes=nbytes / 1e6, tb_per_s=nbytes / ms / 1e9))

            def torch_step():
                p = pred.detach().requires_grad_(True)
                ssim_loss_torch(p, target, channel).backward()
            ms = _median_ms(torch_step, steps, warmup, max(1, reps // 4))
            rows.append(dict(launch=f'torch autograd through F.conv2d {channel} (forward + backward)', us=1e3 * ms))
    return rows, clock.summary()


def _opt(ssim):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), net_g_pretrain_steps=0,
                 pixel_criterion='L1Loss', pixel_weight=1.0)
    if ssim:
        train['ssim_opt'] = dict(loss_weight=0.1, channel='y')
    return dict(name='ssim_loss_time', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, is_train=True, dist=False,
                network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8),
                network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                                 vgg_type='vgg19'),
                network_extractor=dict(type='ContrasMultiExtractorSep'), path={}, train=train)


def _step_times(b, k, lr, steps, warmup):
    import bench
    import synth
    from mrefsr_amd.models import build_model
    models = {}
    for name, ssim in (('l1', False), ('l1_ssim', True)):
        m = build_model(_opt(ssim))
        for net in (m.get_bare_model(getattr(m, n)) for n in ('net_g', 'net_extractor', 'net_map')):
            spec = [(key, tuple(v.shape)) for key, v in net.state_dict().items()]
            net.load_state_dict({key: torch.from_numpy(v) for key, v in synth.state_dict(spec).items()})
        models[name] = m
    samples = [synth.sr_sample(f'ssim_loss_time/s{i}', k, lr, lr) for i in range(b)]
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
    out['l_g_ssim'] = float(models['l1_ssim'].get_current_log()['l_g_ssim'])
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
    assert torch.cuda.is_available(), 'ssim_loss_time.py measures on a GPU'
    rows, clock = _kernel_rows(a.batch, a.lr, a.steps, a.warmup, a.reps)
    res = dict(batch=a.batch, refs=a.refs, lr=a.lr, launches=rows, launches_clock_mhz=clock)
    for r in rows:
        extra = f"  {r['mbytes']:6.2f} MB  {r['tb_per_s']:5.2f} TB/s" if 'tb_per_s' in r else ''
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
