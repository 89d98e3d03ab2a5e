#!/usr/bin/env python3
"""What the contextual loss costs.

  python tools/contextual_time.py [--steps 10] [--warmup 3] [--reps 10] [--batch 4] [--refs 5] [--lr 40] [--out FILE.json]

(1) the forward (six launches) and the backward (four launches) of csrc/contextual.hip for one tap at the relu3 / conv3 size of a
training step of --batch samples and LR --lr x --lr (C = 256, N = lr^2) and at the conv4_2 size (C = 512, N = (lr / 2)^2), on
correlated feature fields: HIP events around --reps back-to-back calls, divided by their number, the FLOPs of the all-pairs
products over that time, and the shader clock sampled while they run; for comparison the same tap as torch autograd of
losses.contextual_loss_torch on the GPU (forward and backward, fp32).  The per-kernel times come from running this file with
--no-step under a kernel trace;
(2) MultiRefRestorationModel.optimize_parameters at that size (16 residual blocks, synthetic weights): L1 alone and L1 with the
contextual loss on relu3_1 and conv4_2, two models in one process, steps alternating, ms per step (median of --steps after
--warmup)."""
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
import torch.nn.functional as F  # noqa: E402

TAPS = {'relu3_1': 1.0, 'conv4_2': 1.0}   # (relu2 taps of a 160 x 160 GT have 6400 positions: over hip.CX_MAX_N)


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


def _fields(b, c, h, w):
    g = torch.Generator().manual_seed(0)
    z = F.avg_pool2d(F.pad(torch.randn(b, 8, h + 1, w + 1, generator=g), (2, 2, 2, 2), mode='replicate'), 5, 1) * 5
    f = torch.einsum('ck,bkhw->bchw', torch.randn(c, 8, generator=g), z)
    return F.relu(f[:, :, 1:, 1:] + 0.1 * torch.randn(b, c, h, w, generator=g)).cuda().contiguous(), F.relu(f[:, :, :h, :w]).cuda().contiguous()


def _kernel_rows(b, lr, steps, warmup, reps):
    import bench
    from mrefsr_amd import hip
    from mrefsr_amd.losses import contextual_loss_torch
    rows = []
    up = torch.ones(1, device='cuda')
    with bench.ClockSampler(0) as clock:
        for c, side in ((256, lr), (512, lr // 2)):
            n = side * side
            x, y = _fields(b, c, side, side)
            xd, yd = x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous()
            _, saved = hip.contextual_fwd(xd, yd, 0.5)
            g = torch.empty_like(xd)
            flop = 2.0 * b * n * n * c
            for label, fn, fl in ((f'contextual_fwd C={c} N={n}', lambda: hip.contextual_fwd(xd, yd, 0.5), flop),
                                  (f'contextual_bwd C={c} N={n}', lambda: hip.contextual_bwd(saved, 0.5, 1.0, g, gup=up), 2 * flop)):
                ms = _median_ms(fn, steps, warmup, reps)
                rows.append(dict(launch=label, us=1e3 * ms, mflop=fl / 1e6, tflops=fl / ms / 1e9, CX=saved['cx'].tolist()))

            def torch_step():
                p = x.detach().requires_grad_(True)
                contextual_loss_torch(p, y, 0.5).backward()
            ms = _median_ms(torch_step, steps, warmup, max(1, reps // 4))
            rows.append(dict(launch=f'torch autograd of contextual_loss_torch C={c} N={n} (forward + backward)', us=1e3 * ms))
            with torch.no_grad():
                ms = _median_ms(lambda: contextual_loss_torch(x, y, 0.5), steps, warmup, max(1, reps // 4))
            rows.append(dict(launch=f'contextual_loss_torch C={c} N={n} (forward only)', us=1e3 * ms))
    return rows, clock.summary()


def _opt(contextual):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), net_g_pretrain_steps=0,
                 pixel_criterion='L1Loss', pixel_weight=1.0)
    if contextual:
        train['contextual_opt'] = dict(contextual)
    return dict(name='contextual_time', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, is_train=True, dist=False,
                network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8),
                network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                                 vgg_type='vgg19'),
                network_extractor=dict(type='ContrasMultiExtractorSep'), path={}, train=train)


def _step_times(b, k, lr, steps, warmup, taps):
    import bench
    import synth
    from mrefsr_amd.models import build_model
    models = {}
    for name, cx in (('l1', None), ('l1_contextual', dict(layer_weights=taps, band_width=0.5, loss_weight=0.1))):
        m = build_model(_opt(cx))
        nets = [m.get_bare_model(getattr(m, n)) for n in ('net_g', 'net_extractor', 'net_map')] + ([m.cri_contextual] if cx else [])
        for net in nets:
            spec = [(key, tuple(v.shape)) for key, v in net.state_dict().items()]
            net.load_state_dict({key: torch.from_numpy(v) for key, v in synth.state_dict(spec).items()})
        models[name] = m
    samples = [synth.sr_sample(f'contextual_time/s{i}', k, lr, lr) for i in range(b)]
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
    out['l_g_contextual'] = float(models['l1_contextual'].get_current_log()['l_g_contextual'])
    out['range_fallbacks'] = {n: m.range_fallbacks for n, m in models.items()}
    out['clock_mhz'] = clock.summary()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--refs', type=int, default=5)
    ap.add_argument('--lr', type=int, default=40)
    ap.add_argument('--no-step', action='store_true', help='the launches only')
    ap.add_argument('--out')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'contextual_time.py measures on a GPU'
    rows, clock = _kernel_rows(a.batch, a.lr, a.steps, a.warmup, a.reps)
    res = dict(batch=a.batch, refs=a.refs, lr=a.lr, launches=rows, launches_clock_mhz=clock)
    for r in rows:
        extra = f"  {r['mflop']:8.1f} MFLOP  {r['tflops']:5.2f} TFLOP/s" if 'tflops' in r else ''
        print(f"{r['launch']:84s} {r['us']:9.1f} us{extra}")
    print('shader clock while the launches ran:', json.dumps(clock))
    if not a.no_step:
        res['step'] = _step_times(a.batch, a.refs, a.lr, a.steps, a.warmup, TAPS)
        print(json.dumps(res['step']))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
