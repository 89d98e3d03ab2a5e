#!/usr/bin/env python3
"""Times of the degradation kernels (csrc/degrade.hip) and of the whole chain against the same chain built from the *_torch
operators on the same GPU (mrefsr_amd/degradation.py).

    python tools/degrade_time.py [--batch 4] [--gt 160] [--iters 30] [--step] [--json out.json]

Per operator: the median of `iters` calls between HIP events, after warm-up, kernel and torch form on the same tensors.  The chain:
HighOrderDegradation.apply / apply_torch with one fixed plan per noise model (Gaussian in both stages, Poisson in both), host time
per call with a synchronise behind it (that is what a training step waits for), and the launches per call counted by the profiler.
--step: feed_data + optimize_parameters of the 16-block model at K = 5 without and with the option, two models alternating."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def wall_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t))
    return statistics.median(times)


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type is not None and 'cuda' in str(e.device_type).lower())


def step_times(b, k, lr, steps, warmup):
    """feed_data + optimize_parameters (16 residual blocks, L1, synthetic weights) without and with `degradation`, two models in one
    process, steps alternating; host time per step with a synchronise behind it, and feed_data's share of it"""
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden'))
    import synth
    from mrefsr_amd.models import build_model

    def opt(deg):
        train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                     scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), net_g_pretrain_steps=0,
                     pixel_criterion='L1Loss', pixel_weight=1.0)
        o = dict(name='degrade_time', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, is_train=True, dist=False,
                 manual_seed=0, network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8),
                 network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1,
                                  vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'], vgg_type='vgg19'),
                 network_extractor=dict(type='ContrasMultiExtractorSep'), path={}, train=train)
        if deg:
            o['degradation'] = {}
        return o
    models = {}
    for name, deg in (('plain', False), ('degradation', True)):
        m = build_model(opt(deg))
        for net in (m.get_bare_model(getattr(m, n)) for n in ('net_g', 'net_extractor', 'net_map')):
            spec = [(key, tuple(v.shape)) for key, v in net.state_dict().items()]
            net.load_state_dict({key: torch.from_numpy(v) for key, v in synth.state_dict(spec).items()})
        models[name] = m
    samples = [synth.sr_sample(f'degrade_time/s{i}', k, lr, lr) for i in range(b)]
    data = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    total, feed = {n: [] for n in models}, {n: [] for n in models}
    for it in range(1, warmup + steps + 1):
        for name, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.feed_data(data)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            m.optimize_parameters(it)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if it > warmup:
                total[name].append(1e3 * (t2 - t0))
                feed[name].append(1e3 * (t1 - t0))
    return {n: dict(step_ms=statistics.median(total[n]), feed_data_ms=statistics.median(feed[n]), range_fallbacks=models[n].range_fallbacks)
            for n in models}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', action='store_true', help='also: the training step at B = batch, K = 5, LR = gt / 4 without and with the option')
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--gt', type=int, default=160)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--json')
    args = ap.parse_args()
    from mrefsr_amd import degradation as D, hip
    b, s = args.batch, args.gt
    g = torch.Generator(device='cuda').manual_seed(0)
    img = torch.rand(b, 3, s, s, device='cuda', generator=g)
    kern = torch.rand(b, 21, 21, device='cuda', generator=g)
    kern = kern / kern.sum(dim=(1, 2), keepdim=True)
    q = torch.full((b,), 60.0, device='cuda')
    n, ng = torch.randn(b, 3, s, s, device='cuda', generator=g), torch.randn(b, 1, s, s, device='cuda', generator=g)
    sigma, gray = torch.full((b,), 10.0, device='cuda'), (torch.arange(b, device='cuda') % 2).float()
    vals = hip.degrade_levels(img)
    out = {'batch': b, 'gt': s, 'ops_ms': {}, 'chain': {}}
    ops = {
        'filter2d k=21': (lambda: hip.degrade_filter2d(img, kern), lambda: D.filter2d_torch(img, kern)),
        'usm radius 51': (lambda: hip.degrade_usm(img), lambda: D.usm_sharp_torch(img)),
        'resize bicubic x0.5': (lambda: hip.degrade_resize(img, scale_factor=0.5, mode='bicubic'),
                                lambda: D.resize_torch(img, scale_factor=0.5, mode='bicubic')),
        'resize area x0.5': (lambda: hip.degrade_resize(img, scale_factor=0.5, mode='area'), lambda: D.resize_torch(img, scale_factor=0.5, mode='area')),
        'noise gaussian': (lambda: hip.degrade_noise(img, n, ng, sigma, gray), lambda: D.noise_torch(img, n, ng, sigma, gray)),
        'noise poisson': (lambda: hip.degrade_noise(img, n.abs(), ng.abs(), sigma, gray, vals, poisson=True),
                          lambda: D.noise_torch(img, n.abs(), ng.abs(), sigma, gray, vals, poisson=True)),
        'levels': (lambda: hip.degrade_levels(img), lambda: D.levels_torch(img)),
        'jpeg': (lambda: hip.degrade_jpeg(img, q), lambda: D.jpeg_torch(img, q)),
    }
    for name, (kernel, torch_form) in ops.items():
        out['ops_ms'][name] = {'hip': event_ms(kernel, args.iters), 'torch': event_ms(torch_form, args.iters)}
        print(f"{name:22s} hip {out['ops_ms'][name]['hip'] * 1e3:8.1f} us   torch {out['ops_ms'][name]['torch'] * 1e3:8.1f} us", flush=True)
    for label, prob in (('gaussian', 1.0), ('poisson', 0.0)):
        deg = D.HighOrderDegradation(dict(gaussian_noise_prob=prob, gaussian_noise_prob2=prob, resize_range=[0.3, 1.5]))
        plan = deg.sample(b, (s, s), 3)
        gen = torch.Generator(device='cuda').manual_seed(1)
        row = {'hip_ms': wall_ms(lambda: deg.apply(img, plan, gen), args.iters), 'torch_ms': wall_ms(lambda: deg.apply_torch(img, plan, gen), args.iters)}
        try:
            row['hip_launches'], row['torch_launches'] = launches(lambda: deg.apply(img, plan, gen)), launches(lambda: deg.apply_torch(img, plan, gen))
        except Exception as e:   # the profiler is optional equipment
            row['launches_error'] = repr(e)
        row['sample_ms'] = statistics.median([(lambda t: (deg.sample(b, (s, s), 5), 1e3 * (time.perf_counter() - t))[1])(time.perf_counter())
                                              for _ in range(10)])
        out['chain'][label] = row
        print(label, row, flush=True)
    if args.step:
        out['step'] = step_times(b, 5, s // 4, 20, 5)
        print('step', out['step'], flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
