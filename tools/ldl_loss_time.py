#!/usr/bin/env python3
"""What the LDL artifact loss costs.

  python tools/ldl_loss_time.py [--steps 10] [--warmup 3] [--reps 20] [--batch 4] [--refs 5] [--lr 40] [--out FILE.json]

(1) the launches of csrc/ldl_loss.hip at the GT size of a training step of --batch samples and LR --lr x --lr (GT 4 lr): HIP events
around --reps back-to-back launches, divided by their number (at 1.8 MB of input a launch is a few microseconds: this is the
launch-to-launch time on a busy stream, with the host running ahead), the bytes each must move over that time, and the shader
clock sampled while they run; for comparison the same criterion as torch autograd on the GPU (losses.ldl_loss_torch: unfold, forward
and backward, fp32);
(2) MultiRefRestorationModel.optimize_parameters at that size (16 residual blocks, synthetic weights, ema_decay 0.999): L1 alone and
L1 with train.ldl_opt, two models in one process, steps alternating, ms per step (median of --steps after --warmup); inside the
second model's steps, HIP events around the EMA pass (net_g_ema without a graph, its weights re-packed: the EMA update moved them)
and the number of weight packings that pass makes per step; afterwards the same pass with every packed copy current."""
import argparse
import ctypes
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
    from mrefsr_amd.losses import ldl_loss_torch
    h = w = 4 * lr
    g = torch.Generator().manual_seed(0)
    target = torch.rand(b, 3, h, w, generator=g).cuda()
    pred = (target + 0.1 * torch.randn(b, 3, h, w, generator=g).cuda()).contiguous()
    ema = (target + 0.1 * torch.randn(b, 3, h, w, generator=g).cuda()).contiguous()
    up = torch.ones((), device='cuda')
    rows = []
    img_b, map_b = 4.0 * pred.numel(), 4.0 * b * h * w
    with bench.ClockSampler(0) as clock:
        _, saved, _ = hip.ldl_loss_fwd(pred, target, ema, 1.0, want_grad=True)
        for name, fn, nbytes in (
                ('ldl_loss_fwd (loss only)', lambda: hip.ldl_loss_fwd(pred, target, ema, 1.0), 3 * img_b),
                ('ldl_loss_fwd (+ the three maps)', lambda: hip.ldl_loss_fwd(pred, target, ema, 1.0, want_grad=True), 3 * img_b + 3 * map_b),
                ('ldl_loss_bwd', lambda: hip.ldl_loss_bwd(pred, target, saved, up, 1.0), 3 * img_b + 3 * map_b),
                ('ldl_loss_fwd + ldl_loss_map (artifact_map)', lambda: hip.ldl_loss_fwd(pred, target, ema, 1.0, want_map=True), 3 * img_b + 3 * map_b)):
            ms = _median_ms(fn, steps, warmup, reps)
            rows.append(dict(launch=name, us=1e3 * ms, mbytes=nbytes / 1e6, tb_per_s=nbytes / ms / 1e9))

        # the kernels alone: the C entry points on preallocated outputs (the wrappers above allocate two to five tensors per call,
        # which at this size is most of a call's time: the host is the slower side)
        from mrefsr_amd import _lib
        grad, loss = torch.empty_like(pred), torch.empty((), device='cuda')
        part, ticket = hip._det_scratch(pred.device, 16 * _lib.load().mrefsr_ldl_loss_blocks(b, h, w))
        mr, mu, vm, stats = saved
        ptr, lw, st = hip._p, ctypes.c_float(1.0), hip._stream()
        for name, fn, nbytes in (
                ('mrefsr_ldl_loss_fwd_f32 alone (+ the three maps)',
                 lambda: _lib.call('mrefsr_ldl_loss_fwd_f32', ptr(pred), ptr(target), ptr(ema), b, h, w, lw, ptr(mr), ptr(mu), ptr(vm), ptr(stats),
                                   ptr(part), ptr(ticket), ptr(loss), st), 3 * img_b + 3 * map_b),
                ('mrefsr_ldl_loss_bwd_f32 alone',
                 lambda: _lib.call('mrefsr_ldl_loss_bwd_f32', ptr(pred), ptr(target), ptr(mr), ptr(mu), ptr(vm), ptr(stats), ptr(up), b, h, w, lw,
                                   ptr(grad), st), 3 * img_b + 3 * map_b)):
            ms = _median_ms(fn, steps, warmup, reps)
            rows.append(dict(launch=name, us=1e3 * ms, mbytes=nbytes / 1e6, tb_per_s=nbytes / ms / 1e9))

        def torch_step():
            p = pred.detach().requires_grad_(True)
            ldl_loss_torch(p, target, ema).backward()
        ms = _median_ms(torch_step, steps, warmup, max(1, reps // 4))
        rows.append(dict(launch='torch autograd of ldl_loss_torch (forward + backward)', us=1e3 * ms))
    return rows, clock.summary()


def _opt(ldl):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), net_g_pretrain_steps=0,
                 pixel_criterion='L1Loss', pixel_weight=1.0, ema_decay=0.999)
    if ldl:
        train['ldl_opt'] = dict(type='L1Loss', loss_weight=1.0, reduction='mean')
    return dict(name='ldl_loss_time', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, is_train=True, dist=False,
                network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8),
                network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                                 vgg_type='vgg19'),
                network_extractor=dict(type='ContrasMultiExtractorSep'), path={}, train=train)


def _step_times(b, k, lr, steps, warmup):
    import bench
    import synth
    from mrefsr_amd import hip
    from mrefsr_amd.models import build_model
    models = {}
    for name, ldl in (('l1_ema', False), ('l1_ema_ldl', True)):
        m = build_model(_opt(ldl))
        for net in (m.get_bare_model(getattr(m, n)) for n in ('net_g', 'net_extractor', 'net_map')):
            spec = [(key, tuple(v.shape)) for key, v in net.state_dict().items()]
            net.load_state_dict({key: torch.from_numpy(v) for key, v in synth.state_dict(spec).items()})
        m.model_ema(0)
        models[name] = m
    # events around the EMA pass of the second model, and its weight packings
    ldl, pass_events, packings = models['l1_ema_ldl'], [], [0]
    ema_pass, pack = ldl._ema_pass, hip.conv_pack_weight
    in_pass = [False]

    def timed_pass():
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        in_pass[0] = True
        try:
            out = ema_pass()
        finally:
            in_pass[0] = False
        e.record()
        pass_events.append((a, e))
        return out

    def counted_pack(*args, **kw):
        packings[0] += in_pass[0]
        return pack(*args, **kw)
    ldl._ema_pass, hip.conv_pack_weight = timed_pass, counted_pack
    samples = [synth.sr_sample(f'ldl_loss_time/s{i}', k, lr, lr) for i in range(b)]
    data = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    times = {n: [] for n in models}
    try:
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
        # the pass alone: a second call finds every packed copy current (the first one re-packs behind the last step's EMA update)
        hip.amax_pool_reset()
        ema_pass()
        alone = _median_ms(lambda: (hip.amax_pool_reset(), ema_pass()), steps, 1, 1)
    finally:
        hip.conv_pack_weight = pack
    out = {n: dict(ms=statistics.median(t), min_ms=min(t), max_ms=max(t)) for n, t in times.items()}
    passes = [a.elapsed_time(e) for a, e in pass_events[warmup:]]
    out['ema_pass_ms'] = dict(ms=statistics.median(passes), min_ms=min(passes), max_ms=max(passes))
    out['ema_pass_weight_packings_per_step'] = packings[0] / len(pass_events)
    out['ema_pass_current_weights_ms'] = alone
    out['l_g_ldl'] = float(ldl.get_current_log()['l_g_ldl'])
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
    assert torch.cuda.is_available(), 'ldl_loss_time.py measures on a GPU'
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
