#!/usr/bin/env python3
"""What the contextual loss costs.

  python tools/contextual_time.py [--steps 10] [--warmup 3] [--reps 10] [--batch 4] [--refs 5] [--lr 40] [--out FILE.json]
                                  [--weight-sp WS] [--rgb-patch SIZE,STRIDE] [--tap-stride LAYER=S[,LAYER=S]]

(1) the forward (six launches) and the backward (four launches) of csrc/contextual.hip for one tap at the relu3 / conv3 size of a
training step of --batch samples and LR --lr x --lr (C = 256, N = lr^2) and at the conv4_2 size (C = 512, N = (lr / 2)^2), on
correlated feature fields: HIP events around --reps back-to-back calls, divided by their number, the FLOPs of the all-pairs
products over that time, and the shader clock sampled while they run; for comparison the same tap as torch autograd of
losses.contextual_loss_torch on the GPU (forward and backward, fp32).  The per-kernel times come from running this file with
--no-step under a kernel trace;
(2) MultiRefRestorationModel.optimize_parameters at that size (16 residual blocks, synthetic weights): L1 alone and L1 with the
contextual loss on relu3_1 and conv4_2, two models in one process, steps alternating, ms per step (median of --steps after
--warmup).
The CoBi options (the rows above stay as they are: weight_sp = 0 on the plain kernels): --weight-sp adds the two taps with the
spatial term in cx_dist's epilogue; --rgb-patch the RGB tap of the GT-sized images (hip.cx_patches of the 2 B images, the tap,
hip.cx_patches_bwd); --tap-stride, per named layer, the tap at its stride (hip.cx_subsample of the 2 B maps, the tap,
hip.cx_subsample_bwd).  With any of them the step of (2) takes all of them in its contextual_opt, the strided layers as taps too."""
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


def _layer_geometry(name, lr):
    """(channels, side) of a VGG19 tap of a GT of 4 lr x 4 lr"""
    block = int(name[4])
    return (64, 128, 256, 512, 512)[block - 1], (4 * lr) >> (block - 1)


def _tap_rows(rows, label, xd, yd, ws, steps, warmup, reps):
    """the forward and the backward of one tap [B,h,w,C] at weight_sp = ws"""
    from mrefsr_amd import hip
    b, h, w, c = xd.shape
    n = h * w
    up = torch.ones(1, device='cuda')
    _, saved = hip.contextual_fwd(xd, yd, 0.5, weight_sp=ws)
    g = torch.empty_like(xd)
    flop = 2.0 * b * n * n * c
    for name, fn, fl in ((f'contextual_fwd {label}', lambda: hip.contextual_fwd(xd, yd, 0.5, weight_sp=ws), flop),
                         (f'contextual_bwd {label}', lambda: hip.contextual_bwd(saved, 0.5, 1.0, g, gup=up, weight_sp=ws), 2 * flop)):
        ms = _median_ms(fn, steps, warmup, reps)
        rows.append(dict(launch=name, us=1e3 * ms, mflop=fl / 1e6, tflops=fl / ms / 1e9, CX=saved['cx'].tolist()))


def _kernel_rows(b, lr, steps, warmup, reps, weight_sp=0.0, rgb_patch=None, tap_stride=None):
    import bench
    from mrefsr_amd import hip
    from mrefsr_amd.losses import contextual_loss_torch
    rows = []
    with bench.ClockSampler(0) as clock:
        for c, side in ((256, lr), (512, lr // 2)):
            n = side * side
            x, y = _fields(b, c, side, side)
            xd, yd = x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous()
            _tap_rows(rows, f'C={c} N={n}', xd, yd, 0.0, steps, warmup, reps)
            if weight_sp > 0:
                _tap_rows(rows, f'C={c} N={n} weight_sp={weight_sp}', xd, yd, weight_sp, steps, warmup, reps)

            def torch_step():
                p = x.detach().requires_grad_(True)
                contextual_loss_torch(p, y, 0.5).backward()
            ms = _median_ms(torch_step, steps, warmup, max(1, reps // 4))
            rows.append(dict(launch=f'torch autograd of contextual_loss_torch C={c} N={n} (forward + backward)', us=1e3 * ms))
            with torch.no_grad():
                ms = _median_ms(lambda: contextual_loss_torch(x, y, 0.5), steps, warmup, max(1, reps // 4))
            rows.append(dict(launch=f'contextual_loss_torch C={c} N={n} (forward only)', us=1e3 * ms))
        if rgb_patch:
            size, stride = rgb_patch
            gt = 4 * lr
            img = torch.rand(2 * b, 3, gt, gt, generator=torch.Generator().manual_seed(1)).cuda()
            img[:b] = torch.roll(img[b:], (1, 1), (2, 3))
            p = hip.cx_patches(img, size, stride)
            label = f'RGB patches {size} x {size} stride {stride} of {gt} x {gt}: C={p.shape[3]} N={p.shape[1] * p.shape[2]}'
            rows.append(dict(launch=f'cx_patches (2 B images) {label}', us=1e3 * _median_ms(lambda: hip.cx_patches(img, size, stride), steps, warmup, reps)))
            _tap_rows(rows, f'{label} weight_sp={weight_sp}', p[:b], p[b:], weight_sp, steps, warmup, reps)
            gp = torch.randn_like(p[:b])
            rows.append(dict(launch=f'cx_patches_bwd {label}',
                             us=1e3 * _median_ms(lambda: hip.cx_patches_bwd(gp, (b, 3, gt, gt), size, stride), steps, warmup, reps)))
        for name, s in (tap_stride or {}).items():
            c, side = _layer_geometry(name, lr)
            x, y = _fields(b, c, side, side)
            f = torch.cat([x, y]).permute(0, 2, 3, 1).contiguous()
            sub = hip.cx_subsample(f, s)
            label = f'{name} {side} x {side} at stride {s}: C={c} N={sub.shape[1] * sub.shape[2]}'
            rows.append(dict(launch=f'cx_subsample (2 B maps) {label}', us=1e3 * _median_ms(lambda: hip.cx_subsample(f, s), steps, warmup, reps)))
            _tap_rows(rows, f'{label} weight_sp={weight_sp}', sub[:b], sub[b:], weight_sp, steps, warmup, reps)
            gs, gfull = torch.randn_like(sub[:b]), torch.empty_like(f[:b])
            rows.append(dict(launch=f'cx_subsample_bwd {label}', us=1e3 * _median_ms(lambda: hip.cx_subsample_bwd(gs, gfull, s), steps, warmup, reps)))
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


def _step_times(b, k, lr, steps, warmup, taps, extra=None):
    import bench
    import synth
    from mrefsr_amd.models import build_model
    models = {}
    for name, cx in (('l1', None), ('l1_contextual', dict(layer_weights=taps, band_width=0.5, loss_weight=0.1, **(extra or {})))):
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
    out['contextual_opt'] = dict(layer_weights=taps, **(extra or {}))
    return out


def _pair(text):
    size, stride = (int(v) for v in text.split(','))
    return size, stride


def _strides(text):
    return {name: int(s) for name, s in (item.split('=') for item in text.split(','))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--refs', type=int, default=5)
    ap.add_argument('--lr', type=int, default=40)
    ap.add_argument('--weight-sp', type=float, default=0.0, help="CoBi's spatial weight in [0, 1)")
    ap.add_argument('--rgb-patch', type=_pair, metavar='SIZE,STRIDE', help='the RGB patch tap')
    ap.add_argument('--tap-stride', type=_strides, metavar='LAYER=S[,LAYER=S]', help='VGG taps evaluated on a strided grid, e.g. relu2_2=2')
    ap.add_argument('--no-step', action='store_true', help='the launches only')
    ap.add_argument('--out')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'contextual_time.py measures on a GPU'
    rows, clock = _kernel_rows(a.batch, a.lr, a.steps, a.warmup, a.reps, a.weight_sp, a.rgb_patch, a.tap_stride)
    res = dict(batch=a.batch, refs=a.refs, lr=a.lr, launches=rows, launches_clock_mhz=clock)
    for r in rows:
        extra = f"  {r['mflop']:8.1f} MFLOP  {r['tflops']:5.2f} TFLOP/s" if 'tflops' in r else ''
        print(f"{r['launch']:84s} {r['us']:9.1f} us{extra}")
    print('shader clock while the launches ran:', json.dumps(clock))
    if not a.no_step:
        taps, extra = dict(TAPS), {}
        if a.weight_sp > 0:
            extra['weight_sp'] = a.weight_sp
        if a.rgb_patch:
            extra['rgb_patch'] = dict(size=a.rgb_patch[0], stride=a.rgb_patch[1], weight=1.0)
        if a.tap_stride:
            extra['tap_stride'] = a.tap_stride
            taps.update({name: 1.0 for name in a.tap_stride})
        res['step'] = _step_times(a.batch, a.refs, a.lr, a.steps, a.warmup, taps, extra)
        print(json.dumps(res['step']))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
