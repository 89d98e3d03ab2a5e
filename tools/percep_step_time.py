#!/usr/bin/env python3
"""What the perceptual / style loss adds to a training step.

  python tools/percep_step_time.py [--steps 10] [--warmup 3] [--out FILE.json] [--trace]

(1) MultiRefRestorationModel.optimize_parameters at B = 4, K = 5, LR 40 x 40 (GT 160 x 160) in three configurations -- L1 only, L1 +
perceptual (layers conv1_2 .. conv5_4), L1 + perceptual + style -- ms per step (median of --steps, after --warmup);
(2) PerceptualLoss forward + backward alone on [4,3,160,160] images, with the pool's arg-max recomputed and stored;
(3) per layer: the forward convolution (2B images), the input-gradient convolution (B images), the pool kernels, and per tap the
criterion / Gram kernels, each timed by HIP events over repeated launches.
--trace: one perceptual + style step only (for rocprofv3 --kernel-trace --stats)."""
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

LAYERS = {'conv1_2': 0.1, 'conv2_2': 0.1, 'conv3_4': 1.0, 'conv4_4': 1.0, 'conv5_4': 1.0}


def _opt(percep, style):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000], gamma=0.5), net_g_pretrain_steps=0, pixel_criterion='L1Loss',
                 pixel_weight=1.0)
    if percep:
        train['perceptual_opt'] = dict(layer_weights=LAYERS, perceptual_weight=1.0, style_weight=0.0, criterion='l1')
    if style:
        train['style_opt'] = dict(layer_weights=LAYERS, perceptual_weight=0.0, style_weight=100.0, criterion='l1')
    return dict(name='percep_time', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, is_train=True, dist=False,
                network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8),
                network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                                 vgg_type='vgg19'),
                network_extractor=dict(type='ContrasMultiExtractorSep'), path={}, train=train)


def _model(percep, style):
    import synth
    from mrefsr_amd.models import build_model
    model = build_model(_opt(percep, style))
    nets = [model.get_bare_model(model.net_g), model.net_extractor, model.net_map]
    nets += [c for c in (model.cri_perceptual, model.cri_style) if c is not None]
    for net in nets:
        spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()})
    samples = [synth.sr_sample(f'percep_time/s{i}', 5, 40, 40) for i in range(4)]
    model.feed_data({n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]})
    return model


def _events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def step_times(steps, warmup):
    out = {}
    for name, percep, style in (('l1', False, False), ('l1_percep', True, False), ('l1_percep_style', True, True)):
        model = _model(percep, style)
        for i in range(warmup):
            model.optimize_parameters(i + 1)
        torch.cuda.synchronize()
        ts = []
        for i in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            model.optimize_parameters(warmup + i + 1)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        out[name] = dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), losses=model.get_current_log(),
                         range_fallbacks=model.range_fallbacks)
        del model
        torch.cuda.empty_cache()
    return out


def loss_alone(reps):
    from mrefsr_amd.archs import nhwc_train
    from mrefsr_amd.losses import PerceptualLoss
    import synth
    out = {}
    for style in (False, True):
        loss = PerceptualLoss(LAYERS, perceptual_weight=1.0, style_weight=100.0 if style else 0.0).cuda()
        spec = [(k, tuple(v.shape)) for k, v in loss.state_dict().items()]
        loss.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()})
        g = torch.Generator().manual_seed(0)
        gt = torch.rand(4, 3, 160, 160, generator=g).cuda()
        x = (gt + 0.05 * torch.randn(gt.shape, generator=g).cuda()).clamp(0, 1).requires_grad_(True)

        def fwd_bwd():
            p, s = loss(x, gt)
            (p + s if s is not None else p).backward()

        def fwd():
            with torch.no_grad():
                loss(x, gt)
        for plane in (False, True):
            nhwc_train.POOL_PLANE = plane
            key = ('percep_style' if style else 'percep') + ('_plane' if plane else '_recompute')
            out[key] = dict(fwd_bwd_ms=_events(fwd_bwd, reps), fwd_ms=_events(fwd, reps))
        nhwc_train.POOL_PLANE = False
    return out


def per_layer(reps):
    """the VGG node's launches one by one at B = 4, GT 160 x 160 (2B = 8 images forward)"""
    from mrefsr_amd import hip
    from mrefsr_amd.archs import nhwc_train
    from mrefsr_amd.archs.vgg_arch import VGGFeatureExtractor
    import synth
    vgg = VGGFeatureExtractor(list(LAYERS)).cuda()
    spec = [(k, tuple(v.shape)) for k, v in vgg.state_dict().items()]
    vgg.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()})
    b = 4
    g = torch.Generator().manual_seed(1)
    h = hip.image_to_nhwc4(torch.rand(2 * b, 3, 160, 160, generator=g).cuda(), vgg.mean, vgg.std, True)
    rows = []
    for name, mod in vgg.vgg_net._modules.items():
        if isinstance(mod, torch.nn.Conv2d):
            pk, terms = nhwc_train._vgg_pack(mod.weight, (0, mod.in_channels), False)
            pkd, termsd = nhwc_train._vgg_pack(mod.weight, (0, mod.in_channels), True)
            x = h
            n, hh, ww, _ = x.shape
            fwd = _events(lambda: hip.conv_nhwc(x, pk, mod.bias.detach(), mod.out_channels, 3, act=True, slope=0.0), reps)
            h = hip.conv_nhwc(x, pk, mod.bias.detach(), mod.out_channels, 3, act=True, slope=0.0)
            gy = torch.randn(b, hh, ww, mod.out_channels, generator=g).cuda() * 1e-6
            amax = gy.abs().max().reshape(1)
            cin = mod.in_channels
            if cin % 4 == 0:
                dg = _events(lambda: hip.conv_nhwc(gy, pkd, None, cin, 3, in_amax=amax if termsd == 16 else None), reps)
            else:
                g4 = torch.empty(b, hh, ww, 4, device='cuda')
                dg = _events(lambda: hip.conv_nhwc(gy, pkd, None, cin, 3, out=g4[..., :cin], in_amax=amax if termsd == 16 else None), reps)
            flop = 2.0 * hh * ww * cin * mod.out_channels * 9
            row = dict(layer=name, hw=[hh, ww], cin=cin, cout=mod.out_channels, fwd_ms=fwd, fwd_tflops=2 * b * flop / fwd / 1e9,
                       dgrad_ms=dg, dgrad_tflops=b * flop / dg / 1e9)
            if name in LAYERS:
                t = h
                row['tap_l1_loss_ms'] = _events(lambda: hip.tap_crit_loss([t[:b]], [t[b:]], [1.0], [0], 'l1', (1.0, 0.0)), reps)
                gr = torch.empty_like(t[:b])
                row['tap_l1_grad_ms'] = _events(lambda: hip.tap_crit_grad(t[:b], t[b:], gr, 1.0, 0, 'l1', (1.0, 0.0)), reps)
                row['gram_ms'] = _events(lambda: hip.gram_nhwc(t), reps)
                gm = hip.gram_nhwc(t)
                row['gram_bwd_ms'] = _events(lambda: hip.gram_bwd_nhwc(t[:b], gm[:b], gm[b:], gr, 100.0, 1.0, accumulate=True), reps)
            rows.append(row)
        elif isinstance(mod, torch.nn.MaxPool2d):
            x = h
            n, hh, ww, c = x.shape
            rec = _events(lambda: hip.maxpool2_nhwc(x), reps)
            pl = _events(lambda: hip.maxpool2_nhwc(x, want_plane=True), reps)
            p_, plane = hip.maxpool2_nhwc(x, want_plane=True)
            gp = torch.randn(b, hh // 2, ww // 2, c, generator=g).cuda()
            brec = _events(lambda: hip.maxpool2_bwd_nhwc(gp, x[:b]), reps)
            bpl = _events(lambda: hip.maxpool2_bwd_nhwc(gp, None, plane[:b], shape=(b, hh, ww, c)), reps)
            rows.append(dict(layer=name, hw=[hh, ww], c=c, fwd_ms=rec, fwd_plane_ms=pl, bwd_recompute_ms=brec, bwd_plane_ms=bpl))
            h = p_
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', action='store_true', help='one perceptual + style step after one warm-up step, nothing else')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.trace:
        model = _model(True, True)
        model.optimize_parameters(1)
        torch.cuda.synchronize()
        model.optimize_parameters(2)
        torch.cuda.synchronize()
        print(json.dumps(model.get_current_log()))
        return
    res = dict(steps=step_times(args.steps, args.warmup), loss_alone=loss_alone(args.reps), per_layer=per_layer(args.reps))
    s = res['steps']
    res['added_ms'] = dict(percep=s['l1_percep']['median_ms'] - s['l1']['median_ms'],
                           percep_style=s['l1_percep_style']['median_ms'] - s['l1']['median_ms'])
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(txt)


if __name__ == '__main__':
    main()
