#!/usr/bin/env python3
"""What the texture loss costs.

  python tools/texture_time.py [--steps 10] [--warmup 3] [--batch 4] [--refs 5] [--lr 40] [--out FILE.json]

(1) the kernels of csrc/texture.hip and the raw Gram product, per launch (HIP events around --reps back-to-back launches, divided
by their number), at the shapes a training step of --batch samples, --refs references and LR --lr x --lr launches them with;
for the swap, the bytes it must move (the output once, the references' maps and the index planes once) over its time, beside
the 6.3 TB/s a float4 copy reaches on this GPU -- at these sizes everything fits the Infinity Cache;
(2) MultiRefRestorationModel.optimize_parameters at that size (16 residual blocks, synthetic weights): L1 alone and L1 with
train.texture_opt, two models in one process, steps alternating, ms per step (median of --steps after --warmup)."""
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

HBM_COPY_TBS = 6.3
CH = {1: 256, 2: 128, 4: 64}
DIV = {1: 256, 2: 512, 4: 1024}


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


def _kernel_rows(b, k, lr, steps, warmup, reps):
    from mrefsr_amd import hip
    gh = gw = lr - 2
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, gh * gw, (k, b, gh, gw), generator=g).cuda()
    val = (torch.rand(k, b, gh, gw, generator=g) * 3).cuda()
    rows = []

    def row(name, fn, nbytes=None, flops=None):
        ms = _median_ms(fn, steps, warmup, reps)
        r = dict(kernel=name, us=1e3 * ms)
        if nbytes is not None:
            r.update(mbytes=nbytes / 1e6, tb_per_s=nbytes / ms / 1e9, of_copy=nbytes / ms / 1e9 / HBM_COPY_TBS)
        if flops is not None:
            r.update(gflop=flops / 1e9, tflops=flops / ms / 1e9)
        rows.append(r)

    row('texture_select', lambda: hip.texture_select(idx, val), 12.0 * idx.numel() + 12.0 * b * gh * gw)
    sel, wts, pidx = hip.texture_select(idx, val)
    row('texture_coeff (three scales)', lambda: hip.texture_coeff(wts), 4.0 * 21 * b * lr * lr)
    coeff = hip.texture_coeff(wts)
    gxs, gms, norms = {}, {}, None
    for s in (1, 2, 4):
        c, sh = CH[s], s * lr
        feat = torch.relu(torch.randn(k * b, sh, sh, c, generator=g)).cuda()
        x = torch.relu(torch.randn(b, sh, sh, c, generator=g)).cuda()
        out_b = 4.0 * b * sh * sh * c
        row(f'texture_swap_nhwc s={s} C={c}', lambda: hip.texture_swap_nhwc(feat, sel, pidx, k, s), out_b + 4.0 * feat.numel() + 8.0 * sel.numel())
        rows[-1]['gather_mbytes'] = out_b * ((3 * lr - 6) / lr) ** 2 / 1e6     # mean cover x the output: what the gathers request
        maps = hip.texture_swap_nhwc(feat, sel, pidx, k, s)
        row(f'texture_scale_nhwc s={s} C={c}', lambda: hip.texture_scale_nhwc(x, coeff[s]), 2 * out_b)
        fc = hip.texture_scale_nhwc(x, coeff[s])
        row(f'gram_raw_nhwc s={s} C={c}', lambda: hip.gram_raw_nhwc(fc), out_b, 2.0 * b * sh * sh * c * c)
        gxs[s], gms[s] = hip.gram_raw_nhwc(fc), hip.gram_raw_nhwc(hip.texture_scale_nhwc(maps, coeff[s]))
        del feat
        if s == 4:
            order = (4, 2, 1)
            divs = [float((4 * lr * 4 * lr * DIV[t]) ** 2) for t in order]
            row('texture_crit (three layers)', lambda: hip.texture_crit([gxs[t] for t in order], [gms[t] for t in order], divs, 1.0),
                8.0 * sum(gxs[t].numel() for t in order))
            norms = hip.texture_crit([gxs[t] for t in order], [gms[t] for t in order], divs, 1.0)[0]
    g2 = torch.Generator().manual_seed(1)
    for j, s in enumerate((4, 2, 1)):
        c, sh = CH[s], s * lr
        fc = torch.relu(torch.randn(b, sh, sh, c, generator=g2)).cuda()
        df = torch.empty_like(fc)
        scale = 1.0 / 3 / 4 / float((4 * lr * 4 * lr * DIV[s]) ** 2)
        row(f'texture_gram_bwd_nhwc s={s} C={c}',
            lambda: hip.texture_gram_bwd_nhwc(fc, gxs[s], gms[s], coeff[s], norms[j:j + 1], df, scale), 8.0 * fc.numel(), 2.0 * fc.numel() * c)
    return rows


def _opt(texture):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), net_g_pretrain_steps=0,
                 pixel_criterion='L1Loss', pixel_weight=1.0)
    if texture:
        train['texture_opt'] = dict(use_weights=True, loss_weight=1e-3)
    return dict(name='texture_time', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, is_train=True, dist=False,
                network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8),
                network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                                 vgg_type='vgg19'),
                network_extractor=dict(type='ContrasMultiExtractorSep'), path={}, train=train)


def _step_times(b, k, lr, steps, warmup):
    import synth
    from mrefsr_amd.models import build_model
    models = {}
    for name, texture in (('l1', False), ('l1_texture', True)):
        m = build_model(_opt(texture))
        nets = [m.get_bare_model(getattr(m, n)) for n in ('net_g', 'net_extractor', 'net_map')] + ([m.cri_texture] if texture else [])
        for net in nets:
            spec = [(key, tuple(v.shape)) for key, v in net.state_dict().items()]
            net.load_state_dict({key: torch.from_numpy(v) for key, v in synth.state_dict(spec).items()})
        models[name] = m
    samples = [synth.sr_sample(f'texture_time/s{i}', k, lr, lr) for i in range(b)]
    data = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    times = {n: [] for n in models}
    for it in range(1, warmup + steps + 1):
        for name, m in models.items():
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
    out['l_g_texture'] = float(models['l1_texture'].get_current_log()['l_g_texture'])
    out['range_fallbacks'] = {n: m.range_fallbacks for n, m in models.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--refs', type=int, default=5)
    ap.add_argument('--lr', type=int, default=40)
    ap.add_argument('--out')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'texture_time.py measures on a GPU'
    res = dict(batch=a.batch, refs=a.refs, lr=a.lr, kernels=_kernel_rows(a.batch, a.refs, a.lr, a.steps, a.warmup, a.reps),
               step=_step_times(a.batch, a.refs, a.lr, a.steps, a.warmup))
    for r in res['kernels']:
        extra = ''
        if 'tb_per_s' in r:
            extra += f"  {r['mbytes']:8.2f} MB  {r['tb_per_s']:5.2f} TB/s ({100 * r['of_copy']:3.0f} % of the float4 copy)"
        if 'tflops' in r:
            extra += f"  {r['gflop']:6.2f} GFLOP  {r['tflops']:5.1f} TFLOP/s"
        print(f"{r['kernel']:36s} {r['us']:8.1f} us{extra}")
    print(json.dumps(res['step']))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
