#!/usr/bin/env python3
"""What a reference pool costs (ref_select).

  python tools/refselect_bench.py [--lr 40 125] [--pool 10] [--top-k 5] [--steps 10] [--warmup 3] [--out FILE.json]

Per LR size, on one model (16 residual blocks, synthetic weights, B = 1) in one process, the three calls alternating inside every
timed round:
  (a) test() fed the pool of --pool references with ref_select top_k = --top-k;
  (b) test() fed all --pool references, no selection;
  (c) test() fed --top-k references;
ms per call (median over --steps rounds after --warmup), the shader clock sampled while the rounds run.  Then the launches of
csrc/refselect.hip alone at the shapes (a) makes them with (HIP events around --reps back-to-back launches): hip.ref_select in both
score modes, hip.ref_gather of the index maps, the value maps and the image stack, and the image gather against a float4 copy of the
same bytes (torch's copy_ of the K B gathered rows) -- at those shapes every launch is bound by the host's ~12 us per call, so the
gather and the copy are timed once more on rows of 48 MiB, past the Infinity Cache.  With random-init weights nothing is said about image quality."""
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


def _events_ms(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _median_ms(fn, steps, warmup, reps=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(_events_ms(fn, reps) for _ in range(steps))


def _model(top_k):
    import synth
    from mrefsr_amd.models import build_model
    opt = dict(name='refselect_bench', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, is_train=False, dist=False,
               network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8),
               network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                                vgg_type='vgg19'),
               network_extractor=dict(type='ContrasMultiExtractorSep'), path={}, val={}, ref_select=dict(top_k=top_k))
    model = build_model(opt)
    for net in (model.get_bare_model(model.net_g), model.net_extractor, model.net_map):
        spec = [(key, tuple(v.shape)) for key, v in net.state_dict().items()]
        net.load_state_dict({key: torch.from_numpy(v) for key, v in synth.state_dict(spec).items()})
    return model


def _data(lr, n):
    import synth
    s = synth.sr_sample(f'refselect_bench/{lr}', n, lr, lr)
    return {k: torch.from_numpy(np.ascontiguousarray(v[None])).cuda() for k, v in s.items()}


def _calls(model, lr, pool, top_k, steps, warmup):
    import bench
    data = _data(lr, pool)
    few = dict(data, img_ref_list=data['img_ref_list'][:, :top_k].contiguous())
    select = model.ref_select

    def run(d, sel):
        model.ref_select = sel
        model.feed_data(d)
        model.test()

    variants = dict(pool_selected=lambda: run(data, select), all_fed=lambda: run(data, None), top_k_fed=lambda: run(few, None))
    try:
        for _ in range(warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        ts = {name: [] for name in variants}
        with bench.ClockSampler(0) as clock:
            for _ in range(steps):
                for name, fn in variants.items():   # (alternating: all three see the same clock and the same neighbours)
                    ts[name].append(_events_ms(fn))
    finally:
        model.ref_select = select
    res = {f'test_ms_{name}': statistics.median(v) for name, v in ts.items()}
    res.update({f'test_ms_{name}_min_max': [min(v), max(v)] for name, v in ts.items()})
    run(data, select)
    res.update(lr=lr, pool=pool, top_k=top_k, clock_mhz=clock.summary(), range_fallbacks=model.range_fallbacks,
               selection=model.ref_selection.tolist(), scores=model.ref_scores.tolist())
    return res


def _kernels(lr, pool, top_k, steps, warmup, reps):
    from mrefsr_amd import hip
    gh = lr - 2
    hr = 4 * lr
    val = torch.rand(pool, 1, gh, gh, device='cuda') * 2 - 1
    idx = torch.randint(0, gh * gh, (pool, gh, gh), device='cuda', dtype=torch.int64)
    imgs = torch.rand(pool, 3, hr, hr, device='cuda')
    rows = []
    for mode in ('mean', 'wins'):
        ms = _median_ms(lambda: hip.ref_select(val, None, top_k, mode), steps, warmup, reps)
        rows.append(dict(launch=f'ref_select, {mode} (two kernels)', us=1e3 * ms, mbytes=4 * val.numel() / 1e6, tb_per_s=4 * val.numel() / ms / 1e9))
    sel = hip.ref_select(val, None, top_k, 'mean')[0]
    for name, src in (('index maps (int64)', idx), ('value maps (fp32)', val.view(pool, gh, gh)), ('image stack (fp32)', imgs)):
        out = torch.empty((top_k, *src.shape[1:]), device='cuda', dtype=src.dtype)
        ms = _median_ms(lambda: hip.ref_gather(src, sel, pool, out=out), steps, warmup, reps)
        nbytes = 2 * out.numel() * out.element_size()
        rows.append(dict(launch=f'ref_gather, {name}', row_bytes=src[0].numel() * src.element_size(), us=1e3 * ms, mbytes=nbytes / 1e6,
                         tb_per_s=nbytes / ms / 1e9))
    out, src = torch.empty((top_k, 3, hr, hr), device='cuda'), imgs[:top_k]
    ms = _median_ms(lambda: out.copy_(src), steps, warmup, reps)
    nbytes = 2 * 4 * out.numel()
    rows.append(dict(launch='float4 copy of the image gather\'s bytes (torch copy_)', us=1e3 * ms, mbytes=nbytes / 1e6, tb_per_s=nbytes / ms / 1e9))
    return rows


def _kernels_past_the_cache(pool, top_k, steps, warmup, reps, side=2048):
    """the gather where the launch, not the host, takes the time and the bytes pass the 256-MiB Infinity Cache: rows of 3 x side x side
    floats (48 MiB at 2048), against torch's copy_ of the same K rows"""
    from mrefsr_amd import hip
    imgs = torch.rand(pool, 3, side, side, device='cuda')
    sel = torch.arange(0, 2 * top_k, 2, device='cuda', dtype=torch.int32).clamp_(max=pool - 1).view(1, top_k)
    out = torch.empty((top_k, 3, side, side), device='cuda')
    nbytes = 2 * 4 * out.numel()
    rows = []
    for name, fn in (('ref_gather, image rows past the Infinity Cache', lambda: hip.ref_gather(imgs, sel, pool, out=out)),
                     ('float4 copy of the same bytes (torch copy_)', lambda: out.copy_(imgs[:top_k]))):
        ms = _median_ms(fn, steps, warmup, reps)
        rows.append(dict(launch=name, row_bytes=12 * side * side, us=1e3 * ms, mbytes=nbytes / 1e6, tb_per_s=nbytes / ms / 1e9))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lr', type=int, nargs='+', default=[40, 125])
    ap.add_argument('--pool', type=int, default=10)
    ap.add_argument('--top-k', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20, help='back-to-back launches per timed window of a kernel')
    ap.add_argument('--out')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'refselect_bench.py measures on the GPU'
    assert 1 <= a.top_k < a.pool <= 32
    torch.cuda.set_device(0)
    model = _model(a.top_k)
    res = dict(sizes=[])
    for lr in a.lr:
        r = _calls(model, lr, a.pool, a.top_k, a.steps, a.warmup)
        r['kernels'] = _kernels(lr, a.pool, a.top_k, a.steps, a.warmup, a.reps)
        res['sizes'].append(r)
        torch.cuda.empty_cache()
    res['kernels_past_the_cache'] = _kernels_past_the_cache(a.pool, a.top_k, a.steps, a.warmup, a.reps)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
