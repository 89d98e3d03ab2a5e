#!/usr/bin/env python3
"""What the x8 geometric self-ensemble of test() costs.

  python tools/selfens_time.py [--steps 10] [--warmup 3] [--lr 125] [--refs 5] [--out FILE.json]

(1) the two kernels of csrc/selfens.hip, per launch (HIP events around --reps back-to-back launches, divided by their number), at the
shapes an ensemble test() of the CUFED validation size launches them with (LR 125 x 125, K = 5, B = 1: the LR input, the up-sampled
input, the reference stack, the merge of the two groups' outputs), and at shapes larger than the 256-MiB Infinity Cache, where the
bytes really come from and go to HBM; bytes moved (every operand and result once) over time, as TB/s and as a fraction of the
6.3 TB/s a float4 copy reaches on this GPU (8.0 TB/s in the data sheet);
(2) MultiRefRestorationModel.test() at that size (16 residual blocks, synthetic weights): plain, with val.self_ensemble, and the
hand-written loop the option replaces -- eight feed_data + test() calls on torch-transformed inputs, their outputs inverse-transformed
and averaged in torch -- ms per call (median of --steps, after --warmup), all three on the same model in the same process."""
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

HBM_COPY_TBS, HBM_SPEC_TBS = 6.3, 8.0


def _median_ms(fn, steps, warmup, reps=1):
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


def _kernel_rows(lr, k, steps, warmup, reps):
    from mrefsr_amd import hip
    hr = 4 * lr
    big = 1024
    shapes = [('expand LR input', (1, 3, lr, lr), 1), ('expand up-sampled input', (1, 3, hr, hr), 1), ('expand reference stack', (k, 3, hr, hr), k),
              ('expand, past the Infinity Cache', (64, 3, big, big), 1)]
    rows = []
    for name, shape, outer in shapes:
        x = torch.randn(shape, device='cuda')
        for tr in (0, 1):
            ms = _median_ms(lambda: hip.dihedral_expand(x, tr, outer=outer), steps, warmup, reps)
            nbytes = 5 * 4 * x.numel()
            rows.append(dict(kernel=f'{name}, tr = {tr}', shape=list(shape), us=1e3 * ms, mbytes=nbytes / 1e6, tb_per_s=nbytes / ms / 1e9))
        del x
    for name, n, side in (('merge', 1, hr), ('merge, past the Infinity Cache', 16, big)):
        a, b = torch.randn(4 * n, 3, side, side, device='cuda'), torch.randn(4 * n, 3, side, side, device='cuda')
        ms = _median_ms(lambda: hip.dihedral_merge(a, b), steps, warmup, reps)
        nbytes = 9 * 4 * n * 3 * side * side
        rows.append(dict(kernel=name, shape=[4 * n, 3, side, side], us=1e3 * ms, mbytes=nbytes / 1e6, tb_per_s=nbytes / ms / 1e9))
        del a, b
    for r in rows:
        r['of_hbm_copy_rate'] = r['tb_per_s'] / HBM_COPY_TBS
        r['of_hbm_spec'] = r['tb_per_s'] / HBM_SPEC_TBS
    return rows


def _model(lr, k):
    import synth
    from mrefsr_amd.models import build_model
    opt = dict(name='selfens_time', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, is_train=False, dist=False,
               network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8),
               network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                                vgg_type='vgg19'),
               network_extractor=dict(type='ContrasMultiExtractorSep'), path={}, val={})
    model = build_model(opt)
    for net in (model.get_bare_model(model.net_g), model.net_extractor, model.net_map):
        spec = [(key, tuple(v.shape)) for key, v in net.state_dict().items()]
        net.load_state_dict({key: torch.from_numpy(v) for key, v in synth.state_dict(spec).items()})
    s = synth.sr_sample('selfens_time', k, lr, lr)
    return model, {n: torch.from_numpy(np.ascontiguousarray(v[None])).cuda() for n, v in s.items()}


def _copy(t, j, tr):
    if j & 1:
        t = t.flip(-1)
    if j & 2:
        t = t.flip(-2)
    return t.transpose(-1, -2) if tr else t


def _inverse(t, j, tr):
    if tr:
        t = t.transpose(-1, -2)
    if j & 2:
        t = t.flip(-2)
    return t.flip(-1) if j & 1 else t


def _hand_loop(model, data):
    """what a user writes around feed_data / test() without the option: eight batch-1 passes"""
    acc = None
    for tr in (0, 1):
        for j in range(4):
            model.feed_data({n: _copy(t, j, tr).contiguous() for n, t in data.items()})
            model.test()
            out = _inverse(model.output, j, tr)
            acc = out if acc is None else acc + out
    return acc * 0.125


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20, help='back-to-back launches per timed window of a kernel')
    ap.add_argument('--lr', type=int, default=125)
    ap.add_argument('--refs', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'selfens_time.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(lr=a.lr, refs=a.refs, kernels=_kernel_rows(a.lr, a.refs, a.steps, a.warmup, a.reps))
    torch.cuda.empty_cache()
    model, data = _model(a.lr, a.refs)

    def call():
        model.feed_data(data)
        model.test()
    res['test_ms_plain'] = _median_ms(call, a.steps, a.warmup)
    plain = model.output.clone()
    model.opt['val']['self_ensemble'] = True
    res['test_ms_self_ensemble'] = _median_ms(call, a.steps, a.warmup)
    ens = model.output.clone()
    model.opt['val']['self_ensemble'] = False
    res['test_ms_eight_single_calls'] = _median_ms(lambda: _hand_loop(model, data), a.steps, a.warmup)
    loop = _hand_loop(model, data)
    # (batch 4 and batch 1 differ in their batch-wide input scales: the two ensembles agree closely, not bit for bit)
    res['max_abs_ensemble_minus_hand_loop'] = float((ens - loop).abs().max())
    res['max_abs_ensemble_minus_plain'] = float((ens - plain).abs().max())
    res['range_fallbacks'] = model.range_fallbacks
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
