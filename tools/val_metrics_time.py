#!/usr/bin/env python3
"""Validation metric time on the host (numpy) and on the device (csrc/metrics.hip), DESIGN 3.7.

  python tools/val_metrics_time.py [--images 126] [--reps 20] [--out FILE.json] [--trace]

(1) per 500 x 500 image pair (fp32 on the GPU, as nondist_validation holds them), median over --reps:
    host:   tensor2img x 2 (with their device-to-host copies), calculate_psnr, PSNR-Y, SSIM-Y, each timed on its own;
    device: metrics.validation_metrics (launches + the one copy of the result rows; the host clock after the copy returns), and the
            three kernels alone between device events;
(2) one MultiRefRestorationModel.validation pass over --images synthetic CUFED5-shaped samples (LR 125 x 125 zero-padded, 5
    references of 500 x 500, GT cropped to CUFED5-like sizes, crop_border 4), in both modes, after one warm-up pass each.
--trace: one device-mode pass over --images samples only (for rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = [(500, 332), (332, 500), (500, 500), (375, 500), (500, 375), (480, 320)]   # GT sizes of the synthetic set (mod 4)


def _host_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def _event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def per_image(reps):
    from mrefsr_amd import hip, metrics
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(1, 3, 500, 500, generator=g)
    out = (gt + 0.03 * torch.randn(1, 3, 500, 500, generator=g)).cuda()
    gt = gt.cuda()
    a, b = metrics.tensor2img(out), metrics.tensor2img(gt)
    host = dict(tensor2img_x2=_host_ms(lambda: (metrics.tensor2img(out), metrics.tensor2img(gt)), reps),
                psnr=_host_ms(lambda: metrics.calculate_psnr(a, b, 4), reps),
                psnr_y=_host_ms(lambda: metrics.calculate_psnr(a, b, 4, test_y_channel=True), reps),
                ssim_y=_host_ms(lambda: metrics.calculate_ssim(a, b, 4, test_y_channel=True), reps))
    host['total'] = sum(host.values())
    dev = dict(validation_metrics=_host_ms(lambda: metrics.validation_metrics(out, gt, 4), 5 * reps),
               kernels=_event_ms(lambda: hip.val_metrics(out, gt, 4), 5 * reps))
    want = (metrics.calculate_psnr(a, b, 4), metrics.calculate_psnr(a, b, 4, True), metrics.calculate_ssim(a, b, 4, True))
    got = metrics.validation_metrics(out, gt, 4)
    diff = max(abs(got[k][0] - w) for k, w in zip(('psnr', 'psnr_y', 'ssim_y'), want))
    return dict(host_ms=host, device_ms=dev, max_abs_diff=diff)


class _Set(torch.utils.data.Dataset):
    """CUFED5-shaped samples as MultiRefCUFEDSet yields them (a few distinct inputs, cycled)"""
    opt = dict(name='CUFED5-synthetic')

    def __init__(self, n):
        import synth
        self.n = n
        self.samples = []
        for i, (oh, ow) in enumerate(SIZES):
            s = synth.sr_sample(f'val_time/{i}', 5, 125, 125)
            s['img_in'] = np.ascontiguousarray(s['img_in'][:, :oh, :ow])
            self.samples.append(s)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        j = i % len(self.samples)
        d = {k: torch.from_numpy(v) for k, v in self.samples[j].items()}
        d.update(lq_path=f'{i:03d}_multi.png', padding=True, original_size=SIZES[j])
        return d


def _model():
    import synth
    from mrefsr_amd.models import build_model
    opt = dict(name='val_time', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, is_train=False, dist=False,
               network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8),
               network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                                vgg_type='vgg19'),
               network_extractor=dict(type='ContrasMultiExtractorSep'), path={}, val=dict(save_img=False))
    model = build_model(opt)
    for net in (model.get_bare_model(model.net_g), model.net_extractor, model.net_map):
        spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()})
    return model


def validation_pass(model, loader, on_device):
    model.opt['val']['metrics_on_device'] = on_device
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = model.validation(loader, 0, None, save_img=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=126)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    import logging
    logging.getLogger('basicsr').setLevel(logging.ERROR)
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    model = _model()
    loader = torch.utils.data.DataLoader(_Set(args.images), batch_size=1, shuffle=False, num_workers=0)
    if args.trace:
        ms, res = validation_pass(model, loader, True)
        print(json.dumps(dict(trace_pass_ms=ms, result=res)))
        return
    result = dict(per_image_500x500=per_image(args.reps), images=args.images)
    for mode in (False, True):          # warm-up: kernels, workspaces, the first forward at this shape
        validation_pass(model, torch.utils.data.DataLoader(_Set(2), batch_size=1), mode)
    passes = {}
    for mode, name in ((False, 'host'), (True, 'device'), (False, 'host_again'), (True, 'device_again')):
        ms, res = validation_pass(model, loader, mode)
        passes[name] = dict(ms=ms, **{k: float(v) for k, v in res.items()})
    result['validation_pass'] = passes
    result['pass_speedup'] = min(passes['host']['ms'], passes['host_again']['ms']) / min(passes['device']['ms'], passes['device_again']['ms'])
    result['pass_max_abs_diff'] = max(abs(passes['device'][k] - passes['host'][k]) for k in ('psnr', 'psnr_y', 'ssim_y'))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
