#!/usr/bin/env python3
"""Step time and launch count of the training step with the parameter-update options ("EMA weights and the Adam
step in HIP"): bench.py's own train-step figure -- B = 4, K = 5, LR 40 x 40, the same warm-up, timing and profiler pass -- on a
model built with train.ema_decay / train.hip_adam / train.grad_clip_norm_g / train.skip_nonfinite_steps set.  bench.py has no way to pass these options and is not changed for it.

  python tools/update_step_time.py [--ema-decay 0.999] [--hip-adam] [--grad-clip-norm-g 1.0] [--skip-nonfinite] [--steps 30]
                                   [--update-launches]

One JSON line: ms_per_step, launches, kernel_ms, loss, and with --update-launches the kernels of the profiled step that belong to
the update (torch's multi-tensor Adam, this project's optim_multi_kernel and gradient-norm kernels).  Run each setting in a fresh process and interleave
the settings; without options it measures the tree as it is (also a tree that does not know the options)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ema-decay', type=float, default=0.0)
    ap.add_argument('--hip-adam', action='store_true')
    ap.add_argument('--grad-clip-norm-g', type=float, default=0.0)
    ap.add_argument('--skip-nonfinite', action='store_true')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--update-launches', action='store_true')
    a = ap.parse_args()
    import torch
    import bench
    from mrefsr_amd import models
    extra = {}
    if a.ema_decay > 0:
        extra['ema_decay'] = a.ema_decay
    if a.hip_adam:
        extra['hip_adam'] = True
    if a.grad_clip_norm_g > 0:
        extra['grad_clip_norm_g'] = a.grad_clip_norm_g
    if a.skip_nonfinite:
        extra['skip_nonfinite_steps'] = True
    build_model = models.build_model

    def build_with_options(opt):
        opt['train'].update(extra)
        return build_model(opt)
    models.build_model = build_with_options
    torch.cuda.set_device(0)
    args = argparse.Namespace(train_steps=a.steps, mode='train', batch=4, refs=5, lr=40, miopen_find=False, dtype='fp32')
    names = []
    if a.update_launches:   # the names of the profiled step's kernels, through the profiler bench.py itself uses
        from torch import profiler
        real = profiler.profile

        class Recording(real):
            def __exit__(self, *exc):
                out = super().__exit__(*exc)
                names.extend(e.name for e in self.events() if e.device_type == torch.autograd.DeviceType.CUDA)
                return out
        profiler.profile = Recording
    res = bench.train_step_figure(args, False, 0)
    out = dict(options=extra, ms_per_step=res['ms_per_step'], steps=res['steps'], launches=res['launches'], kernel_ms=res['kernel_ms'],
               loss=res['loss'])
    if a.update_launches:
        upd = [n for n in names if 'adam' in n.lower() or 'optim_multi' in n or 'multi_tensor_apply' in n or 'grad_walk' in n or 'grad_norm_finalize' in n]
        out['update_kernels'] = {n[:90]: upd.count(n) for n in sorted(set(upd))}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
