#!/usr/bin/env python3
"""Generate tests/golden/optim_ema.npz: the learning rates of the reference's own CosineAnnealingRestartLR
(basicsr/models/lr_scheduler.py:57-96) over 60 iterations, for two period / restart settings, on an optimizer with two parameter
groups (base learning rates 1e-4 and 2.5e-5).  Row 0 is the rate after construction, row i the rate after the i-th scheduler.step().

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_optim.py
(The EMA and Adam yardsticks of tests/test_optim_*_gpu.py are computed from the float64 formulas; they need no fixture.)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refimport as R  # noqa: E402

SETTINGS = [dict(periods=[10, 10, 10, 10, 10, 10], restart_weights=[1, 0.5, 0.5, 0.25, 0.25, 0.1], eta_min=1e-7),
            dict(periods=[25, 40], restart_weights=[1, 0.3], eta_min=0)]
BASE_LRS = [1e-4, 2.5e-5]
ITERS = 60


def main():
    assert R.available(), 'reference tree not present: run in the build container'
    sched_mod = R.ref_module('basicsr.models.lr_scheduler')
    out = {'settings': np.array(json.dumps(dict(settings=SETTINGS, base_lrs=BASE_LRS, iters=ITERS)))}
    for i, kw in enumerate(SETTINGS):
        params = [torch.nn.Parameter(torch.zeros(1)) for _ in BASE_LRS]
        opt = torch.optim.Adam([{'params': [p], 'lr': lr} for p, lr in zip(params, BASE_LRS)])
        sched = sched_mod.CosineAnnealingRestartLR(opt, **kw)
        lrs = [[g['lr'] for g in opt.param_groups]]
        for _ in range(ITERS):
            opt.step()
            sched.step()
            lrs.append([g['lr'] for g in opt.param_groups])
        out[f'lr_{i}'] = np.asarray(lrs, dtype=np.float64)
    np.savez(os.path.join(HERE, 'optim_ema.npz'), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
