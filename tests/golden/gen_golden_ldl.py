#!/usr/bin/env python3
"""Generate tests/golden/ldl.npz: the reference's own artifact map and LDL loss (basicsr/losses/loss_util.py:99-145,
get_refined_artifact_map; used as l1_loss(w out, w gt) by basicsr/models/realesrgan_model.py:211-226) with autograd in float64 on
the CPU, on the inputs of tests/golden/ldl_cases.py at 1 x 4 x 4, 1 x 5 x 6, 1 x 7 x 9 and 3 x 33 x 17, both classes.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_ldl.py
loss_util.py is loaded by file path (the package's __init__ cannot be imported; the module itself needs only torch).  Stored per
case <class>_<B>x<H>x<W>: the fp32 inputs out, gt, ema, and in float64 the map w, the loss and d loss / d out.  The map is not
detached, as in the reference.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ldl_cases  # noqa: E402
from _refimport import REF_ROOT  # noqa: E402  (where the reference tree lies; nothing else of that module is used)

LOSS_WEIGHT = 1.0


def main():
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location('_ref_loss_util', os.path.join(REF_ROOT, 'basicsr', 'losses', 'loss_util.py'))
    lu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lu)
    arrays = {'loss_weight': np.array(LOSS_WEIGHT)}
    for ci, cls in enumerate(ldl_cases.CLASSES):
        for si, shape in enumerate(ldl_cases.GOLDEN_SHAPES):
            out, gt, ema = ldl_cases.make_inputs(cls, shape, 7000 + 100 * ci + si)
            o = out.double().requires_grad_(True)
            w = lu.get_refined_artifact_map(gt.double(), o, ema.double(), 7)
            loss = LOSS_WEIGHT * torch.nn.functional.l1_loss(torch.mul(w, o), torch.mul(w, gt.double()), reduction='mean')
            loss.backward()
            r = (gt.double() - out.double()).abs().sum(1, keepdim=True)
            r_e = (gt.double() - ema.double()).abs().sum(1, keepdim=True)
            ties = int((r == r_e).sum())
            assert bool(((r - r_e).abs() >= 1e-3).logical_or(r == r_e).all())
            key = ldl_cases.golden_key(cls, shape)
            print(f'{key:22s} loss {float(loss):.6e}  max w {float(w.max()):.3e}  masked {float((w == 0).double().mean()):.2f}  '
                  f'ties {ties}  max |grad| {float(o.grad.abs().max()):.3e}')
            arrays.update({f'{key}_out': out.numpy(), f'{key}_gt': gt.numpy(), f'{key}_ema': ema.numpy(), f'{key}_w': w.detach().numpy(),
                           f'{key}_loss': np.array(float(loss)), f'{key}_grad': o.grad.numpy()})
    np.savez_compressed(os.path.join(HERE, 'ldl.npz'), **arrays)


if __name__ == '__main__':
    main()
