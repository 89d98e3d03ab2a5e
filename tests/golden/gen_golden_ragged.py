#!/usr/bin/env python3
"""Generate tests/golden/e2e_ragged.npz: the reference's own MultiRefRestorationModel.test() and optimize_parameters(1)
(multi_ref_restoration_model.py:197-294) at an LR size whose sides are not multiples of 4: B = 2, K = 3, LR 45 x 39 -> GT 180 x 156.
MRAPAFusion then reflect-pads its inputs at the bottom and right and crops the result back (ref_mrapa_restoration_arch.py:306-311,
348): pads of 3 x 1 at the small scale (45 x 39), 2 x 2 at the medium scale (90 x 78), none at the large one.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_ragged.py
The nets, weights and inputs are made exactly as gen_golden.gen_e2e does for the other e2e fixtures.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402


def main():
    assert G.R.available(), 'reference tree not present: run in the build container'
    G.R.install()
    G.gen_e2e(2, 3, 45, 39, 'e2e_ragged', store_inputs=False, key='e2e_ragged')


if __name__ == '__main__':
    main()
