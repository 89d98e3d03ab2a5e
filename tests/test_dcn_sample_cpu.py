"""CPU: the sampling rule of csrc/dcn_sample.h, evaluated on the host.  The bilinear set-up is __host__ __device__ and the shape check
is host code; tests/dcn_sample_host.hip is a stand-alone program that evaluates the set-up for float and double on every pair of the
16 x 16 edge classes of tests/golden/dcn_edge_cases.py (maps of side 1, 5 and 70) against a plain restatement of the reference's
rule (offsets, validities, weights and both derivative sets, exactly), checks that nothing contributes on or outside the window
boundary and that the weights of a sample with four corners in range sum to 1 within one ulp, and calls make_geo on the degenerate
shapes.  Built with the host side under -fsanitize=undefined."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dcn_sampling_rule_on_the_host(tmp_path):
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    exe = str(tmp_path / 'dcn_sample_host')
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-std=c++17', '-O1', '-Xarch_host', '-fsanitize=undefined', '-Xarch_host',
                    '-fno-sanitize-recover=undefined', '-I', os.path.join(ROOT, 'mrefsr_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'dcn_sample_host.hip'), '-o', exe], check=True, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'dcn_sample host check: 0 failures' in out.stdout
    assert 'float: 2304 positions' in out.stdout and 'double: 2304 positions' in out.stdout
    assert 'runtime error' not in out.stderr
