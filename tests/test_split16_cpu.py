"""CPU: the operand splits and the amax scale of csrc/split16.h, computed on the host.  The header's conversions, splits and scale
helper are __host__ __device__; tests/split16_host.hip is a stand-alone program that checks them (the scale's window, exactness
and guard; the split errors against the bounds the header states; WH2 against scale_wh) and is built with the host side under
-fsanitize=undefined."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split16_helpers_on_the_host(tmp_path):
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    exe = str(tmp_path / 'split16_host')
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-std=c++17', '-O1', '-Xarch_host', '-fsanitize=undefined', '-Xarch_host',
                    '-fno-sanitize-recover=undefined', '-I', os.path.join(ROOT, 'mrefsr_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'split16_host.hip'), '-o', exe], check=True, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'split16 host check: 0 failures' in out.stdout
    assert 'runtime error' not in out.stderr
