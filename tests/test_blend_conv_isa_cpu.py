"""CPU (needs hipcc): the built ISA of mrattn_blend_conv_kernel (csrc/mrattn_conv.hip), compiled with the library's flags.  The kernel
rests on two blocks living on a CU and on a straight-line tap loop whose blend issues between the MFMAs: a spill to
scratch, more than 256 registers, or MFMAs pushed back into one run behind the blend would undo it without failing a result.
The kernel neither waits by hand nor sets M0 (its tiles go through registers, the compiler counts the waits): both are asserted,
so that a later LDS-DMA version brings its in-flight check with it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-fno-slp-vectorize', '-S', '--cuda-device-only']


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    """{mangled name: lines of the kernel's body and metadata comment}"""
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    asm = str(tmp_path_factory.mktemp('isa') / 'mrattn_conv.s')
    subprocess.run(['hipcc'] + FLAGS + [os.path.join(ROOT, 'mrefsr_amd', 'csrc', 'mrattn_conv.hip'), '-o', asm], check=True, capture_output=True)
    lines = open(asm).read().splitlines()
    starts = [i for i, ln in enumerate(lines) if re.match(r'^_Z\w*mrattn_blend_conv_kernel\w*:', ln)]
    out = {}
    for i in starts:
        end = next(j for j in range(i, len(lines)) if '; ScratchSize:' in lines[j])
        out[lines[i].split(':')[0].strip()] = lines[i:end + 40]
    return out


def test_six_instantiations_without_scratch_at_two_waves_per_simd(kernels):
    assert len(kernels) == 6, sorted(kernels)       # C = 64, 128, 256, with and without valid_bits
    for name, body in kernels.items():
        text = '\n'.join(body)
        assert '; ScratchSize: 0' in text, name
        assert not re.search(r'\bscratch_(load|store)', text), name
        vgprs = int(re.search(r'; NumVgprs: (\d+)', text).group(1)) + int(re.search(r'; NumAgprs: (\d+)', text).group(1))
        assert vgprs <= 256, f'{name}: {vgprs} registers: one wave per SIMD'
        assert re.search(r'; Occupancy: (\d+)', text).group(1) == '2', name


def test_no_packed_fp32_no_hand_waits_no_m0(kernels):
    for name, body in kernels.items():
        text = '\n'.join(body)
        assert not re.search(r'\bv_pk_\w+_f32\b', text), name
        assert '#ASMSTART' not in text, f'{name}: inline assembly (a hand-waited kernel needs its in-flight check: tools/asm_inflight_check.py)'
        assert not re.search(r'\bs_mov_b32\s+m0\b|\bglobal_load_lds_|\bbuffer_load\w*\s.*\blds\b', text), name


def test_blend_issues_between_the_mfmas(kernels):
    """the VALU work of the blend sits between the MFMAs: of the gaps between consecutive MFMAs at least two thirds carry four or
    more VALU instructions (eight of a pass's nine taps carry the next tap's blend in 11 of their 12 slots, the last tap only the
    derived weight plane: 90 of 108; issued back to back, as the compiler orders the loop when left to itself, it is under a tenth)"""
    for name, body in kernels.items():
        code = [ln.split(';')[0].strip() for ln in body]
        code = [ln for ln in code if ln and not ln.startswith('.') and not ln.endswith(':')]
        mfma = [i for i, ln in enumerate(code) if ln.startswith('v_mfma_f32_32x32x16_f16')]
        assert len(mfma) >= 6 * 9 * 12, f'{name}: {len(mfma)} MFMAs (six variants of nine unrolled taps)'
        gaps = [sum(1 for ln in code[a + 1:b] if ln.startswith('v_')) for a, b in zip(mfma, mfma[1:])]
        filled = sum(1 for g in gaps if g >= 4)
        print(f'{name}: {len(mfma)} MFMAs, {filled} of {len(gaps)} gaps with >= 4 VALU instructions')
        assert filled >= len(gaps) * 8 // 12, name
