"""CPU: the build of csrc/metrics.hip, the shape checks of its C entry points, the val.metrics_on_device option and the refusal of
CPU tensors by the device metrics.  The GPU side: tests/test_metrics_device_gpu.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_metrics_kernels_compile_without_scratch(tmp_path):
    """every kernel of csrc/metrics.hip builds for gfx950 (with the Makefile's -ffp-contract=off) and uses no scratch memory"""
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    asm = str(tmp_path / 'metrics.s')
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-fno-slp-vectorize', '-ffp-contract=off',
                    '-S', '--cuda-device-only', os.path.join(ROOT, 'mrefsr_amd', 'csrc', 'metrics.hip'), '-o', asm], check=True, capture_output=True)
    text = open(asm).read()
    kernels = re.findall(r'^(_ZN12_GLOBAL__N_1\d+(\w+?_kernel)\w*):', text, flags=re.M)
    names = sorted({k for _, k in kernels})
    assert names == ['finish_kernel', 'quant_kernel', 'ssim_kernel', 'tensor2img_kernel'], names
    sizes = re.findall(r'; ScratchSize: (\d+)', text)
    assert len(sizes) == len(kernels) and set(sizes) == {'0'}, sizes
    assert 'metrics.o: FPFLAGS := -ffp-contract=off' in open(os.path.join(ROOT, 'mrefsr_amd', 'csrc', 'Makefile')).read()


def test_y_table_is_the_float32_quotient():
    """the kernels widen float(double(v) / 255) for rgb_to_y's float32 v / 255: the same float for every uint8 value"""
    v = np.arange(256)
    assert (np.float32(v) / np.float32(255.) == (v / 255.0).astype(np.float32)).all()


def _call(n=1, h=32, w=32, hg=None, wg=None, sizes=None, cb=0, flags=1, ws_bytes=None):
    """the C entry point with non-null dummy device pointers: each case here is refused before anything is launched"""
    from mrefsr_amd import _lib
    lib = _lib.load()
    hg, wg = hg or h, wg or w
    sz = C.c_void_p(0)
    if sizes is not None:
        flat = [v for s in sizes for v in s]
        keep = (C.c_int * len(flat))(*flat)
        sz = C.cast(keep, C.c_void_p)
    need = lib.mrefsr_val_metrics_workspace_bytes(n, h, w)
    dummy = C.c_void_p(256)
    with pytest.raises(_lib.MrefsrHipError) as e:
        _lib.call('mrefsr_val_metrics_f32', dummy, dummy, n, h, w, hg, wg, sz, cb, flags, C.c_void_p(0), dummy, dummy,
                  C.c_int64(need if ws_bytes is None else ws_bytes), C.c_void_p(0))
    return str(e.value)


def test_c_entry_refuses_bad_shapes():
    from mrefsr_amd import _lib
    lib = _lib.load()
    assert lib.mrefsr_val_metrics_workspace_bytes(0, 8, 8) < 0
    assert lib.mrefsr_val_metrics_workspace_bytes(1, 500, 500) >= 6 * 500 * 500
    assert 'at least 11x11' in _call(h=10, w=40)                           # SSIM needs the 11 x 11 window
    assert 'at least 11x11' in _call(h=18, w=40, cb=4)                     # ... after the crop: 18 - 8 = 10
    assert 'at least 11x11' in _call(h=32, w=32, sizes=[(14, 32)], cb=2)   # ... of the valid region
    assert 'at least 1x1' in _call(h=8, w=40, cb=4, flags=0)               # PSNR alone: one pixel
    assert 'outside' in _call(h=32, w=32, hg=20, wg=32, sizes=[(24, 32)])  # the region must lie in both tensors
    assert 'differ' in _call(h=32, w=32, hg=20, wg=32)                     # unequal shapes need sizes
    assert 'flags' in _call(flags=4)
    assert 'crop_border' in _call(cb=-1)
    assert 'workspace' in _call(ws_bytes=16)


def test_cpu_tensors_are_refused():
    from mrefsr_amd import metrics
    x, y = torch.rand(1, 3, 24, 24), torch.rand(1, 3, 24, 24)
    for fn in (lambda: metrics.tensor2img_device(x), lambda: metrics.validation_metrics(x, y, 0),
               lambda: metrics.calculate_psnr_device(x, y, 0), lambda: metrics.calculate_ssim_device(x[0], y[0], 0, test_y_channel=True)):
        with pytest.raises(NotImplementedError, match='cpu'):
            fn()


class _Loader(list):
    class dataset:
        opt = dict(name='tiny')


def _validation_model(val):
    """nondist_validation on a model object whose forward is replaced by fixed CPU tensors (the constructor needs a GPU)"""
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    m = MultiRefRestorationModel.__new__(MultiRefRestorationModel)
    m.opt = dict(crop_border=4, is_train=False, name='t', path={}, val=val)
    m.is_train = False
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(1, 3, 30, 34, generator=g)
    m.feed_data = lambda data: setattr(m, 'gt', gt)
    m.test = lambda: setattr(m, 'output', (gt + 0.05 * torch.randn(1, 3, 30, 34, generator=g)).clamp(0, 1))
    return m


def test_option_is_parsed_and_the_default_stays_on_numpy():
    from mrefsr_amd import metrics
    from mrefsr_amd.models.multi_ref_restoration_model import RefRestorationModel
    assert _validation_model(None)._metrics_on_device() is False
    assert _validation_model(dict(save_img=False))._metrics_on_device() is False
    assert _validation_model(dict(metrics_on_device=True))._metrics_on_device() is True
    assert RefRestorationModel._metrics_on_device is type(_validation_model(None))._metrics_on_device
    loader = _Loader([{'lq_path': ['a/x.png']}, {'lq_path': ['a/y.png']}])
    res = _validation_model(dict(save_img=False)).nondist_validation(loader, 0, None, False)   # CPU tensors: numpy path
    m = _validation_model(None)
    want = []
    for _ in loader:
        m.feed_data(None)
        m.test()
        a, b = metrics.tensor2img(m.output), metrics.tensor2img(m.gt)
        want.append((metrics.calculate_psnr(a, b, 4), metrics.calculate_psnr(a, b, 4, True), metrics.calculate_ssim(a, b, 4, True)))
    assert res == dict(zip(('psnr', 'psnr_y', 'ssim_y'), (sum(v) / 2 for v in zip(*want))))
    with pytest.raises(NotImplementedError, match='cpu'):                                    # the option asks for the device
        _validation_model(dict(metrics_on_device=True)).nondist_validation(loader, 0, None, False)
