"""CPU: the drop-in boundary.  The C-ABI library loads and exports every symbol the header
declares; the product never touches the oracle; the python mirror exposes the reference's names."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, 'include', 'mrefsr_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(mrefsr_[a-z0-9_]+)\s*\(', src)))


def test_library_builds_and_exports_every_header_symbol():
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'mrefsr_amd', 'csrc'), '-s'])
    from mrefsr_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = header_functions()
    assert len(names) >= 27
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/mrefsr_hip.h but not exported'
    # ...and the python binding table covers exactly the header
    assert sorted(_lib.SIGNATURES) == names
    assert _lib.load().mrefsr_abi_version() == 1


def test_product_library_reads_eight_switches_and_carries_no_retired_kernel():
    """the environment variables libmrefsr_hip.so reads are the six the tests flip in one process and the two user-facing arithmetic
    fallbacks; every other kernel-variant switch, and the retired row-stationary pre-filter that MREFSR_CORR_RS_DUP
    selects, exist only in the -DMREFSR_AB_KERNELS build (mrefsr_amd/lib_ab)"""
    csrc = os.path.join(ROOT, 'mrefsr_amd', 'csrc')
    subprocess.check_call(['make', '-C', csrc, '-s'])
    subprocess.check_call(['make', '-C', csrc, '-s', '-j4', 'OBJDIR=_obj_ab', 'OUTDIR=../lib_ab', 'EXTRA=-DMREFSR_AB_KERNELS'])
    kept = {'MREFSR_CORR_W', 'MREFSR_CORR_RESCORE', 'MREFSR_DCN_PT', 'MREFSR_DCN_T', 'MREFSR_CONV1X1', 'MREFSR_WINO_WAVES',
            'MREFSR_DCN_BF16', 'MREFSR_DCN_TERMS'}
    ab_only = {'MREFSR_CONV_XCD', 'MREFSR_CONV_XCD_MIN', 'MREFSR_CONV8', 'MREFSR_CONV_WARM', 'MREFSR_CORR_XCD', 'MREFSR_CORR_RS_DUP',
               'MREFSR_DCN_XCD', 'MREFSR_DCN_MAP8', 'MREFSR_UP_TPB'}

    def env_names(blob):   # a name given to getenv is a whole C string (names inside messages are not)
        return {m.decode() for m in re.findall(rb'(?<=\0)MREFSR_[A-Z0-9_]+(?=\0)', blob)}

    product = open(os.path.join(ROOT, 'mrefsr_amd', 'lib', 'libmrefsr_hip.so'), 'rb').read()
    assert env_names(product) == kept
    assert b'corr_prefilter_rs16_kernel' not in product          # no host stub, no device symbol, no name string
    ab = open(os.path.join(ROOT, 'mrefsr_amd', 'lib_ab', 'libmrefsr_hip.so'), 'rb').read()
    assert env_names(ab) >= kept | ab_only
    assert b'corr_prefilter_rs16_kernel' in ab


def test_no_crossed_packed_fp32_multiply_in_the_device_code(tmp_path):
    """`v_pk_mul_f32 ... op_sel:[0,1] op_sel_hi:[1,0]` (crossed halves, formed by the SLP vectoriser) returned wrong
    values in lanes 48..63 on gfx950 while other workgroups' MFMAs shared the SIMD: the kernels are
    written so that the compiler never forms a packed fp32 instruction with a source-half swizzle of VGPR pairs.
    The built code objects are disassembled and checked."""
    import shutil
    objdump = '/opt/rocm/lib/llvm/bin/llvm-objdump'
    if not os.path.exists(objdump):
        pytest.skip('llvm-objdump not available')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'mrefsr_amd', 'csrc'), '-s'])
    from mrefsr_amd import _lib
    so = shutil.copy(_lib.LIB_PATH, tmp_path / 'lib.so')
    subprocess.run([objdump, '--offloading', os.path.basename(so)], cwd=tmp_path, check=True, capture_output=True)
    images = [f for f in os.listdir(tmp_path) if f.endswith('gfx950')]
    assert images, 'no gfx950 code object found in the library'
    bad, n_mfma = [], 0
    for f in images:
        asm = subprocess.run([objdump, '-d', f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        n_mfma += asm.count('v_mfma_')
        # (one form is admitted: `v_pk_mov_b32 d, a, b op_sel:[1,0]` = {a.hi, b.lo}, which hipcc forms for float2 shuffles in
        #  upfirdn2d_pair_kernel -- it swizzles source 0 only and returns the scalar moves' bits next to bf16 / fp16 MFMAs:
        #  tools/hazard/pk_mul_hazard.hip, profiles/r4_pk_mov_hazard.txt; every failing form takes source 1's HIGH half for the low result)
        bad += [ln.strip() for ln in asm.splitlines() if re.search(r'\bv_pk_\w+\b.*\bop_sel:\[', ln)
                and not re.search(r'\bv_pk_mov_b32\b[^/]*\bop_sel:\[1,0\]\s*(//|$)', ln)]
    assert n_mfma > 1000          # the disassembly really is the kernels
    assert not bad, f'{len(bad)} packed (VOP3P) instructions with swizzled source halves, e.g. {bad[:3]}'


def test_winograd_kernel_hand_waited_loop_is_hazard_free_in_the_built_isa(tmp_path):
    """conv_wino_kernel issues and waits for its loads by hand: the kernel is compiled to assembly with the library's
    flags and tools/asm_inflight_check_wino.py walks the chunk loop of every instantiation twice for both wave groups -- no instruction
    may touch a register with a load in flight under the in-order model, and the waits must be the counted ones (8 / 3), never a drain"""
    import shutil
    import sys
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'mrefsr_amd', 'csrc', 'conv_wino.hip')
    asm = str(tmp_path / 'conv_wino.s')
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-fno-slp-vectorize', '-S',
                    '--cuda-device-only', src, '-o', asm], check=True, capture_output=True)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'asm_inflight_check_wino.py'), asm], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:]
    assert out.stdout.count('in-flight register hazards: 0') == 6, out.stdout          # 3 instantiations x 2 wave groups
    assert '(0, ' not in out.stdout, 'a vmcnt(0) inside the chunk loop:\n' + out.stdout   # waits are (vmcnt, in flight before) pairs


def test_four_wave_winograd_kernel_isa(tmp_path):
    """conv_wino4_kernel (csrc/conv_wino4.hip): patch pieces by hand-waited register loads, weight fragments by LDS-DMA with counted
    waits.  In the built ISA of all sixteen instantiations: (1) on every path of the WHOLE kernel no instruction touches a register with
    a load in flight (the pieces fly across the end of a step; at a tile's end they are handed over before the epilogue); (2) the
    chunk loop's counted waits are 8 / 4 / 4 / 10 of 12 / 8 / 8 / 20 operations in flight, never a drain; (3) no scratch memory (a spill reload is a
    vmcnt(0) and, for a register in flight, a wrong result); (4) M0 -- the LDS base of the DMAs, set once per fragment group -- is
    written by the kernel's own assembly only"""
    import shutil
    import sys
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'mrefsr_amd', 'csrc', 'conv_wino4.hip')
    asm = str(tmp_path / 'conv_wino4.s')
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-fno-slp-vectorize', '-S',
                    '--cuda-device-only', src, '-o', asm], check=True, capture_output=True)
    tool = os.path.join(ROOT, 'tools', 'asm_inflight_check_wino4.py')
    whole = subprocess.run([sys.executable, tool, asm, 'whole'], capture_output=True, text=True)
    assert whole.returncode == 0 and whole.stdout.count('in-flight register hazards: 0') == 16, whole.stdout[-3000:]
    loop = subprocess.run([sys.executable, tool, asm], capture_output=True, text=True)
    assert loop.returncode == 0 and loop.stdout.count('in-flight register hazards: 0') == 16, loop.stdout[-3000:]
    assert loop.stdout.count('(8, 12), (4, 8), (4, 8), (10, 20)') == 16, loop.stdout
    text = open(asm).read()
    assert text.count('; ScratchSize: 0') == 16 and text.count('; ScratchSize:') == 16
    inside, stray = False, []
    for ln in text.splitlines():
        if '#ASMSTART' in ln:
            inside = True
        elif '#ASMEND' in ln:
            inside = False
        elif not inside and re.search(r'\bm0\b', ln.split(';')[0]) and not ln.lstrip().startswith('.'):
            stray.append(ln.strip())
    assert not stray, f'M0 touched outside the kernel\'s own assembly: {stray[:3]}'


def test_conv1x1_kernel_isa(tmp_path):
    """conv1x1_kernel (csrc/conv_nhwc.hip) requests its tiles and weight fragments by hand, two chunks ahead, and waits with counted
    `s_waitcnt vmcnt(N)`.  In the built ISA of both instantiations: no scratch memory; the kernel's own waits are exactly the counted 8 / 12
    / 8 / 12 of the chunk loop and the drain behind it; walked twice under the in-order model, no instruction of the loop touches a register with a
    load in flight (tools/asm_inflight_check.py)"""
    import shutil
    import sys
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'mrefsr_amd', 'csrc', 'conv_nhwc.hip')
    asm = str(tmp_path / 'conv_nhwc.s')
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-fno-slp-vectorize', '-S',
                    '--cuda-device-only', src, '-o', asm], check=True, capture_output=True)
    lines = open(asm).read().split('\n')
    found = 0
    for i, ln in enumerate(lines):
        if not re.match(r'_ZN12_GLOBAL__N_114conv1x1_kernelILb[01]EEEvN11mrefsr_conv8ConvArgsE:', ln):
            continue
        found += 1
        end = next(j for j in range(i, len(lines)) if 's_endpgm' in lines[j])
        # the kernel's own waits (inside #ASMSTART / #ASMEND): the chunk loop's 8 / 12 / 8 / 12 -- unrolled by two, in whatever block order the
        # compiler lays the loop out -- then the drain behind it
        hand = [(j + 1, int(re.search(r'vmcnt\((\d+)\)', lines[j + 1]).group(1))) for j in range(i, end)
                if '#ASMSTART' in lines[j] and 's_waitcnt vmcnt' in lines[j + 1]]
        assert [w for _, w in hand] == [8, 12, 8, 12, 0], hand
        # (the loop's text ends at its last branch: the exit block in front of the drain holds register copies of in-flight fragment
        # registers -- phi moves of values nothing reads, the loads behind them are the clamped re-requests past the last chunk)
        last = max(j for j in range(hand[3][0], hand[4][0]) if re.match(r'\s*s_c?branch', lines[j]))
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'asm_inflight_check.py'), asm, str(hand[0][0] + 1), str(last + 1)],
                             capture_output=True, text=True)
        assert out.returncode == 0 and 'in-flight register hazards: 0' in out.stdout, out.stdout[-2000:]
        size = next(lines[j] for j in range(end, min(end + 3000, len(lines))) if '; ScratchSize:' in lines[j])
        assert size.strip() == '; ScratchSize: 0', size
    assert found == 2


def test_argument_validation_without_gpu():
    """error paths return codes + messages before any launch (safe on a CPU-only host)"""
    from mrefsr_amd import _lib
    lib = _lib.load()
    assert lib.mrefsr_corr_padded_channels(256) == 256
    assert lib.mrefsr_corr_padded_channels(100) == 128
    assert lib.mrefsr_corr_padded_channels(300) < 0 and b'outside' in lib.mrefsr_last_error()
    assert lib.mrefsr_pixnorm_f32(None, None, None, None, 1, 8, 16, 1, 0, 0, None, None) == -1
    assert b'null' in lib.mrefsr_last_error()
    with pytest.raises(_lib.MrefsrHipError):
        _lib.call('mrefsr_patch_norm_f32', ctypes.c_void_p(8), ctypes.c_void_p(8), None, 1, 2, 2, None)  # h, w < 3


def test_product_never_imports_the_oracle():
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, 'mrefsr_amd')):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')) or f == 'Makefile':
                txt = open(os.path.join(base, f)).read()
                code = '\n'.join(ln for ln in txt.splitlines() if not ln.lstrip().startswith(('#', '//', '*', '/*')))
                if (re.search(r'^\s*(from|import)\s+oracle\b', code, flags=re.M)            # python import
                        or re.search(r'#\s*include\s*[<"].*oracle', txt)                      # C include
                        or re.search(r'libmrefsr_oracle|oracle/_build|-lmrefsr_oracle', code)):  # link / dlopen
                    bad.append(os.path.join(base, f))
    assert not bad, f'product code references the oracle: {bad}'
    # and there is no CPU fallback: ops refuse CPU tensors
    import torch
    from mrefsr_amd.ops.dcn import modulated_deform_conv
    from mrefsr_amd.ops.upfirdn2d import upfirdn2d
    with pytest.raises(NotImplementedError):
        modulated_deform_conv(torch.zeros(1, 4, 5, 5), torch.zeros(1, 18, 5, 5), torch.zeros(1, 9, 5, 5), torch.zeros(4, 4, 3, 3))
    # (upfirdn2d on CPU tensors is the one exception, and it is the REFERENCE's: its `upfirdn2d` dispatches CPU tensors to a
    #  plain-torch `upfirdn2d_native`, upfirdn2d.py:153-155, 162-192 -- the mirror ships the same form, pinned below on the
    #  reference's own outputs; nothing of it touches the oracle or the HIP library)
    import numpy as np
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'metrics_ops.npz'), allow_pickle=True)
    for i, (u, d, p0, p1, ks) in enumerate(g['up_cases']):
        x, k = torch.from_numpy(g[f'up_x{i}']), torch.from_numpy(g[f'up_k{i}'])
        np.testing.assert_allclose(upfirdn2d(x, k, up=int(u), down=int(d), pad=(int(p0), int(p1))).numpy(), g[f'up_out{i}'], rtol=0, atol=2e-6)


def test_mirror_exposes_reference_names():
    import mrefsr_amd.ops.dcn as dcn
    assert dcn.__all__ == ['DeformConv', 'DeformConvPack', 'ModulatedDeformConv', 'ModulatedDeformConvPack', 'deform_conv',
                           'modulated_deform_conv']  # basicsr/ops/dcn/__init__.py:4-7
    from mrefsr_amd.ops.fused_act import FusedLeakyReLU, fused_leaky_relu  # noqa: F401
    from mrefsr_amd.ops.upfirdn2d import upfirdn2d  # noqa: F401
    from mrefsr_amd.archs import ARCH_REGISTRY, build_network
    for name in ('MRAPARestorationNet', 'CorrespondenceGenerationArch', 'ContrasMultiExtractorSep', 'VGGFeatureExtractor'):
        assert name in ARCH_REGISTRY
    with pytest.raises(KeyError):
        build_network(dict(type='NoSuchNet'))
    from mrefsr_amd.models import MODEL_REGISTRY
    assert 'MultiRefRestorationModel' in MODEL_REGISTRY
    # state-dict compatibility of the restoration net: 23,711,633 parameters
    net = build_network(dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8))
    assert sum(p.numel() for p in net.parameters()) == 23711633


def test_state_dict_keys_match_reference(golden):
    from conftest import spec_from
    from mrefsr_amd.archs import build_network
    g = golden('e2e')
    nets = dict(net_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8),
                net_extractor=dict(type='ContrasMultiExtractorSep'),
                net_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1,
                             vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'], vgg_type='vgg19'))
    for name, opt in nets.items():
        mine = [(k, tuple(v.shape)) for k, v in build_network(opt).state_dict().items()]
        assert mine == spec_from(g, name + '_'), name  # same keys, same shapes, same order


_HOST_ARCHS = ('MRAPARestorationNet', 'RestorationNet', 'CorrespondenceGenerationArch', 'ContrasMultiExtractorSep',
               'ContrasExtractorSep', 'VGGFeatureExtractor')
_HOST_MODELS = ('MultiRefRestorationModel', 'RefRestorationModel')


@pytest.fixture
def host_basicsr():
    """a stand-in for the ``basicsr`` package compat installs into (the reference's; not part of this repository): its two
    registries with the reference's lookup contract (mrefsr_amd/utils/registry.py restates it), every slot compat replaces
    already taken -- the host's arch / model modules register their classes at import --, no mmcv; sys.modules restored after"""
    import sys
    import types
    from mrefsr_amd.utils.registry import Registry

    def host_keys():
        return [k for k in sys.modules if k.split('.')[0] in ('basicsr', 'mmcv')]
    saved = {k: sys.modules.pop(k) for k in host_keys()}
    reg = types.ModuleType('basicsr.utils.registry')
    reg.ARCH_REGISTRY, reg.MODEL_REGISTRY = Registry('arch'), Registry('model')
    for registry, names in ((reg.ARCH_REGISTRY, _HOST_ARCHS), (reg.MODEL_REGISTRY, _HOST_MODELS)):
        for name in names:
            registry.register(type(name, (), {}))
    for name in ('basicsr', 'basicsr.utils', 'basicsr.ops'):
        sys.modules[name] = types.ModuleType(name)
        sys.modules[name].__path__ = []
    sys.modules['basicsr.utils.registry'] = reg
    try:
        yield reg
    finally:
        for k in host_keys():
            del sys.modules[k]
        sys.modules.update(saved)


def test_compat_installs_into_reference_registries(host_basicsr):
    """our classes replace the registry slots train.py / test.py resolve by name"""
    import mrefsr_amd.compat as compat
    from mrefsr_amd.archs import ARCH_REGISTRY
    from mrefsr_amd.archs.ref_mrapa_restoration_arch import MRAPARestorationNet
    from mrefsr_amd.models import MODEL_REGISTRY
    assert compat.install_into_basicsr(ops=False, mmcv=False)
    REF = host_basicsr.ARCH_REGISTRY
    assert REF.get('MRAPARestorationNet') is MRAPARestorationNet
    for name in _HOST_ARCHS:
        assert REF.get(name) is ARCH_REGISTRY.get(name), name
    for name in _HOST_MODELS:
        assert host_basicsr.MODEL_REGISTRY.get(name) is MODEL_REGISTRY.get(name), name
    net = REF.get('MRAPARestorationNet')(ngf=64, n_blocks=16, groups=8)   # what the host's build_network does with the type name
    assert isinstance(net, MRAPARestorationNet)


def test_compat_mmcv_shim_builds_the_reference_dynagg(host_basicsr):
    """install_into_basicsr(ops=True, mmcv=True): the import the reference's arch files make (``from mmcv.ops import
    ModulatedDeformConv2d, modulated_deform_conv2d``) resolves to the shim, and a DynAgg-style subclass (mmcv's DCNv2 pack
    pattern: the super().__init__ signature, a zero-initialised conv_offset_mask sized from deform_groups and kernel_size)
    constructs on it and finds every attribute it reads; basicsr.ops.* are the mrefsr_amd modules"""
    import sys
    from torch import nn
    import mrefsr_amd.compat as compat
    assert compat.install_into_basicsr(models=False, ops=True, mmcv=True)
    from mmcv.ops import ModulatedDeformConv2d, modulated_deform_conv2d
    assert ModulatedDeformConv2d is compat.ModulatedDeformConv2d and modulated_deform_conv2d is compat.modulated_deform_conv2d

    class DynAgg(ModulatedDeformConv2d):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deform_groups=1):
            super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, deform_groups)
            self.conv_offset_mask = nn.Conv2d(self.in_channels, self.deform_groups * 3 * self.kernel_size[0] * self.kernel_size[1],
                                              kernel_size=self.kernel_size, stride=self.stride, padding=self.padding,
                                              dilation=self.dilation, bias=True)
            self.conv_offset_mask.weight.data.zero_()
            self.conv_offset_mask.bias.data.zero_()

    agg = DynAgg(64, 64, 3, stride=1, padding=1, dilation=1, deform_groups=8)
    assert isinstance(agg, compat.ModulatedDeformConv2d) and agg.deform_groups == 8 and agg.groups == 1
    assert tuple(agg.conv_offset_mask.weight.shape) == (216, 64, 3, 3) and float(agg.conv_offset_mask.weight.detach().abs().sum()) == 0.0
    assert tuple(agg.weight.shape) == (64, 64, 3, 3) and agg.bias is not None
    import mrefsr_amd.ops.dcn.deform_conv_ext as ext
    from mrefsr_amd.ops import dcn, fused_act, upfirdn2d
    assert sys.modules['basicsr.ops.dcn.deform_conv_ext'] is ext and sys.modules['basicsr.ops.dcn'] is dcn
    assert sys.modules['basicsr.ops.fused_act'] is fused_act and sys.modules['basicsr.ops.upfirdn2d'] is upfirdn2d
    for name in ('deform_conv_forward', 'deform_conv_backward_input', 'deform_conv_backward_parameters',
                 'modulated_deform_conv_forward', 'modulated_deform_conv_backward'):   # deform_conv_ext.cpp:150-164
        assert callable(getattr(ext, name))


def test_sample_patches_is_the_reference_unfold():
    """ref_map_util.sample_patches (ref_map_util.py:4-23; API parity, the path reads its 3x3 windows in place): (c,h,w) ->
    (c, p, p, n) with the patches row-major, against explicit slicing, for the path's patch size / stride and a general one"""
    import torch
    from mrefsr_amd.archs.ref_map_util import sample_patches
    x = torch.arange(2 * 7 * 9, dtype=torch.float32).reshape(2, 7, 9)
    for p, st in ((3, 1), (2, 2), (3, 2)):
        got = sample_patches(x, p, st)
        ny, nx = (7 - p) // st + 1, (9 - p) // st + 1
        assert tuple(got.shape) == (2, p, p, ny * nx)
        for n, (iy, ix) in enumerate((iy, ix) for iy in range(ny) for ix in range(nx)):
            assert torch.equal(got[..., n], x[:, iy * st:iy * st + p, ix * st:ix * st + p])


def test_ssim_matches_an_independent_restatement():
    """calculate_ssim (psnr_ssim.py:85-129, :172-200; the reference needs cv2 for it) against scipy: the 11-tap sigma 1.5
    Gaussian of cv2.getGaussianKernel and 'valid' 2-D correlation"""
    import numpy as np
    from scipy import ndimage
    from mrefsr_amd.metrics import _gaussian_window, calculate_ssim, rgb_to_y
    k = _gaussian_window()
    np.testing.assert_allclose(k[:6], [0.00102838, 0.00759876, 0.03600077, 0.10936069, 0.21300554, 0.26601172], atol=5e-9)
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (40, 52, 3)).astype(np.uint8)
    b = np.clip(a.astype(int) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)

    def ssim_ref(x, y):
        w = np.outer(k, k)
        f = lambda z: ndimage.correlate(z, w, mode='reflect')[5:-5, 5:-5]   # noqa: E731
        c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
        m1, m2 = f(x), f(y)
        s1, s2, s12 = f(x * x) - m1 * m1, f(y * y) - m2 * m2, f(x * y) - m1 * m2
        return (((2 * m1 * m2 + c1) * (2 * s12 + c2)) / ((m1 * m1 + m2 * m2 + c1) * (s1 + s2 + c2))).mean()
    for cb in (0, 4):
        ya, yb = rgb_to_y(a).astype(np.float64)[..., 0], rgb_to_y(b).astype(np.float64)[..., 0]
        if cb:
            ya, yb = ya[cb:-cb, cb:-cb], yb[cb:-cb, cb:-cb]
        assert abs(calculate_ssim(a, b, crop_border=cb, test_y_channel=True) - ssim_ref(ya, yb)) < 1e-10
    assert abs(calculate_ssim(a, a, crop_border=0) - 1.0) < 1e-12


def test_wgrad_workspace_plan_is_host_arithmetic():
    """the weight-gradient launch plan (rows per block against CU rounds) is pure host arithmetic: sizes are positive, a batch of
    jobs needs no more partial sums per job than a single launch, and nonsense shapes are refused"""
    from mrefsr_amd import _lib
    lib = _lib.load()
    one = lib.mrefsr_conv_wgrad3x3_workspace_bytes(4, 160, 160, 64, 64)
    assert one > 0 and one % (9 * 4096 * 4) == 0
    assert lib.mrefsr_conv_wgrad3x3_batch_workspace_bytes(1, 4, 160, 160, 64, 64) == one
    for n, h in ((4, 40), (4, 80), (4, 160), (20, 160)):
        single = lib.mrefsr_conv_wgrad3x3_workspace_bytes(n, h, h, 64, 64)
        batch = lib.mrefsr_conv_wgrad3x3_batch_workspace_bytes(32, n, h, h, 64, 64)
        assert 0 < batch <= 32 * single, (n, h, single, batch)
    assert lib.mrefsr_conv_wgrad3x3_batch_workspace_bytes(33, 4, 40, 40, 64, 64) == -1
    assert lib.mrefsr_conv_wgrad3x3_batch_workspace_bytes(0, 4, 40, 40, 64, 64) == -1
    assert lib.mrefsr_conv_wgrad3x3_workspace_bytes(0, 40, 40, 64, 64) == -1


def test_basicsr_jit_builds_the_library_before_loading_it(monkeypatch):
    """BASICSR_JIT=True (basicsr/ops/dcn/deform_conv.py:10-21 and the two sibling ops: a run-time build of the extension at import)
    runs the library's Makefile -- incremental -- before the first dlopen; without the variable nothing is built at load time; an
    explicit MREFSR_HIP_LIB is loaded as it is"""
    import subprocess
    from mrefsr_amd import _lib
    calls = []
    monkeypatch.setattr(subprocess, 'check_call', lambda cmd, **kw: calls.append(cmd) or 0)
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.delenv('BASICSR_JIT', raising=False)
    monkeypatch.delenv('MREFSR_HIP_LIB', raising=False)
    _lib.load()
    assert not calls
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setenv('BASICSR_JIT', 'True')
    lib = _lib.load()
    assert len(calls) == 1 and calls[0][:2] == ['make', '-C'] and calls[0][2].endswith(os.path.join('mrefsr_amd', 'csrc'))
    assert lib.mrefsr_abi_version() == _lib.ABI_VERSION
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setenv('MREFSR_HIP_LIB', _lib.LIB_PATH)
    _lib.load()
    assert len(calls) == 1
