"""CPU: StyleGAN2Discriminator's module tree and initialisation against the reference's, its registry key and refusals, the model's
acceptance of it, and the build of csrc/disc_sg2.hip.  The GPU side: tests/test_sg2disc_kernels_gpu.py,
tests/test_sg2disc_train_gpu.py."""
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import synth_sg2disc
from conftest import spec_from
from test_losses_cpu import _Bare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAN_TRAIN = dict(gan_type='wgan', gan_weight=1e-3, grad_penalty_weight=10.0, lr_d=1e-4, beta_d=[0.9, 0.999])
NET_D = dict(type='StyleGAN2Discriminator', out_size=128)


def expected_spec(out_size, channel_multiplier=2, narrow=1):
    """the reference's state_dict layout, written out from stylegan2_arch.py:748-779"""
    ch = {4: int(512 * narrow), 8: int(512 * narrow), 16: int(512 * narrow), 32: int(512 * narrow),
          64: int(256 * channel_multiplier * narrow), 128: int(128 * channel_multiplier * narrow),
          256: int(64 * channel_multiplier * narrow), 512: int(32 * channel_multiplier * narrow), 1024: int(16 * channel_multiplier * narrow)}
    c = ch[out_size]
    spec = [('conv_body.0.0.weight', (c, 3, 1, 1)), ('conv_body.0.1.bias', (c, ))]
    size, n = out_size, 1
    while size > 4:
        co = ch[size // 2]
        spec += [(f'conv_body.{n}.conv1.0.weight', (c, c, 3, 3)), (f'conv_body.{n}.conv1.1.bias', (c, )),
                 (f'conv_body.{n}.conv2.1.weight', (co, c, 3, 3)), (f'conv_body.{n}.conv2.2.bias', (co, )),
                 (f'conv_body.{n}.skip.1.weight', (co, c, 1, 1))]
        c, size, n = co, size // 2, n + 1
    spec += [('final_conv.0.weight', (ch[4], c + 1, 3, 3)), ('final_conv.1.bias', (ch[4], )),
             ('final_linear.0.weight', (ch[4], ch[4] * 16)), ('final_linear.0.bias', (ch[4], )),
             ('final_linear.1.weight', (1, ch[4])), ('final_linear.1.bias', (1, ))]
    return spec


def test_registered():
    from mrefsr_amd.archs import ARCH_REGISTRY, build_network
    from mrefsr_amd.archs.discriminator_arch import StyleGAN2Discriminator
    assert 'StyleGAN2Discriminator' in ARCH_REGISTRY
    assert ARCH_REGISTRY.get('StyleGAN2Discriminator') is StyleGAN2Discriminator
    assert isinstance(build_network(dict(type='StyleGAN2Discriminator', out_size=8)), StyleGAN2Discriminator)


def test_state_dict_is_the_references(golden):
    """keys, shapes and order of StyleGAN2Discriminator(128).state_dict() == the reference's (recorded by gen_golden_gan_sg2.py); the FIR
    is no buffer; other sizes follow the reference's channel table"""
    from mrefsr_amd.archs import build_network
    net = build_network(dict(NET_D))
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert got == spec_from(golden('e2e_c2_gan_sg2'), 'net_d_')
    assert got == spec_from(golden('e2e_c2_gan_sg2_vanilla'), 'net_d_')
    assert got == expected_spec(128)
    assert len(got) == 2 + 5 * 5 + 6 and not list(net.buffers())
    assert got[-6] == ('final_conv.0.weight', (512, 513, 3, 3))
    for kw in (dict(out_size=64, narrow=0.5), dict(out_size=256, channel_multiplier=1), dict(out_size=8), dict(out_size=1024, narrow=0.5)):
        net = build_network(dict(type='StyleGAN2Discriminator', **kw))
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == expected_spec(**kw), kw


def test_default_initialisation_is_the_references_bit_for_bit(golden):
    """under torch.manual_seed(0), every state_dict tensor has the sha256 of the reference module's"""
    from mrefsr_amd.archs.discriminator_arch import StyleGAN2Discriminator
    g = golden('e2e_c2_gan_sg2')
    torch.manual_seed(0)
    sd = StyleGAN2Discriminator(128).state_dict()
    assert list(sd) == [str(n) for n in g['init_names']]
    for (k, v), want in zip(sd.items(), g['init_sha256']):
        assert hashlib.sha256(np.ascontiguousarray(v.numpy()).tobytes()).hexdigest() == str(want), k


def test_reference_format_checkpoint_loads_strictly(golden, tmp_path):
    from mrefsr_amd.archs import build_network
    spec = spec_from(golden('e2e_c2_gan_sg2'), 'net_d_')
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_sg2disc.state_dict(spec).items()}
    path = str(tmp_path / 'net_d.pth')
    torch.save({'params': sd}, path)
    net = build_network(dict(NET_D))
    net.load_state_dict(torch.load(path, map_location='cpu')['params'], strict=True)
    assert list(net.state_dict()) == list(sd)
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_scales_are_the_equalised_learning_rates():
    from mrefsr_amd.archs.discriminator_arch import StyleGAN2Discriminator
    net = StyleGAN2Discriminator(16, narrow=0.125)   # 64 channels
    assert net.conv_body[0][0].scale == 1 / np.sqrt(3)
    b = net.conv_body[1]
    assert b.conv1[0].scale == 1 / np.sqrt(64 * 9) and b.conv2[1].scale == 1 / np.sqrt(64 * 9) and b.skip[1].scale == 1 / np.sqrt(64)
    assert b.conv2[0].pad == (2, 2) and b.skip[0].pad == (1, 1) and b.conv2[1].stride == 2 and b.conv2[1].padding == 0
    assert b.skip[1].bias is None and len(b.skip) == 2
    assert net.final_conv[0].scale == 1 / np.sqrt(65 * 9)
    assert net.final_linear[0].scale == 1 / np.sqrt(64 * 16) and net.final_linear[1].scale == 1 / np.sqrt(64)
    assert net.resample_taps == (0.125, 0.375, 0.375, 0.125)


def test_refusals():
    from mrefsr_amd.archs.discriminator_arch import StyleGAN2Discriminator
    from mrefsr_amd.archs.nhwc_sg2disc import check_input
    with pytest.raises(TypeError):
        StyleGAN2Discriminator()                         # out_size is required, as in the reference
    for size in (4, 48, 100, 2048, 0):
        with pytest.raises(NotImplementedError, match='out_size'):
            StyleGAN2Discriminator(size)
    with pytest.raises(NotImplementedError, match='multiple of 16'):
        StyleGAN2Discriminator(64, narrow=0.01)
    with pytest.raises(NotImplementedError, match='multiple of 16'):
        StyleGAN2Discriminator(1024, channel_multiplier=1, narrow=0.5)   # 8 channels at 1024
    for k in ((1, ), (1, 2, 3, 2, 1), ((1, 1), (1, 1))):
        with pytest.raises(NotImplementedError, match='resample_kernel'):
            StyleGAN2Discriminator(16, resample_kernel=k)
    StyleGAN2Discriminator(16, resample_kernel=(1, 2, 1), narrow=0.125)
    StyleGAN2Discriminator(16, resample_kernel=[1, 1], narrow=0.125)
    net = StyleGAN2Discriminator(32, narrow=0.125)
    with pytest.raises(NotImplementedError, match='CPU'):
        net(torch.rand(4, 3, 32, 32))
    # what forward checks on a GPU tensor before the first launch
    assert check_input(net, torch.empty(4, 3, 32, 32)) == 4 and check_input(net, torch.empty(2, 3, 32, 32)) == 2
    assert check_input(net, torch.empty(8, 3, 32, 32)) == 4
    for shape in ((4, 3, 64, 64), (4, 3, 32, 48), (4, 3, 16, 16)):
        with pytest.raises(RuntimeError, match='final_linear'):
            check_input(net, torch.empty(shape))
    with pytest.raises(RuntimeError, match='not divisible'):
        check_input(net, torch.empty(6, 3, 32, 32))


def test_model_accepts_stylegan2_discriminator():
    from mrefsr_amd.archs.discriminator_arch import StyleGAN2Discriminator
    from mrefsr_amd.losses import GANLoss, GradientPenaltyLoss
    m = _Bare.settings(dict(GAN_TRAIN), network_d=dict(type='StyleGAN2Discriminator', out_size=32, narrow=0.125))
    assert isinstance(m.net_d, StyleGAN2Discriminator) and m.net_d.training and m.net_d.out_size == 32
    assert isinstance(m.cri_gan, GANLoss) and isinstance(m.cri_grad_penalty, GradientPenaltyLoss)
    assert m.optimizers == [m.optimizer_d] and len(m.schedulers) == 1
    assert len(m.optimizer_d.param_groups[0]['params']) == len(list(m.net_d.parameters())) == 2 + 3 * 5 + 6
    with pytest.raises(NotImplementedError, match='StyleGAN2Discriminator are'):
        _Bare.settings(dict(GAN_TRAIN), network_d=dict(type='StyleGAN2Generator', out_size=32))


def test_compat_replaces_the_stylegan2_discriminator():
    from mrefsr_amd import compat
    from mrefsr_amd.archs import ARCH_REGISTRY
    assert 'StyleGAN2Discriminator' in compat._ARCHS
    assert ARCH_REGISTRY.get('StyleGAN2Discriminator').__module__ == 'mrefsr_amd.archs.discriminator_arch'


def test_disc_sg2_kernels_compile_without_scratch(tmp_path):
    """every kernel of csrc/disc_sg2.hip builds for gfx950 with no scratch memory and no float atomics"""
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    asm = str(tmp_path / 'disc_sg2.s')
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-fno-slp-vectorize', '-S',
                    '--cuda-device-only', os.path.join(ROOT, 'mrefsr_amd', 'csrc', 'disc_sg2.hip'), '-o', asm], check=True, capture_output=True)
    text = open(asm).read()
    kernels = re.findall(r'^(_ZN12_GLOBAL__N_1\d+(\w+?_kernel)\w*):', text, flags=re.M)
    names = sorted({k for _, k in kernels})
    assert names == sorted(['sg2_fir_kernel', 'dconv_pack_weight_kernel', 'dconv_gemm_kernel', 'dconv_finish_kernel',
                            'dconv_wgrad_finish_kernel']), names
    assert len(kernels) == 2 + 1 + 6 + 2
    sizes = re.findall(r'; ScratchSize: (\d+)', text)
    assert len(sizes) == len(kernels) and set(sizes) == {'0'}, sizes
    assert not re.search(r'(global|buffer|flat)_atomic_(add|pk_add)_f32', text)
    assert text.count('v_mfma_f32_16x16x4_f32') >= 6 * 16
