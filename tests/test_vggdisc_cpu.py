"""CPU: VGGStyleDiscriminator's module tree and initialisation against the reference's, its refusals, the model's acceptance of it,
and the build of csrc/disc_vgg.hip.  The GPU side: tests/test_vggdisc_kernels_gpu.py, tests/test_vggdisc_train_gpu.py."""
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import spec_from
from test_losses_cpu import _Bare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAN_TRAIN = dict(gan_type='wgan', gan_weight=1e-3, grad_penalty_weight=10.0, lr_d=1e-4, beta_d=[0.9, 0.999])
NET_D = dict(type='VGGStyleDiscriminator', num_in_ch=3, num_feat=64)


def test_state_dict_is_the_references(golden):
    """keys, shapes and order of VGGStyleDiscriminator(3, 64).state_dict() == the reference's (recorded by gen_golden_gan_vgg.py)"""
    from mrefsr_amd.archs import build_network
    net = build_network(dict(NET_D))
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert got == spec_from(golden('e2e_c2_gan_vgg'), 'net_d_')
    assert got == spec_from(golden('e2e_c2_gan_vgg_vanilla'), 'net_d_')
    names = [n for n, _ in net.named_modules()][1:]
    assert names[:3] == ['conv0_0', 'conv0_1', 'bn0_1'] and names[-3:] == ['linear1', 'linear2', 'lrelu']


def test_default_initialisation_is_the_references_bit_for_bit(golden):
    """under torch.manual_seed(0), every state_dict tensor has the sha256 of the reference module's"""
    from mrefsr_amd.archs.discriminator_arch import VGGStyleDiscriminator
    g = golden('e2e_c2_gan_vgg')
    torch.manual_seed(0)
    net = VGGStyleDiscriminator(3, 64)
    sd = net.state_dict()
    assert list(sd) == [str(n) for n in g['init_names']]
    for (k, v), want in zip(sd.items(), g['init_sha256']):
        assert hashlib.sha256(np.ascontiguousarray(v.numpy()).tobytes()).hexdigest() == str(want), k


def test_refusals():
    from mrefsr_amd.archs import build_network
    from mrefsr_amd.archs.discriminator_arch import VGGStyleDiscriminator
    from mrefsr_amd.archs.nhwc_vggdisc import check_width
    with pytest.raises(TypeError):
        VGGStyleDiscriminator(3)                       # num_in_ch and num_feat are both required, as in the reference
    with pytest.raises(NotImplementedError, match='num_in_ch'):
        VGGStyleDiscriminator(1, 64)
    with pytest.raises(NotImplementedError, match='num_feat'):
        VGGStyleDiscriminator(3, 24)
    with pytest.raises(NotImplementedError, match='linear1'):
        VGGStyleDiscriminator(3, 64, input_size=256)
    with pytest.raises(AssertionError):
        VGGStyleDiscriminator(3, 64, input_size=128)
    net = build_network(dict(NET_D))
    with pytest.raises(NotImplementedError, match='CPU'):
        net(torch.rand(1, 3, 160, 160))
    with pytest.raises(AssertionError):
        net(torch.rand(1, 3, 96, 160))               # H must be input_size (the reference's assert, before anything runs)
    for w in (160, 170, 191):
        check_width(net, w)
    for w in (159, 192, 256):
        with pytest.raises(RuntimeError, match='linear1 expects 12800 input features'):
            check_width(net, w)


def test_model_accepts_vggstyle_and_still_refuses_others():
    from mrefsr_amd.archs.discriminator_arch import VGGStyleDiscriminator
    from mrefsr_amd.losses import GANLoss, GradientPenaltyLoss
    m = _Bare.settings(dict(GAN_TRAIN), network_d=dict(NET_D))
    assert isinstance(m.net_d, VGGStyleDiscriminator) and m.net_d.training
    assert isinstance(m.cri_gan, GANLoss) and m.cri_gan.gan_type == 'wgan' and m.cri_gan.loss_weight == 1e-3
    assert isinstance(m.cri_grad_penalty, GradientPenaltyLoss) and m.cri_grad_penalty.loss_weight == 10.0
    assert m.optimizers == [m.optimizer_d] and len(m.schedulers) == 1 and m.schedulers[0].optimizer is m.optimizer_d
    assert len(m.optimizer_d.param_groups[0]['params']) == len(list(m.net_d.parameters())) == 33
    for other in ('UNetDiscriminatorSN', 'VGGStyleDiscriminator160'):
        with pytest.raises(NotImplementedError, match='network_d'):
            _Bare.settings(dict(GAN_TRAIN), network_d=dict(type=other))


def test_compat_replaces_the_vggstyle_discriminator():
    from mrefsr_amd import compat
    assert 'VGGStyleDiscriminator' in compat._ARCHS and 'ImageDiscriminator' in compat._ARCHS


def test_disc_vgg_kernels_compile_without_scratch(tmp_path):
    """every kernel of csrc/disc_vgg.hip builds for gfx950 with no scratch memory; the convolution kernels use the f32-input MFMA"""
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    asm = str(tmp_path / 'disc_vgg.s')
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-fno-slp-vectorize', '-S',
                    '--cuda-device-only', os.path.join(ROOT, 'mrefsr_amd', 'csrc', 'disc_vgg.hip'), '-o', asm], check=True, capture_output=True)
    text = open(asm).read()
    kernels = re.findall(r'^(_ZN12_GLOBAL__N_1\d+(\w+?_kernel)\w*):', text, flags=re.M)
    names = sorted({k for _, k in kernels})
    for want in ('dconv_pack_weight_kernel', 'dconv_gemm_kernel', 'dconv_finish_kernel', 'dconv_wgrad_finish_kernel', 'lrelu_mask_kernel',
                 'lin_rows_kernel', 'lin_out_kernel', 'lin_gf_kernel', 'lin_params_kernel'):
        assert want in names, (want, names)
    assert sum(name == 'dconv_gemm_kernel' for _, name in kernels) == 6   # KS 3 and 4 x forward, input gradient, weight gradient
    sizes = re.findall(r'; ScratchSize: (\d+)', text)
    assert len(sizes) == len(kernels) and set(sizes) == {'0'}, sizes
    for label, name in kernels:
        body = text.split(label + ':', 1)[1].split('s_endpgm', 1)[0]
        assert ('v_mfma_f32_16x16x4_f32' in body) == (name == 'dconv_gemm_kernel'), label
