"""CPU: UNetDiscriminatorSN's module tree, spectral norms and initialisation against the reference's, its registry keys and
refusals, the model's acceptance of it, and the build of csrc/disc_unet.hip.  The GPU side: tests/test_unetdisc_kernels_gpu.py,
tests/test_unetdisc_train_gpu.py."""
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import synth_unetdisc
from conftest import spec_from
from test_losses_cpu import _Bare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAN_TRAIN = dict(gan_type='wgan', gan_weight=1e-3, grad_penalty_weight=10.0, lr_d=1e-4, beta_d=[0.9, 0.999])
NET_D = dict(type='UNetDiscriminatorSN', num_in_ch=3, num_feat=64, skip_connection=True)


def test_state_dict_is_the_references(golden):
    """keys, shapes and order of UNetDiscriminatorSN(3, 64).state_dict() == the reference's (recorded by gen_golden_gan_unet.py)"""
    from mrefsr_amd.archs import build_network
    net = build_network(dict(NET_D))
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert got == spec_from(golden('e2e_c2_gan_unet'), 'net_d_')
    assert got == spec_from(golden('e2e_c2_gan_unet_vanilla'), 'net_d_')
    keys = [k for k, _ in got]
    assert keys[:2] == ['conv0.weight', 'conv0.bias'] and keys[-2:] == ['conv9.weight', 'conv9.bias']
    for i in range(1, 9):
        assert [k for k in keys if k.startswith(f'conv{i}.')] == [f'conv{i}.weight_orig', f'conv{i}.weight_u', f'conv{i}.weight_v']


def test_default_initialisation_is_the_references_bit_for_bit(golden):
    """under torch.manual_seed(0), every state_dict tensor (u and v included) has the sha256 of the reference module's"""
    from mrefsr_amd.archs.discriminator_arch import UNetDiscriminatorSN
    g = golden('e2e_c2_gan_unet')
    torch.manual_seed(0)
    sd = UNetDiscriminatorSN(3, 64).state_dict()
    assert list(sd) == [str(n) for n in g['init_names']]
    for (k, v), want in zip(sd.items(), g['init_sha256']):
        assert hashlib.sha256(np.ascontiguousarray(v.numpy()).tobytes()).hexdigest() == str(want), k


def test_reference_format_checkpoint_loads_strictly(golden, tmp_path):
    """a {'params': state_dict} file in the reference's layout (weight_orig / weight_u / weight_v) loads with strict=True, through
    torch's spectral-norm load hooks, and leaves every tensor as saved"""
    from mrefsr_amd.archs import build_network
    spec = spec_from(golden('e2e_c2_gan_unet'), 'net_d_')
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_unetdisc.state_dict(spec).items()}
    path = str(tmp_path / 'net_d.pth')
    torch.save({'params': sd}, path)
    net = build_network(dict(NET_D))
    net.load_state_dict(torch.load(path, map_location='cpu')['params'], strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    for i in range(1, 9):
        assert abs(float(sd[f'conv{i}.weight_u'].double().norm()) - 1) < 1e-6


def test_registry_keys():
    from mrefsr_amd.archs import ARCH_REGISTRY, build_network
    from mrefsr_amd.archs.discriminator_arch import UNetDiscriminatorSN
    assert 'UNetDiscriminatorSN_basicsr' in ARCH_REGISTRY and 'UNetDiscriminatorSN' not in ARCH_REGISTRY
    assert ARCH_REGISTRY.get('UNetDiscriminatorSN') is UNetDiscriminatorSN
    assert ARCH_REGISTRY.get('UNetDiscriminatorSN_basicsr') is UNetDiscriminatorSN
    for t in ('UNetDiscriminatorSN', 'UNetDiscriminatorSN_basicsr'):
        assert isinstance(build_network(dict(NET_D, type=t)), UNetDiscriminatorSN)


def test_refusals():
    from mrefsr_amd.archs.discriminator_arch import UNetDiscriminatorSN
    from mrefsr_amd.archs.nhwc_unetdisc import check_size
    with pytest.raises(TypeError):
        UNetDiscriminatorSN()                         # num_in_ch is required, as in the reference
    with pytest.raises(NotImplementedError, match='num_in_ch'):
        UNetDiscriminatorSN(1)
    with pytest.raises(NotImplementedError, match='num_feat'):
        UNetDiscriminatorSN(3, 24)
    net = UNetDiscriminatorSN(3, 32)
    with pytest.raises(NotImplementedError, match='CPU'):
        net(torch.rand(1, 3, 32, 32))
    for h, w in ((160, 160), (160, 192), (16, 24), (8, 8)):
        check_size(net, h, w)
    # the shipped Real-ESRGAN config's gt_size 300: 150 -> 75 -> 37, up(37) = 74 against 75
    with pytest.raises(RuntimeError, match=r'skip add x4 \+ x2'):
        check_size(net, 300, 300)
    with pytest.raises(RuntimeError, match=r'skip add x5 \+ x1'):
        check_size(net, 162, 160)
    with pytest.raises(RuntimeError, match=r'skip add x6 \+ x0'):
        check_size(net, 160, 161)
    net = UNetDiscriminatorSN(3, 32, skip_connection=False)
    for h, w in ((300, 300), (162, 160), (160, 161)):
        with pytest.raises(NotImplementedError, match='multiples of 8'):
            check_size(net, h, w)
    # a spectral norm other than the reference's
    net = UNetDiscriminatorSN(3, 32)
    net.sn_hooks()
    next(h for h in net.conv4._forward_pre_hooks.values() if hasattr(h, 'n_power_iterations')).n_power_iterations = 2
    with pytest.raises(NotImplementedError, match='n_power_iterations=2'):
        net.sn_hooks()
    net = UNetDiscriminatorSN(3, 32)
    torch.nn.utils.remove_spectral_norm(net.conv7)
    with pytest.raises(NotImplementedError, match='conv7 has no spectral norm'):
        net.sn_hooks()
    net = UNetDiscriminatorSN(3, 32)
    net.conv2 = torch.nn.utils.spectral_norm(torch.nn.utils.remove_spectral_norm(net.conv2), dim=1)
    with pytest.raises(NotImplementedError, match='dim=1'):
        net.sn_hooks()


def test_model_accepts_unet_discriminator():
    from mrefsr_amd.archs.discriminator_arch import UNetDiscriminatorSN
    from mrefsr_amd.losses import GANLoss, GradientPenaltyLoss
    for t in ('UNetDiscriminatorSN', 'UNetDiscriminatorSN_basicsr'):
        m = _Bare.settings(dict(GAN_TRAIN), network_d=dict(NET_D, type=t))
        assert isinstance(m.net_d, UNetDiscriminatorSN) and m.net_d.training and m.net_d.skip_connection
        assert isinstance(m.cri_gan, GANLoss) and isinstance(m.cri_grad_penalty, GradientPenaltyLoss)
        assert m.optimizers == [m.optimizer_d] and len(m.schedulers) == 1
        assert len(m.optimizer_d.param_groups[0]['params']) == len(list(m.net_d.parameters())) == 12
    m = _Bare.settings(dict(GAN_TRAIN), network_d=dict(type='UNetDiscriminatorSN', num_in_ch=3, num_feat=32, skip_connection=False))
    assert not m.net_d.skip_connection and m.net_d.conv9.in_channels == 32
    for net_d in (dict(type='UNetDiscriminatorSN'), dict(type='UNetDiscriminatorSN_basicsr', num_feat=64)):
        with pytest.raises(NotImplementedError, match='network_d.*num_in_ch'):
            _Bare.settings(dict(GAN_TRAIN), network_d=net_d)


def test_compat_replaces_the_unet_discriminator():
    from mrefsr_amd import compat
    from mrefsr_amd.archs import ARCH_REGISTRY
    assert 'UNetDiscriminatorSN_basicsr' in compat._ARCHS
    assert ARCH_REGISTRY.get('UNetDiscriminatorSN_basicsr').__module__ == 'mrefsr_amd.archs.discriminator_arch'


def test_disc_unet_kernels_compile_without_scratch(tmp_path):
    """every kernel of csrc/disc_unet.hip builds for gfx950 with no scratch memory and no float atomics"""
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    asm = str(tmp_path / 'disc_unet.s')
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-fno-slp-vectorize', '-S',
                    '--cuda-device-only', os.path.join(ROOT, 'mrefsr_amd', 'csrc', 'disc_unet.hip'), '-o', asm], check=True, capture_output=True)
    text = open(asm).read()
    kernels = re.findall(r'^(_ZN12_GLOBAL__N_1\d+(\w+?_kernel)\w*):', text, flags=re.M)
    names = sorted({k for _, k in kernels})
    assert names == sorted(['sn_wtu_kernel', 'sn_v_kernel', 'sn_wv_kernel', 'sn_u_kernel', 'sn_scale_kernel', 'sn_dot_kernel', 'sn_bwd_kernel',
                            'up2_kernel', 'up2_adj_kernel', 'add_kernel', 'conv9_fwd_kernel', 'conv9_dgrad_kernel', 'conv9_wgrad_kernel',
                            'conv9_wgrad_finish_kernel']), names
    sizes = re.findall(r'; ScratchSize: (\d+)', text)
    assert len(sizes) == len(kernels) and set(sizes) == {'0'}, sizes
    assert not re.search(r'(global|buffer|flat)_atomic_(add|pk_add)_f32', text)
