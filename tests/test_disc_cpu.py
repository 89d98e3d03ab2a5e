"""CPU: ImageDiscriminator's module tree, the GAN losses, the model's adversarial options, and the build of csrc/disc.hip.
The GPU side: tests/test_disc_kernels_gpu.py, tests/test_disc_train_gpu.py."""
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import spec_from
from test_losses_cpu import _Bare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAN_TRAIN = dict(gan_type='wgan', gan_weight=1e-3, grad_penalty_weight=10.0, lr_d=1e-4, beta_d=[0.9, 0.999])


def test_state_dict_is_the_references(golden):
    """keys, shapes and order of ImageDiscriminator(3, 32).state_dict() == the reference's (recorded by gen_golden_gan.py)"""
    from mrefsr_amd.archs import build_network
    net = build_network(dict(type='ImageDiscriminator', in_nc=3, ndf=32))
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert len(got) == 74
    assert got == spec_from(golden('e2e_c2_gan'), 'net_d_')


def test_init_and_refusals():
    from mrefsr_amd.archs import build_network
    torch.manual_seed(0)
    net = build_network(dict(type='ImageDiscriminator'))
    bn = net.conv_block3[1]
    assert abs(float(bn.weight.detach().mean()) - 1.0) < 0.01 and float(bn.bias.detach().abs().max()) == 0.0    # srntt_init_weights: BN N(1, 0.02)
    assert abs(float(net.conv_block3[0].weight.detach().std()) - 0.02) < 0.002 and float(net.conv_block3[0].bias.detach().abs().max()) == 0.0
    with pytest.raises(NotImplementedError, match='in_nc'):
        build_network(dict(type='ImageDiscriminator', in_nc=1))
    with pytest.raises(NotImplementedError, match='ndf'):
        build_network(dict(type='ImageDiscriminator', ndf=24))
    with pytest.raises(NotImplementedError, match='CPU'):
        net(torch.rand(1, 3, 32, 32))


@pytest.mark.parametrize('gan_type', ['vanilla', 'lsgan', 'wgan', 'hinge'])
@pytest.mark.parametrize('is_disc', [True, False])
def test_gan_loss_values(gan_type, is_disc):
    """basicsr/models/losses.py:275-356, written out"""
    from mrefsr_amd.losses import GANLoss
    x = torch.rand(4, 1, 1, 1, dtype=torch.float64)
    crit = GANLoss(gan_type, real_label_val=0.9, fake_label_val=0.1, loss_weight=3.0)
    w = 1.0 if is_disc else 3.0
    for real in (True, False):
        label = torch.full_like(x, 0.9 if real else 0.1)
        if gan_type == 'vanilla':
            want = F.binary_cross_entropy_with_logits(x, label)
        elif gan_type == 'lsgan':
            want = ((x - label)**2).mean()
        elif gan_type == 'wgan':
            want = -x.mean() if real else x.mean()
        elif is_disc:
            want = F.relu(1 - x).mean() if real else F.relu(1 + x).mean()
        else:
            want = -x.mean()
        assert torch.allclose(crit(x, real, is_disc=is_disc), want * w, rtol=1e-12, atol=0), (real, )
    with pytest.raises(NotImplementedError):
        GANLoss('wgan-gp')


def test_loss_registry_and_penalty_signature():
    import inspect
    from mrefsr_amd.losses import LOSS_REGISTRY, GradientPenaltyLoss, build_loss, gradient_penalty_loss
    assert 'GANLoss' in LOSS_REGISTRY and 'GradientPenaltyLoss' in LOSS_REGISTRY
    assert build_loss(dict(type='GradientPenaltyLoss', loss_weight=10.0)).loss_weight == 10.0
    assert list(inspect.signature(gradient_penalty_loss).parameters) == ['discriminator', 'real_data', 'fake_data', 'mask']
    assert list(inspect.signature(GradientPenaltyLoss.forward).parameters) == ['self', 'discriminator', 'real_data', 'fake_data', 'mask']


def test_gradient_penalty_formula_on_a_cpu_discriminator():
    """gradient_penalty_loss with a plain differentiable torch module (twice differentiable, CPU): the reference's value"""
    from mrefsr_amd.losses import gradient_penalty_loss
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.Tanh(), torch.nn.AdaptiveAvgPool2d(1))
    real, fake = torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8)
    torch.manual_seed(5)
    got = gradient_penalty_loss(net, real, fake)
    torch.manual_seed(5)
    alpha = torch.rand(2, 1, 1, 1)
    xi = (alpha * real + (1 - alpha) * fake).requires_grad_(True)
    d = net(xi)
    gi, = torch.autograd.grad(d, xi, torch.ones_like(d), create_graph=True)
    assert torch.equal(got, ((gi.view(2, -1).norm(2, dim=1) - 1)**2).mean())


def test_model_refuses_what_the_reference_cannot_run():
    with pytest.raises(NotImplementedError, match='network_d'):
        _Bare.settings(dict(GAN_TRAIN), network_d=dict(type='UNetDiscriminatorSN'))
    with pytest.raises(NotImplementedError, match='gan_type'):
        _Bare.settings(dict(GAN_TRAIN))
    with pytest.raises(NotImplementedError, match='gan_type'):
        _Bare.settings({}, network_d=dict(type='ImageDiscriminator'))
    with pytest.raises(NotImplementedError, match='texture_opt'):
        _Bare.settings(dict(GAN_TRAIN, texture_opt=dict(loss_weight=1.0)), network_d=dict(type='ImageDiscriminator'))


def test_model_builds_discriminator_losses_and_two_optimizers():
    from mrefsr_amd.archs.discriminator_arch import ImageDiscriminator
    from mrefsr_amd.losses import GANLoss, GradientPenaltyLoss
    m = _Bare.settings(dict(GAN_TRAIN), network_d=dict(type='ImageDiscriminator', ndf=32))
    assert isinstance(m.net_d, ImageDiscriminator) and m.net_d.training
    assert isinstance(m.cri_gan, GANLoss) and m.cri_gan.gan_type == 'wgan' and m.cri_gan.loss_weight == 1e-3
    assert isinstance(m.cri_grad_penalty, GradientPenaltyLoss) and m.cri_grad_penalty.loss_weight == 10.0
    assert m.optimizers == [m.optimizer_d] and len(m.schedulers) == 1   # (_Bare has no optimizer_g: optimizer_d is appended)
    assert m.schedulers[0].optimizer is m.optimizer_d
    pg = m.optimizer_d.param_groups[0]
    assert pg['lr'] == 1e-4 and tuple(pg['betas']) == (0.9, 0.999) and len(pg['params']) == len(list(m.net_d.parameters()))
    m = _Bare.settings(dict(GAN_TRAIN, gan_type='vanilla', grad_penalty_weight=0), network_d=dict(type='ImageDiscriminator'))
    assert m.cri_grad_penalty is None


def test_graph_capture_is_not_asked_for_with_a_discriminator():
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    m = MultiRefRestorationModel.__new__(MultiRefRestorationModel)
    m.opt = dict(train=dict(hip_graph=True))
    assert m._train_graph_wanted()
    m.opt = dict(train=dict(hip_graph=True, **GAN_TRAIN), network_d=dict(type='ImageDiscriminator'))
    assert not m._train_graph_wanted()


def test_compat_replaces_the_discriminator():
    from mrefsr_amd import compat
    assert 'ImageDiscriminator' in compat._ARCHS


def test_disc_kernels_compile_without_scratch(tmp_path):
    """every kernel of csrc/disc.hip builds for gfx950 with no scratch memory; the convolution kernels use the f32-input MFMA"""
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    asm = str(tmp_path / 'disc.s')
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-fno-slp-vectorize', '-S',
                    '--cuda-device-only', os.path.join(ROOT, 'mrefsr_amd', 'csrc', 'disc.hip'), '-o', asm], check=True, capture_output=True)
    text = open(asm).read()
    kernels = re.findall(r'^(_ZN12_GLOBAL__N_1\d+(\w+?_kernel)\w*):', text, flags=re.M)
    names = sorted({k for _, k in kernels})
    for want in ('conv_gemm_kernel', 'conv_wgrad_kernel', 'conv_wgrad_finish_kernel', 'conv_pack_weight_kernel', 'pack_image_kernel',
                 'unpack_image_kernel', 'chan_stats_kernel', 'chan_sums_kernel', 'bn_stats_finish_kernel', 'chan_sums_finish_kernel',
                 'bn_apply_kernel', 'bn_bwd_apply_kernel', 'bn_dbl_apply_kernel', 'head_fwd_kernel', 'head_bwd_kernel', 'head_dbl_kernel',
                 'head_params_kernel'):
        assert want in names, (want, names)
    sizes = re.findall(r'; ScratchSize: (\d+)', text)
    assert len(sizes) == len(kernels) and set(sizes) == {'0'}, sizes
    for label, name in kernels:
        body = text.split(label + ':', 1)[1].split('s_endpgm', 1)[0]
        assert ('v_mfma_f32_16x16x4_f32' in body) == (name in ('conv_gemm_kernel', 'conv_wgrad_kernel')), label
