"""CPU: the loss options of the training step (mrefsr_amd/losses, MultiRefRestorationModel.init_training_settings) and the build of
the perceptual-loss kernels (csrc/percep.hip).  The GPU side: tests/test_percep_kernels_gpu.py, tests/test_percep_train_gpu.py."""
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import spec_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = {'conv1_2': 0.1, 'conv2_2': 0.1, 'conv3_4': 1.0, 'conv4_4': 1.0, 'conv5_4': 1.0}


def test_registry_holds_the_reference_loss_names():
    from mrefsr_amd.losses import LOSS_REGISTRY, build_loss
    for name in ('L1Loss', 'MSELoss', 'CharbonnierLoss', 'PerceptualLoss'):
        assert name in LOSS_REGISTRY
    assert build_loss({'type': 'CharbonnierLoss', 'loss_weight': 2.0}).eps == 1e-12   # the reference constructor's default


def test_perceptual_options_refused_at_construction():
    from mrefsr_amd.losses import PerceptualLoss
    with pytest.raises(NotImplementedError, match='L2loss'):
        PerceptualLoss(LAYERS, criterion='l2')
    with pytest.raises(NotImplementedError, match='fro'):
        PerceptualLoss(LAYERS, perceptual_weight=0.0, style_weight=1.0, criterion='fro')
    with pytest.raises(NotImplementedError):
        PerceptualLoss(LAYERS, criterion='cosine')
    PerceptualLoss(LAYERS, criterion='fro')      # a perceptual-only Frobenius loss is fine


@pytest.mark.parametrize('name', ['L1Loss', 'MSELoss', 'CharbonnierLoss'])
def test_pixel_criteria_refuse_what_the_model_never_passes(name):
    from mrefsr_amd import losses
    cls = getattr(losses, name)
    for red in ('sum', 'none'):
        with pytest.raises(NotImplementedError, match='reduction'):
            cls(loss_weight=1.0, reduction=red)
    crit = cls(loss_weight=1.0)
    x = torch.rand(1, 3, 4, 4)
    with pytest.raises(NotImplementedError, match='weight'):
        crit(x, x, weight=torch.ones_like(x))


def test_pixel_criteria_values():
    from mrefsr_amd.losses import CharbonnierLoss, L1Loss, MSELoss
    a, b = torch.rand(2, 3, 8, 8, dtype=torch.float64), torch.rand(2, 3, 8, 8, dtype=torch.float64)
    assert torch.equal(L1Loss(0.5)(a, b), 0.5 * (a - b).abs().mean())
    assert torch.equal(MSELoss(2.0)(a, b), 2.0 * F.mse_loss(a, b, reduction='none').mean())
    assert torch.equal(CharbonnierLoss(3.0, eps=1e-6)(a, b), 3.0 * torch.sqrt((a - b)**2 + 1e-6).mean())


def test_perceptual_loss_refuses_cpu_tensors():
    from mrefsr_amd.losses import PerceptualLoss
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(NotImplementedError, match='CPU'):
        PerceptualLoss({'conv1_2': 1.0})(x, x)


def test_perceptual_state_dict_keys_are_the_references(golden):
    """keys of PerceptualLoss.state_dict() == the reference's (recorded by tests/golden/gen_golden_percep.py): vgg.mean, vgg.std,
    vgg.vgg_net.convX_Y.{weight,bias} with the same shapes"""
    from mrefsr_amd.losses import PerceptualLoss
    g = golden('e2e_c2_percep')
    want = spec_from(g, 'vgg_')
    got = [(k, tuple(v.shape)) for k, v in PerceptualLoss(LAYERS).state_dict().items()]
    assert sorted(got) == sorted(want)


class _Bare:
    """init_training_settings on a model object without a GPU (the constructor itself needs one)"""

    @staticmethod
    def settings(train_extra, network_d=None):
        from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
        m = MultiRefRestorationModel.__new__(MultiRefRestorationModel)
        train = dict(pixel_criterion='L1Loss', pixel_weight=1.0, net_g_pretrain_steps=0,
                     scheduler=dict(type='MultiStepLR', milestones=[10], gamma=0.5))
        train.update(train_extra)
        m.opt = dict(train=train, network_d=network_d)
        m.device = torch.device('cpu')
        m.optimizers, m.schedulers = [], []
        m.init_training_settings()
        return m


def test_model_builds_perceptual_style_and_pixel_criteria():
    from mrefsr_amd.losses import CharbonnierLoss, PerceptualLoss
    m = _Bare.settings(dict(pixel_criterion='CharbonnierLoss', pixel_weight=0.5,
                            perceptual_opt=dict(layer_weights=LAYERS, criterion='l1'),
                            style_opt=dict(layer_weights=LAYERS, perceptual_weight=0, style_weight=10.0)))
    assert isinstance(m.cri_pix, CharbonnierLoss) and m.cri_pix.loss_weight == 0.5 and m.cri_pix.eps == 1e-12
    assert isinstance(m.cri_perceptual, PerceptualLoss) and isinstance(m.cri_style, PerceptualLoss)
    assert m.cri_perceptual.vgg is not m.cri_style.vgg          # two instances, each with its own VGG (ref :126-141)
    assert m.cri_style.style_weight == 10.0 and m.cri_style.perceptual_weight == 0
    assert _Bare.settings(dict(pixel_weight=0)).cri_pix is None   # pixel_weight <= 0 removes the pixel term


def test_model_still_refuses_adversarial_and_texture_losses():
    with pytest.raises(NotImplementedError, match='gan_type'):
        _Bare.settings(dict(gan_type='vanilla', gan_weight=1.0))
    with pytest.raises(NotImplementedError, match='texture_opt'):
        _Bare.settings(dict(texture_opt=dict(loss_weight=1.0)))
    with pytest.raises(NotImplementedError, match='network_d'):
        _Bare.settings({}, network_d=dict(type='VGGStyleDiscriminator160'))
    with pytest.raises(NotImplementedError, match='pixel_criterion'):
        _Bare.settings(dict(pixel_criterion='PerceptualLoss'))


def test_graph_capture_is_not_asked_for_with_a_perceptual_loss(monkeypatch):
    from mrefsr_amd.models.multi_ref_restoration_model import MultiRefRestorationModel
    m = MultiRefRestorationModel.__new__(MultiRefRestorationModel)
    m.opt = dict(train=dict(hip_graph=True))
    assert m._train_graph_wanted()
    m.opt = dict(train=dict(hip_graph=True, perceptual_opt=dict(layer_weights=LAYERS)))
    assert not m._train_graph_wanted()
    m.opt = dict(train=dict(hip_graph=True, style_opt=dict(layer_weights=LAYERS, style_weight=1.0)))
    assert not m._train_graph_wanted()


def test_percep_kernels_compile_without_scratch(tmp_path):
    """every kernel of csrc/percep.hip builds for gfx950 with no scratch memory; the Gram kernels use the f32-input MFMA"""
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    asm = str(tmp_path / 'percep.s')
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-fno-slp-vectorize', '-S',
                    '--cuda-device-only', os.path.join(ROOT, 'mrefsr_amd', 'csrc', 'percep.hip'), '-o', asm], check=True, capture_output=True)
    text = open(asm).read()
    kernels = re.findall(r'^(_ZN12_GLOBAL__N_1\d+(\w+?_kernel)E\w*):', text, flags=re.M)
    assert sorted(k for _, k in kernels) == sorted(['maxpool2_kernel', 'maxpool2_bwd_kernel', 'tap_crit_kernel', 'tap_crit_finish_kernel',
                                                   'gram_kernel', 'gram_finish_kernel', 'gram_bwd_kernel', 'image_bwd_kernel']), kernels
    sizes = re.findall(r'; ScratchSize: (\d+)', text)
    assert len(sizes) == 8 and set(sizes) == {'0'}, sizes
    for label, name in kernels:
        body = text.split(label + ':', 1)[1].split('s_endpgm', 1)[0]
        assert ('v_mfma_f32_16x16x4_f32' in body) == (name in ('gram_kernel', 'gram_bwd_kernel')), name
