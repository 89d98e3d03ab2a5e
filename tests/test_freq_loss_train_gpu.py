"""GPU: the multi-reference training step with train.freq_opt (B = 2, K = 3, LR 16 x 12 -> GT 64 x 48, n_blocks 2, synthetic
weights, one absent reference).

  1. L1 + FFTLoss: l_g_pix and l_g_freq logged, l_g_freq the bits of the module called by hand on the output, the gradient at the
     output the bits of the sum of the two criteria's gradients, finite parameter gradients, the same log value through
     optimize_parameters
  2. pixel_weight 0, FocalFrequencyLoss alone: a step is taken; the gradient at the output against the float64 definition, within
     the generic bar of tests/test_freq_loss_kernels_gpu.py
  3. train.deterministic: the same step twice, identical bits of loss, gradients and updated parameters
  4. RefRestorationModel inherits the term"""
import numpy as np
import pytest
import torch

import synth
from test_freq_loss_kernels_gpu import definition64, reference, rel_grad_err

pytestmark = pytest.mark.gpu

B, K, LR_H, LR_W = 2, 3, 16, 12
VALID = [[True, True, True], [True, False, True]]
FFT_OPT = dict(type='FFTLoss', loss_weight=0.05)
FOCAL_OPT = dict(type='FocalFrequencyLoss', loss_weight=2.0, alpha=1.0)


def _load_synth(module):
    spec = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    module.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()}, strict=True)


def _opt(pixel_weight=1.0, deterministic=False, freq_opt=FFT_OPT):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), total_iter=255000, warmup_iter=-1,
                 net_g_pretrain_steps=0, pixel_criterion='L1Loss', pixel_weight=pixel_weight, freq_opt=dict(freq_opt))
    if deterministic:
        train['deterministic'] = True
    return dict(
        name='freq', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, manual_seed=10, is_train=True,
        dist=False, rank=0, network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=2, groups=8),
        network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                         vgg_type='vgg19'),
        network_extractor=dict(type='ContrasMultiExtractorSep'),
        path=dict(pretrain_network_g=None, pretrain_network_feature_extractor=None, strict_load=True), train=train, val=dict(save_img=False))


def _model_and_data(**kw):
    from mrefsr_amd.models import build_model
    torch.manual_seed(10)
    model = build_model(_opt(**kw))
    for name in ('net_g', 'net_extractor', 'net_map'):
        _load_synth(model.get_bare_model(getattr(model, name)))
    samples = [synth.sr_sample(f'freq/s{i}', K, LR_H, LR_W) for i in range(B)]
    data = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    data['ref_valid'] = torch.tensor(VALID)
    return model, data


def _forward_hooked(model, data):
    """feed, forward, a hook on the output, the losses and their backward: -> the gradient that reached the output"""
    from mrefsr_amd.archs import nhwc_train
    model.feed_data(data)
    model.optimizer_g.zero_grad()
    nhwc_train.begin_step()
    model.output = model._forward()
    seen = []
    model.output.register_hook(lambda g: seen.append(g.detach().clone()))
    assert model._loss_and_backward(1)
    model.check_numeric_range()
    assert len(seen) == 1
    return seen[0]


def test_model_step_with_l1_and_the_fft_loss():
    from mrefsr_amd.losses import FFTLoss
    model, data = _model_and_data()
    assert isinstance(model.cri_freq, FFTLoss) and model.cri_pix is not None and not model._train_graph_wanted()
    seen = _forward_hooked(model, data)
    log = model.get_current_log()
    assert 'l_g_pix' in log and 'l_g_freq' in log and np.isfinite(log['l_g_freq']) and log['l_g_freq'] > 0
    assert tuple(model.output.shape) == (B, 3, 4 * LR_H, 4 * LR_W)
    out = model.output.detach().requires_grad_(True)
    by_hand = model.cri_freq(out, model.gt)
    by_hand.backward()
    assert log['l_g_freq'] == float(by_hand.detach())                            # bit for bit
    out2 = model.output.detach().requires_grad_(True)
    model.cri_pix(out2, model.gt).backward()
    assert float(out.grad.abs().max()) > 0 and torch.equal(seen, out2.grad + out.grad)
    for n, p in model.get_bare_model(model.net_g).named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    # the whole step through the public entry point: the same log value, an update taken
    model2, _ = _model_and_data()
    model2.feed_data(data)
    model2.optimize_parameters(1)
    assert model2.get_current_log()['l_g_freq'] == log['l_g_freq'] and model2.range_fallbacks == 0


def test_model_step_with_the_focal_frequency_loss_alone():
    from mrefsr_amd.losses import FocalFrequencyLoss
    model, data = _model_and_data(pixel_weight=0, freq_opt=FOCAL_OPT)
    assert model.cri_pix is None and isinstance(model.cri_freq, FocalFrequencyLoss)
    seen = _forward_hooked(model, data)
    log = model.get_current_log()
    assert 'l_g_freq' in log and 'l_g_pix' not in log
    loss64, grad64 = definition64(model.output.detach().cpu(), model.gt.cpu(), 'focal-1')
    loss_bar, grad_bar = reference()[1]['generic']
    el, eg = abs(log['l_g_freq'] - 2.0 * loss64) / abs(2.0 * loss64), rel_grad_err(seen.cpu(), 2.0 * grad64)
    print(f'focal alone: l_g_freq {log["l_g_freq"]:.6e}, loss rel err {el:.2e} (bar {loss_bar:.2e}), gradient rel err {eg:.2e} (bar {grad_bar:.2e})')
    assert el <= loss_bar and eg <= grad_bar
    # a step is taken through the public entry point: the parameters move
    model2, _ = _model_and_data(pixel_weight=0, freq_opt=FOCAL_OPT)
    before = {n: p.detach().clone() for n, p in model2.get_bare_model(model2.net_g).named_parameters()}
    model2.feed_data(data)
    model2.optimize_parameters(1)
    assert model2.get_current_log()['l_g_freq'] == log['l_g_freq'] and model2.range_fallbacks == 0
    moved = [n for n, p in model2.get_bare_model(model2.net_g).named_parameters() if not torch.equal(p.detach(), before[n])]
    assert moved


@pytest.mark.parametrize('freq_opt', [FFT_OPT, FOCAL_OPT], ids=['fft', 'focal'])
def test_deterministic_step_twice_gives_identical_bits(freq_opt):
    runs = []
    for _ in range(2):
        model, data = _model_and_data(deterministic=True, freq_opt=freq_opt)
        model.feed_data(data)
        model.optimize_parameters(1)
        net = model.get_bare_model(model.net_g)
        runs.append((model.log_dict['l_g_freq'].clone(), model.log_dict['l_g_pix'].clone(),
                     {n: p.grad.detach().clone() for n, p in net.named_parameters()},
                     {n: p.detach().clone() for n, p in net.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for n in runs[0][2]:
        assert torch.equal(runs[0][2][n], runs[1][2][n]), n
        assert torch.equal(runs[0][3][n], runs[1][3][n]), n


def test_single_reference_model_step_with_the_frequency_loss():
    """RefRestorationModel (K = 1, no ref_valid) inherits the frequency term"""
    from mrefsr_amd.models import build_model
    opt = _opt(freq_opt=dict(type='FocalFrequencyLoss', loss_weight=1.0, alpha=0.5))
    opt.update(model_type='RefRestorationModel', network_g=dict(type='RestorationNet', ngf=64, n_blocks=2, groups=8),
               network_extractor=dict(type='ContrasExtractorSep'))
    torch.manual_seed(10)
    model = build_model(opt)
    for name in ('net_g', 'net_extractor', 'net_map'):
        _load_synth(model.get_bare_model(getattr(model, name)))
    samples = [synth.sr_sample(f'freq1/s{i}', 1, LR_H, LR_W) for i in range(B)]
    data = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    data['img_ref'] = data.pop('img_ref_list')[:, 0].contiguous()
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    hand = float(model.cri_freq(model.output.detach(), model.gt))
    assert np.isfinite(log['l_g_freq']) and log['l_g_freq'] > 0 and log['l_g_freq'] == hand
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.net_g.parameters())
