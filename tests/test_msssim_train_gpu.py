"""GPU: the multi-reference training step with train.msssim_opt (B = 2, K = 3, LR 16 x 12 -> GT 64 x 48, n_blocks 2, synthetic
weights, one absent reference; three levels: 64 x 48, 32 x 24, 16 x 12).

  1. L1 + MS-SSIM: l_g_pix and l_g_msssim logged, l_g_msssim the bits of the module called by hand on the output, the gradient at
     the output the bits of the sum of the two criteria's gradients, finite parameter gradients, the same log value through
     optimize_parameters
  2. pixel_weight 0, MS-SSIM alone: a step is taken; the gradient at the output against the float64 expression, within the generic
     bar of tests/test_msssim_kernels_gpu.py
  3. train.deterministic: the same step twice, identical bits of loss, gradients and updated parameters
  4. RefRestorationModel inherits the term
  5. an unknown key in msssim_opt and five levels on this GT are refused"""
import numpy as np
import pytest
import torch

import synth
from test_msssim_kernels_gpu import expression, reference
from test_ssim_loss_kernels_gpu import rel_grad_err

pytestmark = pytest.mark.gpu

B, K, LR_H, LR_W = 2, 3, 16, 12
VALID = [[True, True, True], [True, False, True]]
MSSSIM_OPT = dict(loss_weight=0.5, channel='y', weights=[0.3, 0.3, 0.4])


@pytest.fixture(autouse=True, scope='module')
def _zero_chunks_as_found():
    """The training engine carves its zeroed accumulators from process-wide chunks (hip.zeros_f32: one fill launch per chunk, a
    chunk lasts a dozen steps), so which step of a process launches a fill follows from every step taken before it -- and
    tests that compare the kernel lists of two steps (test_r1_train_gpu.py::test_options_absent_the_step_launches_what_it_launched)
    see that.  This module's steps take their accumulators from chunks of their own; the chunks it found are put back untouched."""
    from mrefsr_amd import hip
    found = dict(hip._zero_chunks.entries)
    hip._zero_chunks.entries.clear()
    yield
    torch.cuda.synchronize()
    hip._zero_chunks.entries.clear()
    hip._zero_chunks.entries.update(found)


def _load_synth(module):
    spec = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    module.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()}, strict=True)


def _opt(pixel_weight=1.0, deterministic=False, msssim_opt=MSSSIM_OPT):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), total_iter=255000, warmup_iter=-1,
                 net_g_pretrain_steps=0, pixel_criterion='L1Loss', pixel_weight=pixel_weight, msssim_opt=dict(msssim_opt))
    if deterministic:
        train['deterministic'] = True
    return dict(
        name='msssim', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, manual_seed=10, is_train=True,
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
    samples = [synth.sr_sample(f'msssim/s{i}', K, LR_H, LR_W) for i in range(B)]
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


def test_model_step_with_l1_and_the_msssim_loss():
    model, data = _model_and_data()
    assert model.cri_msssim is not None and model.cri_pix is not None and model.cri_ssim is None and not model._train_graph_wanted()
    model.opt['train']['hip_graph'] = True      # excluded from the experimental training graph exactly as ssim_opt is
    assert not model._train_graph_wanted()
    model.opt['train'].pop('hip_graph')
    seen = _forward_hooked(model, data)
    log = model.get_current_log()
    assert 'l_g_pix' in log and 'l_g_msssim' in log and np.isfinite(log['l_g_msssim']) and 0 < log['l_g_msssim'] <= 0.5
    assert tuple(model.output.shape) == (B, 3, 4 * LR_H, 4 * LR_W)
    out = model.output.detach().requires_grad_(True)
    by_hand = model.cri_msssim(out, model.gt)
    by_hand.backward()
    assert log['l_g_msssim'] == float(by_hand.detach())                            # bit for bit
    out2 = model.output.detach().requires_grad_(True)
    model.cri_pix(out2, model.gt).backward()
    assert torch.equal(seen, out.grad + out2.grad)
    for n, p in model.get_bare_model(model.net_g).named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    # the whole step through the public entry point: the same log value, an update taken
    model2, _ = _model_and_data()
    model2.feed_data(data)
    model2.optimize_parameters(1)
    assert model2.get_current_log()['l_g_msssim'] == log['l_g_msssim'] and model2.range_fallbacks == 0


def test_model_step_with_the_msssim_loss_alone():
    model, data = _model_and_data(pixel_weight=0)
    assert model.cri_pix is None
    seen = _forward_hooked(model, data)
    log = model.get_current_log()
    assert 'l_g_msssim' in log and 'l_g_pix' not in log
    weights = tuple(MSSSIM_OPT['weights'])
    loss64, grad64 = expression(model.output.detach().cpu(), model.gt.cpu(), 'y', weights, torch.float64)
    loss_bar, grad_bar = reference()[1]['generic']
    el = abs(log['l_g_msssim'] - 0.5 * loss64)
    eg = rel_grad_err(seen.cpu(), 0.5 * grad64) if float(grad64.abs().max()) > 0 else float(seen.abs().max())
    print(f'MS-SSIM alone: l_g_msssim {log["l_g_msssim"]:.6e}, |loss err| {el:.2e} (bar {0.5 * loss_bar:.2e}), gradient rel err {eg:.2e} '
          f'(bar {grad_bar:.2e})')
    assert el <= 0.5 * loss_bar and eg <= grad_bar
    # a step is taken through the public entry point: the log value is the same
    model2, _ = _model_and_data(pixel_weight=0)
    model2.feed_data(data)
    model2.optimize_parameters(1)
    assert model2.get_current_log()['l_g_msssim'] == log['l_g_msssim'] and model2.range_fallbacks == 0


def test_deterministic_step_twice_gives_identical_bits():
    runs = []
    for _ in range(2):
        model, data = _model_and_data(deterministic=True)
        model.feed_data(data)
        model.optimize_parameters(1)
        net = model.get_bare_model(model.net_g)
        runs.append((model.log_dict['l_g_msssim'].clone(), model.log_dict['l_g_pix'].clone(),
                     {n: p.grad.detach().clone() for n, p in net.named_parameters()},
                     {n: p.detach().clone() for n, p in net.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for n in runs[0][2]:
        assert torch.equal(runs[0][2][n], runs[1][2][n]), n
        assert torch.equal(runs[0][3][n], runs[1][3][n]), n


def test_single_reference_model_step_with_the_msssim_loss():
    """RefRestorationModel (K = 1, no ref_valid) inherits the MS-SSIM term"""
    from mrefsr_amd.models import build_model
    opt = _opt(msssim_opt=dict(loss_weight=1.0, channel='rgb', weights=[0.5, 0.5]))
    opt.update(model_type='RefRestorationModel', network_g=dict(type='RestorationNet', ngf=64, n_blocks=2, groups=8),
               network_extractor=dict(type='ContrasExtractorSep'))
    torch.manual_seed(10)
    model = build_model(opt)
    for name in ('net_g', 'net_extractor', 'net_map'):
        _load_synth(model.get_bare_model(getattr(model, name)))
    samples = [synth.sr_sample(f'msssim1/s{i}', 1, LR_H, LR_W) for i in range(B)]
    data = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    data['img_ref'] = data.pop('img_ref_list')[:, 0].contiguous()
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    hand = float(model.cri_msssim(model.output.detach(), model.gt))
    assert np.isfinite(log['l_g_msssim']) and 0 < log['l_g_msssim'] <= 1 and log['l_g_msssim'] == hand
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.net_g.parameters())


def test_an_unknown_key_and_too_many_levels_are_refused():
    from mrefsr_amd.models import build_model
    with pytest.raises(ValueError, match=r"msssim_opt.*\['levels'\]"):
        build_model(_opt(msssim_opt=dict(loss_weight=0.5, levels=3)))
    model, data = _model_and_data(msssim_opt=dict(loss_weight=0.5))      # the default five levels on a 64 x 48 GT
    before = {n: p.detach().clone() for n, p in model.get_bare_model(model.net_g).named_parameters()}
    model.feed_data(data)
    with pytest.raises(ValueError, match=r'64 x 48.*M = 5.*at most M = 3'):
        model.optimize_parameters(1)
    assert all(torch.equal(p.detach(), before[n]) for n, p in model.get_bare_model(model.net_g).named_parameters())
