"""GPU: the multi-reference training step with train.ldl_opt (B = 2, K = 3, LR 16 x 12 -> GT 64 x 48, n_blocks 2, synthetic
weights, one absent reference, ema_decay 0.999; the EMA weights are net_g's times (1 + 1e-2 randn), seeded, so that
output_ema != output).

  1. L1 + LDL: l_g_pix and l_g_ldl logged, l_g_ldl the bits of the module called by hand on (output, gt, output_ema), the gradient
     at the output the bits of the sum of the two criteria's gradients, finite parameter gradients, the same log value through
     optimize_parameters without a range fallback
  2. output_ema is test()'s output on the same fed batch, bit for bit; the EMA pass leaves the EMA parameters, net_g's
     _offset_count guards and net_g's train mode alone
  3. train.deterministic: the same step twice, identical bits of loss, gradients and updated parameters; with train.hip_adam one
     step runs and the EMA moves
  4. in the pretrain phase there is no l_g_ldl and no EMA pass
  5. RefRestorationModel inherits the term; _train_graph_wanted() is False with ldl_opt"""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

B, K, LR_H, LR_W = 2, 3, 16, 12
VALID = [[True, True, True], [True, False, True]]
LDL_OPT = dict(type='L1Loss', loss_weight=1.0, reduction='mean')


def _load_synth(module):
    spec = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    module.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()}, strict=True)


def _opt(deterministic=False, hip_adam=False, pretrain=0, hip_graph=False):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), total_iter=255000, warmup_iter=-1,
                 net_g_pretrain_steps=pretrain, pixel_criterion='L1Loss', pixel_weight=1.0, ema_decay=0.999, ldl_opt=dict(LDL_OPT))
    if deterministic:
        train['deterministic'] = True
    if hip_adam:
        train['hip_adam'] = True
    if hip_graph:
        train['hip_graph'] = True
    return dict(
        name='ldl', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, manual_seed=10, is_train=True,
        dist=False, rank=0, network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=2, groups=8),
        network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                         vgg_type='vgg19'),
        network_extractor=dict(type='ContrasMultiExtractorSep'),
        path=dict(pretrain_network_g=None, pretrain_network_feature_extractor=None, strict_load=True), train=train, val=dict(save_img=False))


def _perturb_ema(model):
    """net_g_ema = net_g (1 + 1e-2 randn), seeded, through autograd-visible writes (the packed copies follow the versions)"""
    g = torch.Generator().manual_seed(77)
    bare = dict(model.get_bare_model(model.net_g).named_parameters())
    with torch.no_grad():
        for n, p in model.net_g_ema.named_parameters():
            p.copy_(bare[n].detach() * (1.0 + 1e-2 * torch.randn(p.shape, generator=g).to(p.device)))


def _model_and_data(opt=None, single=False, **kw):
    from mrefsr_amd.models import build_model
    torch.manual_seed(10)
    model = build_model(opt if opt is not None else _opt(**kw))
    for name in ('net_g', 'net_extractor', 'net_map'):
        _load_synth(model.get_bare_model(getattr(model, name)))
    _perturb_ema(model)
    samples = [synth.sr_sample(f'ldl/s{i}', 1 if single else K, LR_H, LR_W) for i in range(B)]
    data = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    if single:
        data['img_ref'] = data.pop('img_ref_list')[:, 0].contiguous()
    else:
        data['ref_valid'] = torch.tensor(VALID)
    return model, data


def _forward_hooked(model, data, step=1):
    """feed, forward, a hook on the output, the losses and their backward: -> the gradient that reached the output"""
    from mrefsr_amd.archs import nhwc_train
    model.feed_data(data)
    model.optimizer_g.zero_grad()
    nhwc_train.begin_step()
    model.output = model._forward()
    seen = []
    model.output.register_hook(lambda g: seen.append(g.detach().clone()))
    assert model._loss_and_backward(step)
    model.check_numeric_range()
    assert len(seen) == 1
    return seen[0]


def test_model_step_with_l1_and_the_ldl_loss():
    model, data = _model_and_data()
    assert model.cri_ldl is not None and model.cri_pix is not None and model.net_g_ema is not None and not model._train_graph_wanted()
    seen = _forward_hooked(model, data)
    log = model.get_current_log()
    assert 'l_g_pix' in log and 'l_g_ldl' in log and np.isfinite(log['l_g_ldl']) and log['l_g_ldl'] > 0
    assert tuple(model.output.shape) == tuple(model.output_ema.shape) == (B, 3, 4 * LR_H, 4 * LR_W)
    assert not model.output_ema.requires_grad and not torch.equal(model.output_ema, model.output.detach())
    out = model.output.detach().requires_grad_(True)
    by_hand = model.cri_ldl(out, model.gt, model.output_ema)
    by_hand.backward()
    assert log['l_g_ldl'] == float(by_hand.detach())                            # bit for bit
    out2 = model.output.detach().requires_grad_(True)
    model.cri_pix(out2, model.gt).backward()
    assert float(out.grad.abs().max()) > 0 and torch.equal(seen, out.grad + out2.grad)
    for n, p in model.get_bare_model(model.net_g).named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    # the whole step through the public entry point: the same log value, an update taken, the EMA moved behind the pass
    model2, _ = _model_and_data()
    ema_before = {n: p.detach().clone() for n, p in model2.net_g_ema.named_parameters()}
    model2.feed_data(data)
    model2.optimize_parameters(1)
    assert model2.get_current_log()['l_g_ldl'] == log['l_g_ldl'] and model2.range_fallbacks == 0
    assert torch.equal(model2.output_ema, model.output_ema)
    assert any(not torch.equal(p.detach(), ema_before[n]) for n, p in model2.net_g_ema.named_parameters())


def test_ema_pass_is_the_tested_output_and_leaves_the_training_state_alone():
    model, data = _model_and_data()
    net = model.get_bare_model(model.net_g)
    model.feed_data(data)
    model.optimizer_g.zero_grad()
    from mrefsr_amd.archs import nhwc_train
    nhwc_train.begin_step()
    model.output = model._forward()
    ema_before = {n: p.detach().clone() for n, p in model.net_g_ema.named_parameters()}
    guards = {n: m._offset_count for n, m in net.named_modules() if hasattr(m, '_offset_count')}
    assert guards and all(v > 0 for v in guards.values()) and net.training
    assert model._loss_and_backward(1)
    model.check_numeric_range()
    assert net.training and not model.net_g_ema.training
    assert {n: m._offset_count for n, m in net.named_modules() if hasattr(m, '_offset_count')} == guards
    for n, p in model.net_g_ema.named_parameters():
        assert torch.equal(p.detach(), ema_before[n]) and p.grad is None, n
    for n, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    output_ema = model.output_ema.clone()
    model.feed_data(data)
    model.test()                       # net_g_ema on the same batch (val.hip_graph off)
    assert net.training and torch.equal(model.output, output_ema)


def test_deterministic_step_twice_gives_identical_bits():
    runs = []
    for _ in range(2):
        model, data = _model_and_data(deterministic=True)
        model.feed_data(data)
        model.optimize_parameters(1)
        net = model.get_bare_model(model.net_g)
        runs.append((model.log_dict['l_g_ldl'].clone(), model.log_dict['l_g_pix'].clone(),
                     {n: p.grad.detach().clone() for n, p in net.named_parameters()},
                     {n: p.detach().clone() for n, p in net.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for n in runs[0][2]:
        assert torch.equal(runs[0][2][n], runs[1][2][n]), n
        assert torch.equal(runs[0][3][n], runs[1][3][n]), n


def test_hip_adam_step_reads_the_ema_before_it_writes_it():
    """train.hip_adam writes the EMA inside its launch: the pass has read the weights as they stood before (the same l_g_ldl and
    output_ema as with torch's Adam and model_ema behind it), and the EMA has moved afterwards"""
    plain, data = _model_and_data()
    plain.feed_data(data)
    plain.optimize_parameters(1)
    model, _ = _model_and_data(hip_adam=True)
    before = {n: p.detach().clone() for n, p in model.net_g_ema.named_parameters()}
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert np.isfinite(log['l_g_ldl']) and log['l_g_ldl'] == plain.get_current_log()['l_g_ldl'] and model.range_fallbacks == 0
    assert torch.equal(model.output_ema, plain.output_ema)
    assert any(not torch.equal(p.detach(), before[n]) for n, p in model.net_g_ema.named_parameters())


def test_pretrain_phase_has_no_ldl_term_and_no_ema_pass():
    model, data = _model_and_data(pretrain=1)
    calls = []
    ema_pass = model._ema_pass
    model._ema_pass = lambda: calls.append(1) or ema_pass()
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert 'l_pix' in log and 'l_g_ldl' not in log and not calls and model.output_ema is None
    model.feed_data(data)
    model.optimize_parameters(2)       # the steady phase
    assert 'l_g_ldl' in model.get_current_log() and len(calls) == 1 and model.output_ema is not None


def test_single_reference_model_step_with_the_ldl_loss():
    """RefRestorationModel (K = 1, no ref_valid) inherits the term; train.hip_graph is not taken with it"""
    opt = _opt()
    opt.update(model_type='RefRestorationModel', network_g=dict(type='RestorationNet', ngf=64, n_blocks=2, groups=8),
               network_extractor=dict(type='ContrasExtractorSep'))
    model, data = _model_and_data(opt=opt, single=True)
    assert not model._train_graph_wanted()
    model.opt['train']['hip_graph'] = True
    assert not model._train_graph_wanted()
    model.opt['train'].pop('hip_graph')
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    hand = float(model.cri_ldl(model.output.detach(), model.gt, model.output_ema))
    assert np.isfinite(log['l_g_ldl']) and log['l_g_ldl'] > 0 and log['l_g_ldl'] == hand
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.net_g.parameters())
