"""GPU: ContextualLoss (mrefsr_amd/losses) through the VGG node of the training engine, and the training step with
train.contextual_opt (B = 2, K = 3, LR 16 x 12 -> GT 64 x 48, n_blocks 2, synthetic weights, one absent reference).

  1. the loss and d loss / d output against a float64 CPU restatement (the synthetic-weight VGG in torch, contextual_loss_torch per
     tap) that routes through the device's own selections (nhwc_train.KEEP_CX); yardstick: the same restatement in torch fp32 on
     the GPU, the kernels within 4 x its error (relative L2 for the image gradient: a single near-tie moves the maximum norm)
  2. a model step with L1 + contextual and one with the contextual loss alone; 3. two fresh models the same bits, a
     train.deterministic step twice the same bits; 4. RefRestorationModel inherits the term; 5. without the option the step
     launches what it launched"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth

pytestmark = pytest.mark.gpu

TAPS = {'relu2_2': 1.0, 'relu3_1': 0.5, 'conv4_2': 0.25}
B, K, LR_H, LR_W = 2, 3, 16, 12
VALID = [[True, True, True], [True, False, True]]
CX_OPT = dict(layer_weights={'relu2_2': 1.0, 'relu3_1': 1.0}, band_width=0.5, loss_weight=0.1)
ULP32 = 2.0 ** -23


@pytest.fixture(autouse=True, scope='module')
def _own_zero_chunks():
    """the module's launches draw their zeroed accumulator words (hip.zeros_f32) from chunks of their own and leave the process-wide
    chunk cursor where they found it: tests elsewhere that compare the kernel lists of two steps see its fill launches"""
    from mrefsr_amd import hip
    kept = dict(hip._zero_chunks.entries)
    hip._zero_chunks.entries.clear()
    yield
    hip._zero_chunks.entries.clear()
    hip._zero_chunks.entries.update(kept)


def _vgg_sd(loss):
    spec = [(k, tuple(v.shape)) for k, v in loss.state_dict().items()]
    return synth.state_dict(spec)


def _images(b, h, w, seed):
    """a bicubic-upsampled random base plus 0.05 noise; the target is a crop, the output the crop shifted by (2, 1) pixels plus 0.03
    noise: not registered to the pixel, the case the loss is for"""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(b, 3, (h + 2) // 4 + 2, (w + 1) // 4 + 2, generator=g)
    big = F.interpolate(base, size=(h + 2, w + 1), mode='bicubic', align_corners=False) + 0.05 * torch.randn(b, 3, h + 2, w + 1, generator=g)
    gt = big[:, :, :h, :w].contiguous()
    x = (big[:, :, 2:, 1:] + 0.03 * torch.randn(b, 3, h, w, generator=g)).contiguous()
    return x, gt


def _ref(sd, x, gt, layer_weights, band_width, loss_weight, norm_img=False, picks=None, dtype=torch.float64, device='cpu'):
    """ContextualLoss.forward restated: the VGG stack in torch, contextual_loss_torch per tap in network order -> (loss, d loss / d x,
    per tap the parts of the definition).  picks: per tap dict(jmin, imax), the selections the values and the gradient route through"""
    from mrefsr_amd.archs.vgg_arch import NAMES
    from mrefsr_amd.losses import contextual_loss_torch
    x = x.detach().to(device, dtype).requires_grad_(True)
    gt = gt.detach().to(device, dtype)
    sd = {k: torch.from_numpy(v).to(device, dtype) for k, v in sd.items()}
    mean, std = sd['vgg.mean'], sd['vgg.std']
    order = [n for n in NAMES['vgg19'] if n in layer_weights]
    last = NAMES['vgg19'].index(order[-1])

    def feats(img):
        h = (img + 1.) * 0.5 if norm_img else img
        h = (h - mean) / std
        out = {}
        for name in NAMES['vgg19'][:last + 1]:
            if name.startswith('conv'):
                h = F.conv2d(h, sd[f'vgg.vgg_net.{name}.weight'], sd[f'vgg.vgg_net.{name}.bias'], padding=1)
            elif name.startswith('relu'):
                h = F.relu(h)
            else:
                h = F.max_pool2d(h, 2, 2)
            if name in layer_weights:
                out[name] = h.clone()
        return out
    fx, fg = feats(x), feats(gt)
    total, parts = 0, []
    for j, name in enumerate(order):
        pk = {} if picks is None else {k: picks[j][k].to(device) for k in ('jmin', 'imax')}
        l, p = contextual_loss_torch(fx[name], fg[name], band_width, parts=True, **pk)
        total = total + l * layer_weights[name]
        parts.append(p)
    total = total * loss_weight
    total.backward()
    return total.detach(), x.grad, parts


def _rel_l2(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


@pytest.mark.parametrize('shape', [(2, 48, 40), (2, 64, 64)], ids=['48x40', '64x64'])
def test_contextual_loss_against_fp64(shape):
    from mrefsr_amd.archs import nhwc_train
    from mrefsr_amd.losses import ContextualLoss
    bw, lw, gup = 0.5, 0.8, 1.3
    loss = ContextualLoss(TAPS, band_width=bw, loss_weight=lw).cuda()
    sd = _vgg_sd(loss)
    loss.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    x, gt = _images(*shape, seed=shape[1])
    xc = x.cuda().requires_grad_(True)
    nhwc_train.KEEP_CX = []
    try:
        val = loss(xc, gt.cuda())
        picks = [{k: d[k].cpu().long() for k in ('jmin', 'imax')} for d in nhwc_train.KEEP_CX[0]]
    finally:
        nhwc_train.KEEP_CX = None
    (val * gup).backward()
    l64, g64, parts = _ref(sd, x, gt, TAPS, bw, lw)
    cx64 = [p['CX'].tolist() for p in parts]
    # no tap is saturated (the 6 x 5 positions of conv4_2 sit at 0.98 on the smaller image; the kernel tests' own fields keep 0.98)
    assert all(0.05 <= v <= 0.99 for t in cx64 for v in t), cx64
    differing = [(int((pk['jmin'] != p['jmin']).sum()), int((pk['imax'] != p['imax']).sum())) for pk, p in zip(picks, parts)]
    l64d, g64d, _ = _ref(sd, x, gt, TAPS, bw, lw, picks=picks)
    # the yardstick: the same restatement in torch fp32 on the GPU, against float64 through ITS selections
    l32, g32, parts32 = _ref(sd, x, gt, TAPS, bw, lw, dtype=torch.float32, device='cuda')
    picks32 = [{k: p[k].cpu() for k in ('jmin', 'imax')} for p in parts32]
    _, g64_32, _ = _ref(sd, x, gt, TAPS, bw, lw, picks=picks32)
    yard_loss = max(abs(float(l32) - float(l64)) / abs(float(l64)), ULP32)
    yard_grad = _rel_l2(g32, g64_32)
    loss_err = abs(float(val.detach()) - float(l64d)) / abs(float(l64d))
    grad_err = _rel_l2(xc.grad, gup * g64d)
    print(f'{shape}: loss {float(l64):.6f}, CX per tap {[[round(v, 3) for v in t] for t in cx64]}, differing (jmin, imax) per tap {differing}; '
          f'loss rel err {loss_err:.2e} (torch fp32 {yard_loss:.2e}), image gradient rel L2 err {grad_err:.2e} (torch fp32 {yard_grad:.2e})')
    for (dj, di), p in zip(differing, parts):
        assert dj <= 0.005 * p['jmin'].numel() and di <= 0.005 * p['imax'].numel()
    assert val.dim() == 0 and loss_err <= 4 * yard_loss
    assert grad_err <= 4 * yard_grad


def _load_synth(module):
    spec = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    module.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()}, strict=True)


def _opt(pixel_weight=1.0, deterministic=False, contextual_opt=CX_OPT):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), total_iter=255000, warmup_iter=-1,
                 net_g_pretrain_steps=0, pixel_criterion='L1Loss', pixel_weight=pixel_weight)
    if contextual_opt is not None:
        train['contextual_opt'] = dict(contextual_opt)
    if deterministic:
        train['deterministic'] = True
    return dict(
        name='contextual', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, manual_seed=10, is_train=True,
        dist=False, rank=0, network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=2, groups=8),
        network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                         vgg_type='vgg19'),
        network_extractor=dict(type='ContrasMultiExtractorSep'),
        path=dict(pretrain_network_g=None, pretrain_network_feature_extractor=None, strict_load=True), train=train, val=dict(save_img=False))


def _built(opt):
    from mrefsr_amd.models import build_model
    torch.manual_seed(10)
    model = build_model(opt)
    for name in ('net_g', 'net_extractor', 'net_map'):
        _load_synth(model.get_bare_model(getattr(model, name)))
    if model.cri_contextual is not None:
        _load_synth(model.cri_contextual)
    return model


def _data(key='contextual', k=K):
    samples = [synth.sr_sample(f'{key}/s{i}', k, LR_H, LR_W) for i in range(B)]
    return {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}


def _model_and_data(**kw):
    data = _data()
    data['ref_valid'] = torch.tensor(VALID)
    return _built(_opt(**kw)), data


def _step(model, data):
    net = model.get_bare_model(model.net_g)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    moved = [n for n, p in net.named_parameters() if not torch.equal(p.detach(), before[n])]
    return log, moved


@pytest.mark.parametrize('pixel_weight', [1.0, 0], ids=['l1+contextual', 'contextual alone'])
def test_model_step_with_the_contextual_loss(pixel_weight):
    from mrefsr_amd.losses import ContextualLoss
    model, data = _model_and_data(pixel_weight=pixel_weight)
    assert isinstance(model.cri_contextual, ContextualLoss) and (model.cri_pix is None) == (pixel_weight == 0) and not model._train_graph_wanted()
    log, moved = _step(model, data)
    assert ('l_g_pix' in log) == (pixel_weight > 0) and np.isfinite(log['l_g_contextual']) and log['l_g_contextual'] > 0
    assert moved and model.range_fallbacks == 0
    for n, p in model.get_bare_model(model.net_g).named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    hand = float(model.cri_contextual(model.output.detach(), model.gt))
    assert log['l_g_contextual'] == hand                                       # bit for bit
    # two fresh models give the same bits (the loss values: outside deterministic mode net_g's backward has float-atomic sums)
    model2, _ = _model_and_data(pixel_weight=pixel_weight)
    log2, _ = _step(model2, data)
    assert log2 == log


def test_deterministic_step_twice_gives_identical_bits():
    runs = []
    for _ in range(2):
        model, data = _model_and_data(deterministic=True)
        model.feed_data(data)
        model.optimize_parameters(1)
        net = model.get_bare_model(model.net_g)
        runs.append((model.log_dict['l_g_contextual'].clone(), model.log_dict['l_g_pix'].clone(),
                     {n: p.grad.detach().clone() for n, p in net.named_parameters()},
                     {n: p.detach().clone() for n, p in net.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for n in runs[0][2]:
        assert torch.equal(runs[0][2][n], runs[1][2][n]), n
        assert torch.equal(runs[0][3][n], runs[1][3][n]), n


def test_single_reference_model_step_with_the_contextual_loss():
    """RefRestorationModel (K = 1, no ref_valid) inherits the contextual term"""
    opt = _opt()
    opt.update(model_type='RefRestorationModel', network_g=dict(type='RestorationNet', ngf=64, n_blocks=2, groups=8),
               network_extractor=dict(type='ContrasExtractorSep'))
    model = _built(opt)
    data = _data('contextual1', 1)
    data['img_ref'] = data.pop('img_ref_list')[:, 0].contiguous()
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    hand = float(model.cri_contextual(model.output.detach(), model.gt))
    assert np.isfinite(log['l_g_contextual']) and log['l_g_contextual'] > 0 and log['l_g_contextual'] == hand
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.net_g.parameters())


def _kernel_names(model, data, it):
    from torch.profiler import ProfilerActivity, profile
    model.feed_data(data)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        model.optimize_parameters(it)
        torch.cuda.synchronize()
    return [e.name.replace(' ', '') for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_option_absent_the_step_launches_what_it_launched(monkeypatch):
    """an L1 step without contextual_opt: none of the new kernels, and the same kernel list as a step during which the new path is
    not there to be taken (the class, the engine entry and both hip wrappers replaced by functions that raise).  Both traces start
    from the same process-wide state: nhwc_train's cache of fp16 weight scales emptied, its count of range checks 0, and a fresh
    chunk of hip.zeros_f32."""
    from mrefsr_amd import hip, losses
    from mrefsr_amd.archs import nhwc_train
    data = _data()
    data['ref_valid'] = torch.tensor(VALID)

    def traced(contextual_opt=None):
        hip._zero_chunks.entries.clear()   # (a fresh chunk of zeroed words: its one fill launch falls into the untraced first step)
        nhwc_train.reset_scales()
        monkeypatch.setattr(nhwc_train._scales, 'checks', 0)
        model = _built(_opt(deterministic=True, contextual_opt=contextual_opt))
        model.feed_data(data)
        model.optimize_parameters(1)
        return model, _kernel_names(model, data, 2)
    model, names = traced()
    assert len(names) > 100 and not [n for n in names if 'cx_' in n] and 'l_g_contextual' not in model.get_current_log()

    def gone(*a, **kw):
        raise AssertionError('the contextual path was taken with its option absent')
    for mod, name in ((hip, 'contextual_fwd'), (hip, 'contextual_bwd'), (nhwc_train, 'contextual'), (losses, 'ContextualLoss'),
                      (losses.losses, 'ContextualLoss')):
        monkeypatch.setattr(mod, name, gone)
    _, without = traced()
    assert names == without
    monkeypatch.undo()
    # (the names do show with the option on: per tap six forward and four backward launches, the product twice)
    _, on = traced(CX_OPT)
    taps = len(CX_OPT['layer_weights'])
    count = {k: sum(k in n for n in on) for k in ('cx_mean_kernel', 'cx_normalise_kernel', 'cx_dist_kernel', 'cx_row_kernel', 'cx_col_kernel',
                                                   'cx_finish_kernel', 'cx_rowgrad_kernel', 'cx_grad_gemm_kernel', 'cx_grad_finish_kernel')}
    assert count == dict(cx_mean_kernel=taps, cx_normalise_kernel=taps, cx_dist_kernel=2 * taps, cx_row_kernel=taps, cx_col_kernel=taps,
                         cx_finish_kernel=taps, cx_rowgrad_kernel=taps, cx_grad_gemm_kernel=taps, cx_grad_finish_kernel=taps), count
