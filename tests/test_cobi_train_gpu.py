"""GPU: ContextualLoss with the CoBi options (weight_sp, tap_stride, rgb_patch) through the VGG node of the training engine, and
the training step with them in train.contextual_opt (B = 2, K = 3, LR 16 x 12 -> GT 64 x 48, n_blocks 2, synthetic weights).

  1. the loss and d loss / d output against a float64 CPU restatement (the synthetic-weight VGG in torch; per tap
     contextual_loss_torch on cx_patches_torch / the strided map) that routes through the device's own selections
     (nhwc_train.KEEP_CX); yardstick: the same restatement in torch fp32 on the GPU, the kernels within 4 x its error, a floor of
     one fp32 ulp for the loss (the method of tests/test_contextual_train_gpu.py);  2. the RGB tap alone, no VGG;
  3. none of the new keys: the bits of hip.contextual_fwd / hip.contextual_bwd without weight_sp on the same taps;
  4. a tap of 6400 positions is refused without a stride and runs with one;  5. a model step of both model classes;
  6. a train.deterministic step twice the same bits"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth

pytestmark = pytest.mark.gpu

TAPS = {'relu2_2': 1.0, 'relu3_1': 0.5, 'conv4_2': 0.25}
FULL = dict(weight_sp=0.1, tap_stride={'relu2_2': 2}, rgb_patch=dict(size=5, stride=4, weight=1.0))
B, K, LR_H, LR_W = 2, 3, 16, 12
VALID = [[True, True, True], [True, False, True]]
CX_OPT = dict(layer_weights={'relu2_2': 1.0, 'relu3_1': 1.0}, band_width=0.5, loss_weight=0.1, **FULL)
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


def _load_synth(module):
    spec = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    sd = synth.state_dict(spec) if spec else {}
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return sd


def _images(b, h, w, seed):
    """a bicubic-upsampled random base plus 0.05 noise; the target is a crop, the output the crop shifted by (2, 1) pixels plus 0.03
    noise: not registered to the pixel, the case the loss is for"""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(b, 3, (h + 2) // 4 + 2, (w + 1) // 4 + 2, generator=g)
    big = F.interpolate(base, size=(h + 2, w + 1), mode='bicubic', align_corners=False) + 0.05 * torch.randn(b, 3, h + 2, w + 1, generator=g)
    gt = big[:, :, :h, :w].contiguous()
    x = (big[:, :, 2:, 1:] + 0.03 * torch.randn(b, 3, h, w, generator=g)).contiguous()
    return x, gt


def _ref(sd, x, gt, layer_weights, band_width, loss_weight, weight_sp=0.0, tap_stride=None, rgb_patch=None, norm_img=False, picks=None,
         dtype=torch.float64, device='cpu'):
    """ContextualLoss.forward restated: the RGB tap on cx_patches_torch of the images, then the VGG stack in torch and
    contextual_loss_torch per tap (on its positions (r s, c s)) in network order -> (loss, d loss / d x, per tap the parts of the
    definition).  picks: per tap dict(jmin, imax), the selections the values and the gradient route through"""
    from mrefsr_amd.archs.vgg_arch import NAMES
    from mrefsr_amd.losses import contextual_loss_torch, cx_patches_torch
    x = x.detach().to(device, dtype).requires_grad_(True)
    gt = gt.detach().to(device, dtype)
    sd = {k: torch.from_numpy(v).to(device, dtype) for k, v in sd.items()}
    order = [n for n in NAMES['vgg19'] if n in layer_weights]

    def feats(img):
        h = (img + 1.) * 0.5 if norm_img else img
        out = []
        if rgb_patch:
            out.append((cx_patches_torch(h, rgb_patch['size'], rgb_patch['stride']), rgb_patch['weight']))
        if not order:
            return out
        h = (h - sd['vgg.mean']) / sd['vgg.std']
        for name in NAMES['vgg19'][:NAMES['vgg19'].index(order[-1]) + 1]:
            if name.startswith('conv'):
                h = F.conv2d(h, sd[f'vgg.vgg_net.{name}.weight'], sd[f'vgg.vgg_net.{name}.bias'], padding=1)
            elif name.startswith('relu'):
                h = F.relu(h)
            else:
                h = F.max_pool2d(h, 2, 2)
            if name in layer_weights:
                s = (tap_stride or {}).get(name, 1)
                out.append((h[:, :, ::s, ::s].clone(), layer_weights[name]))
        return out
    total, parts = 0, []
    for j, ((fx, w), (fg, _)) in enumerate(zip(feats(x), feats(gt))):
        pk = {} if picks is None else {k: picks[j][k].to(device) for k in ('jmin', 'imax')}
        l, p = contextual_loss_torch(fx, fg, band_width, parts=True, weight_sp=weight_sp, **pk)
        total = total + l * w
        parts.append(p)
    total = total * loss_weight
    total.backward()
    return total.detach(), x.grad, parts


def _rel_l2(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


def _device(loss, x, gt, gup=1.0):
    """-> (value, d (gup value) / d x, the device's selections per tap)"""
    from mrefsr_amd.archs import nhwc_train
    xc = x.cuda().requires_grad_(True)
    nhwc_train.KEEP_CX = []
    try:
        val = loss(xc, gt.cuda())
        picks = [{k: d[k].cpu().long() for k in ('jmin', 'imax')} for d in nhwc_train.KEEP_CX[0]]
    finally:
        nhwc_train.KEEP_CX = None
    (val * gup).backward()
    return val.detach(), xc.grad, picks


@pytest.mark.parametrize('taps', [TAPS, {}], ids=['three taps + rgb', 'rgb alone'])
def test_cobi_loss_against_fp64(taps):
    from mrefsr_amd.losses import ContextualLoss
    bw, lw, gup = 0.5, 0.8, 1.3
    kw = dict(FULL) if taps else dict(weight_sp=0.1, rgb_patch=FULL['rgb_patch'])
    loss = ContextualLoss(taps, band_width=bw, loss_weight=lw, **kw).cuda()
    sd = _load_synth(loss)
    assert (loss.vgg is None) == (not taps)
    x, gt = _images(2, 48, 40, seed=48)
    val, grad, picks = _device(loss, x, gt, gup)
    assert len(picks) == len(taps) + 1                       # the RGB tap first, then the VGG taps in network order
    assert picks[0]['jmin'].shape == (2, 11 * 9) and (not taps or picks[1]['jmin'].shape == (2, 12 * 10))   # (relu2_2: 24 x 20 at stride 2)
    args = (sd, x, gt, taps, bw, lw)
    l64, g64, parts = _ref(*args, **kw)
    cx64 = [p['CX'].tolist() for p in parts]
    assert all(0.05 <= v <= 0.99 for t in cx64 for v in t), cx64
    differing = [(int((pk['jmin'] != p['jmin']).sum()), int((pk['imax'] != p['imax']).sum())) for pk, p in zip(picks, parts)]
    l64d, g64d, _ = _ref(*args, picks=picks, **kw)
    # the yardstick: the same restatement in torch fp32 on the GPU, against float64 through ITS selections
    l32, g32, parts32 = _ref(*args, dtype=torch.float32, device='cuda', **kw)
    picks32 = [{k: p[k].cpu() for k in ('jmin', 'imax')} for p in parts32]
    _, g64_32, _ = _ref(*args, picks=picks32, **kw)
    yard_loss = max(abs(float(l32) - float(l64)) / abs(float(l64)), ULP32)
    yard_grad = _rel_l2(g32, g64_32)
    loss_err = abs(float(val) - float(l64d)) / abs(float(l64d))
    grad_err = _rel_l2(grad, gup * g64d)
    print(f'{sorted(taps)} + rgb: loss {float(l64):.6f}, CX per tap {[[round(v, 3) for v in t] for t in cx64]}, differing (jmin, imax) per tap '
          f'{differing}; loss rel err {loss_err:.2e} (torch fp32 {yard_loss:.2e}), image gradient rel L2 err {grad_err:.2e} (torch fp32 '
          f'{yard_grad:.2e})')
    for (dj, di), p in zip(differing, parts):
        assert dj <= 0.005 * p['jmin'].numel() and di <= 0.005 * p['imax'].numel()
    assert val.dim() == 0 and loss_err <= 4 * yard_loss
    assert grad_err <= 4 * yard_grad
    # the terms are there: without them the loss is another number
    plain = ContextualLoss(taps, band_width=bw, loss_weight=lw, rgb_patch=FULL['rgb_patch']).cuda()
    _load_synth(plain)
    assert float(plain(x.cuda(), gt.cuda())) != float(val)


def test_norm_img_reaches_the_rgb_tap():
    """norm_img: (x + 1) * 0.5 on both images before the patches; the gradient carries the 0.5"""
    from mrefsr_amd.losses import ContextualLoss
    x, gt = _images(2, 24, 20, seed=3)
    a = ContextualLoss({}, rgb_patch=dict(size=3, stride=2), weight_sp=0.1).cuda()
    n = ContextualLoss({}, rgb_patch=dict(size=3, stride=2), weight_sp=0.1, norm_img=True).cuda()
    va, ga, _ = _device(a, x, gt)
    vn, gn, _ = _device(n, 2 * x - 1, 2 * gt - 1)
    # (2 x - 1 + 1) * 0.5 = x up to one rounding of the inputs: the values agree closely, the gradient is half
    assert abs(float(va) - float(vn)) <= 1e-4 * abs(float(va)) and _rel_l2(2 * gn, ga) <= 1e-3


def test_without_the_new_keys_the_bits_are_those_of_the_plain_calls():
    from mrefsr_amd import hip
    from mrefsr_amd.archs import nhwc_train
    from mrefsr_amd.losses import ContextualLoss
    bw, lw = 0.5, 0.8
    loss = ContextualLoss(TAPS, band_width=bw, loss_weight=lw).cuda()
    _load_synth(loss)
    x, gt = _images(2, 48, 40, seed=48)
    val, grad, _ = _device(loss, x, gt)
    explicit = ContextualLoss(TAPS, band_width=bw, loss_weight=lw, weight_sp=0.0, tap_stride={'relu2_2': 1}, rgb_patch=None).cuda()
    _load_synth(explicit)
    val_e, grad_e, _ = _device(explicit, x, gt)
    assert torch.equal(val, val_e) and torch.equal(grad, grad_e)
    # by hand: the VGG stack of the plan, hip.contextual_fwd / hip.contextual_bwd without weight_sp per tap
    plan, b = loss._plan, 2
    mean, std = loss.vgg.mean.contiguous(), loss.vgg.std.contiguous()
    feats, saved = nhwc_train._vgg_stack_forward(plan, torch.cat([x, gt]).cuda().contiguous(), mean, std)
    run, keep = None, []
    for (_, _, w), f in zip(plan.taps, feats):
        total, s = hip.contextual_fwd(f[:b], f[b:], bw, w, lw, run=run)
        run = s['run']
        keep.append(s)
    assert torch.equal(total.reshape(()), val)
    tap_of = {(i, k): j for j, (i, k, _) in enumerate(plan.taps)}

    def add_tap(g, i, kind):
        j = tap_of.get((i, kind))
        if j is None:
            return g, None
        acc = g is not None
        if g is None:
            g = torch.empty_like(keep[j]['xn'])
        return g, hip.contextual_bwd(keep[j], bw, lw * plan.taps[j][2], g, gup=torch.ones(1, device='cuda'), accumulate=acc)
    assert torch.equal(nhwc_train._vgg_stack_backward(plan, b, saved, std, add_tap), grad)


def test_a_tap_of_6400_positions_needs_a_stride():
    from mrefsr_amd.losses import ContextualLoss
    x, gt = _images(1, 160, 160, seed=7)
    refused = ContextualLoss({'relu2_2': 1.0}, weight_sp=0.1).cuda()
    _load_synth(refused)
    with pytest.raises(NotImplementedError, match=r'tap relu2_2 of 80 x 80 = 6400 positions.*4096.*tap_stride'):
        refused(x.cuda(), gt.cuda())
    with pytest.raises(NotImplementedError, match=r'tap rgb_patch of 78 x 78.*stride of rgb_patch'):
        ContextualLoss({}, rgb_patch=dict(size=5, stride=2)).cuda()(x.cuda(), gt.cuda())
    loss = ContextualLoss({'relu2_2': 1.0}, weight_sp=0.1, tap_stride={'relu2_2': 2}).cuda()
    _load_synth(loss)
    val, grad, picks = _device(loss, x, gt)
    assert picks[0]['jmin'].shape == (1, 1600) and bool(torch.isfinite(val)) and float(val) > 0
    assert grad.shape == x.shape and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0


def _opt(model_type='MultiRefRestorationModel', deterministic=False):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), total_iter=255000, warmup_iter=-1,
                 net_g_pretrain_steps=0, pixel_criterion='L1Loss', pixel_weight=1.0,
                 contextual_opt=dict(CX_OPT, tap_stride=dict(CX_OPT['tap_stride']), rgb_patch=dict(CX_OPT['rgb_patch'])))
    if deterministic:
        train['deterministic'] = True
    multi = model_type == 'MultiRefRestorationModel'
    return dict(
        name='cobi', model_type=model_type, scale=4, crop_border=4, num_gpu=1, manual_seed=10, is_train=True, dist=False, rank=0,
        network_g=dict(type='MRAPARestorationNet' if multi else 'RestorationNet', ngf=64, n_blocks=2, groups=8),
        network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                         vgg_type='vgg19'),
        network_extractor=dict(type='ContrasMultiExtractorSep' if multi else 'ContrasExtractorSep'),
        path=dict(pretrain_network_g=None, pretrain_network_feature_extractor=None, strict_load=True), train=train, val=dict(save_img=False))


def _built(opt):
    from mrefsr_amd.models import build_model
    torch.manual_seed(10)
    model = build_model(opt)
    for name in ('net_g', 'net_extractor', 'net_map'):
        _load_synth(model.get_bare_model(getattr(model, name)))
    _load_synth(model.cri_contextual)
    return model


def _data(key, k):
    samples = [synth.sr_sample(f'{key}/s{i}', k, LR_H, LR_W) for i in range(B)]
    data = {n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]}
    if k == 1:
        data['img_ref'] = data.pop('img_ref_list')[:, 0].contiguous()
    else:
        data['ref_valid'] = torch.tensor(VALID)
    return data


@pytest.mark.parametrize('model_type', ['MultiRefRestorationModel', 'RefRestorationModel'])
def test_model_step_with_the_full_option(model_type):
    model = _built(_opt(model_type))
    cri = model.cri_contextual
    assert (cri.weight_sp, cri.tap_stride, cri.rgb_patch) == (0.1, {'relu2_2': 2}, dict(size=5, stride=4, weight=1.0))
    model.feed_data(_data('cobi', K if model_type == 'MultiRefRestorationModel' else 1))
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert np.isfinite(log['l_g_contextual']) and log['l_g_contextual'] > 0
    assert log['l_g_contextual'] == float(cri(model.output.detach(), model.gt))         # bit for bit
    for n, p in model.get_bare_model(model.net_g).named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n


def test_deterministic_step_twice_gives_identical_bits():
    runs = []
    for _ in range(2):
        model = _built(_opt(deterministic=True))
        model.feed_data(_data('cobi', K))
        model.optimize_parameters(1)
        net = model.get_bare_model(model.net_g)
        runs.append((model.log_dict['l_g_contextual'].clone(), model.log_dict['l_g_pix'].clone(),
                     {n: p.grad.detach().clone() for n, p in net.named_parameters()},
                     {n: p.detach().clone() for n, p in net.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for n in runs[0][2]:
        assert torch.equal(runs[0][2][n], runs[1][2][n]), n
        assert torch.equal(runs[0][3][n], runs[1][3][n]), n
