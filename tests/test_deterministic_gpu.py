"""GPU: the deterministic mode -- net_g's three cross-block gradient reductions (act_bwd_nhwc, dynagg_prep_bwd_nhwc, the per-cout
sums of conv_nhwc_bwd) added in a fixed order under hip.deterministic(): repeated launches agree bit for bit, the sums are the
fp64 sums of the kernels' own element-wise outputs to fp32 rounding, the element-wise outputs are the default mode's bits; whole
training steps of two models built from one seed leave identical outputs, gradients, parameters and Adam moments.

Shapes, from the launchers' grid formulas (C = channels, blocks = the number of partial rows that are added in order):
  act_bwd_nhwc          256 / (C / V) pixels per block and pass (V = 4 when C % 4 == 0, else 1), 16 passes before another block is
                        added, at most 512 blocks.  C = 64: 7 px -> 1 block, 40^2 -> 7 (the last pass ragged), 2 x 192^2 -> 288 (more
                        than the 256 CUs), 4 x 196^2 -> 601 wanted, capped to 512.  C = 3: 7 px -> 1, 96^2 -> 7, 600^2 -> 265.
  dynagg_prep_bwd_nhwc  32-pixel tiles, groups = clamp(HW B / 16384, 1, 32) tiles per block, grid (ceil(HW / (32 groups)), B):
                        B 1, HW 31 -> 1 block (a ragged tile); B 2, 40 x 41 -> 2 x 52 (the last tile ragged); B 2, 96^2 -> 2 x 288
                        (more than the CUs); B 2, 160^2 -> groups 3, 2 x 267 (the last block one tile short).
  conv_nhwc_bwd         16 x 32-pixel tiles x 64 couts; <= 128 such blocks -> 4-row tiles, <= 256 -> 8-row tiles.  1 x 4 x 8 -> 1 block;
                        2 x 48^2 -> 48 blocks of 4 rows (ragged right column); 1 x 16 x 70, 128 couts -> two cout blocks; 4 x 160^2 ->
                        400 blocks of 8 rows (more than the CUs, blocks re-labelled per XCD); 6 x 160^2 -> 300 blocks of 16 rows.
The bound of an n-term fp32 sum in any order, n 2^-24 sum |addend|, is computed per channel from the data."""
import numpy as np
import pytest
import torch

import synth
from conftest import spec_from

pytestmark = pytest.mark.gpu

REPEATS = 5


def _bound(addends, dims):
    """n 2^-24 sum |a| per channel, in fp64"""
    a = addends.double()
    n = a.numel() // a.shape[-1] if dims is None else int(np.prod([a.shape[d] for d in dims]))
    return n * 2.0 ** -24 * a.abs().sum(dims if dims is not None else tuple(range(a.dim() - 1)))


def _check_sums(name, runs, default, addends, dims=None):
    """runs: the sums of REPEATS deterministic launches; default: the default mode's; addends [..., C]: the kernel's own output"""
    dims = tuple(range(addends.dim() - 1)) if dims is None else dims
    want = addends.double().sum(dims)
    bound = _bound(addends, dims)
    for r in runs[1:]:
        assert torch.equal(r, runs[0]), f'{name}: two deterministic launches differ'
    err = (runs[0].double() - want).abs()
    gap = (runs[0].double() - default.double()).abs()
    print(f'{name}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3g}, vs default / bound '
          f'{float((gap / bound.clamp_min(1e-300)).max()):.3g}')
    assert bool((err <= bound).all()), f'{name}: deterministic sum off the fp64 sum by more than n 2^-24 sum|a|'
    assert bool((gap <= bound).all()), f'{name}: deterministic and default sums further apart than n 2^-24 sum|a|'


# ------------------------------------------------------------------ act_bwd_nhwc
ACT_CASES = [(7, 64, 1), (1600, 64, 7), (73728, 64, 288), (153664, 64, 512), (7, 3, 1), (9216, 3, 7), (360000, 3, 265)]


def _act_inputs(npix, c, act):
    torch.manual_seed(npix + c + act)
    g = torch.randn(npix, c, device='cuda') * 1e-3
    out = torch.randn(npix, c, device='cuda') if act else None
    if act == 2:   # a PReLU output: negative values are slope * x
        out = torch.where(out > 0, out, out * 0.25)
    slope_ptr = torch.full((1,), 0.25, device='cuda') if act == 2 else None
    return g, out, slope_ptr


@pytest.mark.parametrize('act', [0, 1, 2], ids=['none', 'lrelu', 'prelu'])
@pytest.mark.parametrize('npix,c,blocks', ACT_CASES, ids=lambda v: str(v))
def test_act_bwd_sums_are_reproducible_and_right(npix, c, blocks, act):
    from mrefsr_amd import _lib, hip
    assert _lib.load().mrefsr_act_bwd_blocks(npix, c) == blocks
    g, out, slope_ptr = _act_inputs(npix, c, act)
    call = lambda: hip.act_bwd_nhwc(g, out, act, 0.2 if act == 1 else 0.0, slope_ptr, want_bias=True, want_amax=True)   # noqa: E731
    pre0, bias0, slope0, amax0 = call()
    with hip.deterministic():
        runs = [call() for _ in range(REPEATS)]
    for pre, _, _, amax in runs:
        assert torch.equal(pre[..., :c], pre0[..., :c]) and torch.equal(amax, amax0)      # element-wise output and max |g|: the same bits
    _check_sums(f'act_bwd bias {npix}x{c} act{act}', [r[1] for r in runs], bias0, runs[0][0][..., :c])
    if act == 2:   # the slope gradient: sum of g * x over x < 0, x = out / slope
        x = out * 4.0                                     # out / slope, exact for slope = 0.25
        addends = torch.where(out > 0, torch.zeros_like(g).double(), g.double() * x.double()).reshape(-1, 1)
        _check_sums(f'act_bwd slope {npix}x{c}', [r[2] for r in runs], slope0, addends)
    else:
        assert all(r[2] is None for r in runs)


# ------------------------------------------------------------------ dynagg_prep_bwd_nhwc
DYN_CASES = [(1, 1, 31, 1), (2, 40, 41, 104), (2, 96, 96, 576), (2, 160, 160, 534)]


@pytest.mark.parametrize('dg', [8, 1], ids=['dg8', 'dg1'])
@pytest.mark.parametrize('b,h,w,blocks', DYN_CASES, ids=lambda v: str(v))
def test_dynagg_prep_bwd_bias_gradient_is_reproducible_and_right(b, h, w, blocks, dg):
    from mrefsr_amd import _lib, hip
    assert _lib.load().mrefsr_dynagg_prep_bwd_blocks(b, dg, h, w) == blocks
    torch.manual_seed(b * h * w + dg)
    g_off = torch.randn(b, 18 * dg, h, w, device='cuda') * 1e-4
    g_m = torch.randn(b, 9 * dg, h, w, device='cuda') * 1e-3
    mask = torch.rand(b, 9 * dg, h, w, device='cuda')
    g_om0, bias0, amax0 = hip.dynagg_prep_bwd_nhwc(g_off, g_m, mask, dg)
    with hip.deterministic():
        runs = [hip.dynagg_prep_bwd_nhwc(g_off, g_m, mask, dg) for _ in range(REPEATS)]
        g_om1, bias1, _ = hip.dynagg_prep_bwd_nhwc(g_off, g_m, mask, dg, want_bias=False)
    assert bias1 is None and torch.equal(g_om1, g_om0)
    for g_om, _, amax in runs:
        assert torch.equal(g_om, g_om0) and torch.equal(amax, amax0)
    _check_sums(f'dynagg bias b{b} {h}x{w} dg{dg}', [r[1] for r in runs], bias0, g_om0)


# ------------------------------------------------------------------ conv_nhwc_bwd (stat_sum)
CONV_CASES = [(1, 4, 8, 64), (1, 8, 8, 64), (2, 48, 48, 64), (1, 16, 70, 128), (4, 160, 160, 64), (6, 160, 160, 64)]


@pytest.mark.parametrize('n,h,w,c', CONV_CASES, ids=lambda v: str(v))
def test_conv_bwd_channel_sums_are_reproducible_and_right(n, h, w, c):
    from mrefsr_amd import hip
    torch.manual_seed(n * h * w + c)
    g = torch.randn(n, h, w, c, device='cuda') * 1e-5
    t = torch.randn(n, h, w, c, device='cuda')          # the forward activation whose sign is the ReLU mask
    skip = torch.randn(n, h, w, c, device='cuda') * 1e-5
    wt = torch.randn(c, c, 3, 3, device='cuda') * 0.05
    amax = g.abs().max().reshape(1)
    pk = hip.conv_pack_view(wt, None, 16, dgrad=True, wscale=2.0 ** 12)
    for what, kw in (('mask', dict(residual=t, residual_is_mask=True)), ('skip', dict(residual=skip))):
        out0, sum0, amax0 = hip.conv_nhwc_bwd(g, pk, c, 3, in_amax=amax, **kw)
        with hip.deterministic():
            runs = [hip.conv_nhwc_bwd(g, pk, c, 3, in_amax=amax, **kw) for _ in range(REPEATS)]
            out1, sum1, amax1 = hip.conv_nhwc_bwd(g, pk, c, 3, in_amax=amax, want_stats=False, **kw)
        assert sum1 is None and amax1 is None and torch.equal(out1, out0)
        for out, _, am in runs:
            assert torch.equal(out, out0) and torch.equal(am, amax0)
        _check_sums(f'conv_bwd {what} {n}x{h}x{w}x{c}', [r[1] for r in runs], sum0, out0)
    hip.check_conv_range()


# ------------------------------------------------------------------ captured and replayed
def _wgrad_close(got, want):
    """the assertion of test_train_engine_gpu.test_batched_wgrad_equals_the_single_launches for this wrapper"""
    err = float((got.double() - want.double()).abs().max()) / (float(want.double().abs().max()) + 1e-30)
    assert err <= 2e-6, err


def test_ticket_resets_itself_across_eager_launches_and_graph_replays():
    """one ticket word per stream serves every launch: five eager launches above already share it; here one linear capture of the
    three reductions and of a weight gradient (its partial tiles in the same cached scratch) is replayed twice and gives the eager
    deterministic bits each time; the capture's cached buffers are listed while the graph lives and gone once they are released"""
    from mrefsr_amd import hip
    npix, c = 73728, 64                                   # 288 blocks
    g, out, slope_ptr = _act_inputs(npix, c, 2)
    torch.manual_seed(3)
    g_off = torch.randn(2, 18 * 8, 96, 96, device='cuda') * 1e-4
    g_m = torch.randn(2, 9 * 8, 96, 96, device='cuda') * 1e-3
    mask = torch.rand(2, 9 * 8, 96, 96, device='cuda')
    gc = torch.randn(2, 48, 48, 64, device='cuda') * 1e-5
    tc = torch.randn(2, 48, 48, 64, device='cuda')
    amax = gc.abs().max().reshape(1)
    pk = hip.conv_pack_view(torch.randn(64, 64, 3, 3, device='cuda') * 0.05, None, 16, dgrad=True, wscale=2.0 ** 12)
    xw = torch.randn(1, 16, 16, 16, device='cuda')        # the smallest weight gradient with a partial tile and a reduction
    gw = torch.randn(1, 16, 16, 16, device='cuda') * 1e-3
    amax_w = gw.abs().max().reshape(1)

    def body():
        _, bias, slope, _ = hip.act_bwd_nhwc(g, out, 2, 0.0, slope_ptr, want_bias=True, want_amax=True)
        _, dyn, _ = hip.dynagg_prep_bwd_nhwc(g_off, g_m, mask, 8)
        _, csum, _ = hip.conv_nhwc_bwd(gc, pk, 64, 3, residual=tc, residual_is_mask=True, in_amax=amax)
        return bias, slope, dyn, csum, hip.conv_wgrad3x3(xw, gw, 16, 16, amax_w)

    def check(got, want):
        for a, b in zip(got[:4], want[:4]):
            assert torch.equal(a, b)
        _wgrad_close(got[4], want[4])

    with hip.deterministic():
        want = [t.clone() for t in body()]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = body()
        keep = hip.capture_refs()                         # the scratch, the ticket and the zero chunk the graph baked in
        assert len(keep) >= 3
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            check(got, want)
        check(body(), want)                               # and the eager stream's ticket is still good
    del graph, keep
    hip.release_capture_workspaces()
    assert len(hip.capture_refs()) == 0 and hip.capture_ptrs() == ()
    with hip.deterministic():
        check(body(), want)
    hip.check_conv_range()


def test_eager_regrowth_leaves_a_captured_graph_alone():
    """an eager call that regrows the eager stream's scratch moves nothing the graph baked in: capture_ptrs() is unchanged (the
    training graph's owner would recapture otherwise) and a replay still gives the eager bits"""
    from mrefsr_amd import hip
    g, out, slope_ptr = _act_inputs(4096, 64, 2)
    call = lambda: hip.act_bwd_nhwc(g, out, 2, 0.0, slope_ptr, want_bias=True, want_amax=True)   # noqa: E731
    wgrad = lambda x, gr: hip.conv_wgrad3x3(x, gr, x.shape[3], x.shape[3], gr.abs().max().reshape(1))   # noqa: E731
    torch.manual_seed(5)
    small = [torch.randn(1, 16, 16, 16, device='cuda') for _ in range(2)]
    large = [torch.randn(2, 32, 32, 64, device='cuda') for _ in range(2)]
    with hip.deterministic():
        want = [t.clone() for t in call()]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = call()
        keep, ptrs = hip.capture_refs(), hip.capture_ptrs()
        assert len(keep) >= 3 and len(ptrs) == len(keep)
        hip._scratch_bufs.entries.pop(hip._scratch_bufs.key(g.device), None)   # (whatever size earlier tests left: start at the floor)
        wgrad(*small)
        before = hip._scratch(g.device, 1)
        dw = wgrad(*large)
        assert hip._scratch(g.device, 1) is not before, 'the second weight gradient was meant to regrow the eager scratch'
        assert hip.capture_ptrs() == ptrs
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    want_dw = torch.nn.grad.conv2d_weight(large[0].permute(0, 3, 1, 2).double(), (64, 64, 3, 3), large[1].permute(0, 3, 1, 2).double(), padding=1)
    assert float((dw.double() - want_dw).abs().max()) <= 2e-5 * float(want_dw.abs().max())   # (the regrown scratch serves its call)
    del graph, keep
    hip.release_capture_workspaces()
    hip.check_conv_range()


# ------------------------------------------------------------------ whole steps
def _opt(deterministic, percep=None):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000, 400000], gamma=0.5), total_iter=255000, warmup_iter=-1,
                 net_g_pretrain_steps=0, pixel_criterion='L1Loss', pixel_weight=1.0)
    if deterministic:
        train['deterministic'] = True
    if percep is not None:
        train['perceptual_opt'] = percep
    return dict(
        name='det', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, manual_seed=10, is_train=True,
        dist=False, rank=0, network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=2, groups=8),
        network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                         vgg_type='vgg19'),
        network_extractor=dict(type='ContrasMultiExtractorSep'),
        path=dict(pretrain_network_g=None, pretrain_network_feature_extractor=None, strict_load=True), train=train, val=dict(save_img=False))


def _batches(lr_h, lr_w):
    out = []
    for it in range(3):
        samples = [synth.sr_sample(f'det/{lr_h}x{lr_w}/b{it}/s{i}', 2, lr_h, lr_w) for i in range(2)]
        out.append({n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]})
    return out


def _three_steps(batches, deterministic, percep_golden=None):
    """a model from one seed, the same three batches: per step (output, gradients), then parameters and both Adam moments"""
    from mrefsr_amd.models import build_model
    percep = None
    if percep_golden is not None:
        layers = dict(zip([str(v) for v in percep_golden['layer_names']], [float(v) for v in percep_golden['layer_weights']]))
        percep = dict(layer_weights=layers, vgg_type='vgg19', use_input_norm=True, perceptual_weight=float(percep_golden['perceptual_weight']),
                      style_weight=0.0, norm_img=True, criterion='l1')
    torch.manual_seed(10)
    model = build_model(_opt(deterministic, percep))
    for name in ('net_g', 'net_extractor', 'net_map'):   # synthetic weights (a fresh MRAPARestorationNet has zero offsets convolutions)
        net = model.get_bare_model(getattr(model, name))
        spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()})
    if percep_golden is not None:   # the random-initialised VGG19 of the perceptual tests
        vsd = synth.state_dict(spec_from(percep_golden, 'vgg_'))
        model.cri_perceptual.load_state_dict({k: torch.from_numpy(v) for k, v in vsd.items()}, strict=True)
    params = dict(model.get_bare_model(model.net_g).named_parameters())
    steps = []
    for it, data in enumerate(batches, 1):
        model.feed_data(data)
        model.optimize_parameters(it)
        assert all(p.grad is not None for p in params.values())
        steps.append((model.output.detach().clone(), {n: p.grad.detach().clone() for n, p in params.items()}))
    state = model.optimizer_g.state
    final = {n: (p.detach().clone(), state[p]['exp_avg'].clone(), state[p]['exp_avg_sq'].clone()) for n, p in params.items()}
    return steps, final


def _assert_same_run(a, b):
    (steps_a, final_a), (steps_b, final_b) = a, b
    for it, ((out_a, g_a), (out_b, g_b)) in enumerate(zip(steps_a, steps_b), 1):
        assert torch.equal(out_a, out_b), f'step {it}: outputs differ'
        for n in g_a:
            assert torch.equal(g_a[n], g_b[n]), f'step {it}: gradient of {n} differs'
    for n in final_a:
        for what, x, y in zip(('parameter', 'exp_avg', 'exp_avg_sq'), final_a[n], final_b[n]):
            assert torch.equal(x, y), f'{what} of {n} differs after the last step'


@pytest.mark.parametrize('lr', [(24, 24), (22, 26)], ids=['lr24x24', 'lr22x26_pad_crop'])
def test_two_runs_from_one_seed_are_bit_identical(lr):
    """B = 2, K = 2, pixel loss, train.deterministic: true"""
    batches = _batches(*lr)
    _assert_same_run(_three_steps(batches, True), _three_steps(batches, True))


def test_two_runs_with_a_perceptual_loss_are_bit_identical(golden):
    batches = _batches(24, 24)
    g = golden('e2e_c2_percep')
    _assert_same_run(_three_steps(batches, True, g), _three_steps(batches, True, g))


def test_torchs_global_flag_alone_turns_the_mode_on():
    """torch.use_deterministic_algorithms(True) and no option"""
    from mrefsr_amd import hip
    batches = _batches(24, 24)
    before, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        assert hip.is_deterministic()
        a = _three_steps(batches, False)
        b = _three_steps(batches, False)
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn)
    _assert_same_run(a, b)


# ------------------------------------------------------------------ the DCN input gradient has no fixed-order form
def test_dcn_input_gradient_is_refused_under_the_switch():
    from mrefsr_amd import hip
    from mrefsr_amd.ops.dcn import modulated_deform_conv
    torch.manual_seed(0)
    b, c, co, dg, h, w = 1, 32, 32, 4, 9, 11
    x = torch.randn(b, c, h, w, device='cuda')
    offset = torch.randn(b, 18 * dg, h, w, device='cuda')
    mask = torch.rand(b, 9 * dg, h, w, device='cuda')
    weight = torch.randn(co, c, 3, 3, device='cuda') * 0.05
    bias = torch.zeros(co, device='cuda')

    def backward(x_grad, w_grad=True):
        xs = x.clone().requires_grad_(x_grad)
        ws = weight.clone().requires_grad_(w_grad)
        modulated_deform_conv(xs, offset, mask, ws, bias, 1, 1, 1, 1, dg).sum().backward()
        return xs.grad, ws.grad

    gx0, gw0 = backward(True)                             # switch off: as before
    assert gx0 is not None and gw0 is not None
    before, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    with hip.deterministic():
        with pytest.raises(RuntimeError, match='does not have a deterministic implementation'):
            backward(True)
        gx, gw = backward(False)                          # without the input gradient the backward runs
        assert gx is None and gw is not None
        try:
            torch.use_deterministic_algorithms(True, warn_only=True)
            with pytest.warns(UserWarning, match='does not have a deterministic implementation'):
                gx, _ = backward(True)
            assert gx is not None
        finally:
            torch.use_deterministic_algorithms(before, warn_only=warn)
