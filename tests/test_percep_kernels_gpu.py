"""GPU: the kernels of the perceptual / style loss (csrc/percep.hip) against torch on the same tensors (bit for bit where torch's
arithmetic is restated) and against fp64 (Gram products)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _pool_input(n, c, h, w, seed):
    """values with exact ties: small integers, a share of the windows all zero (post-ReLU), equal positive maxima"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (n, c, h, w), generator=g).float()
    x = torch.relu(x)
    x[:, :, :4, :4] = 0.0                      # all-zero windows
    x[:, :c // 2, 4:8, 4:8] = 2.0              # equal positive maxima in every window
    return x.cuda()


@pytest.mark.parametrize('shape', [(2, 64, 16, 20), (2, 128, 11, 13), (1, 512, 5, 7), (3, 8, 10, 2)])
@pytest.mark.parametrize('plane', [False, True])
def test_maxpool_forward_backward_bit_equal_to_torch(shape, plane):
    from mrefsr_amd import hip
    n, c, h, w = shape
    x = _pool_input(n, c, h, w, 1 + h)
    pre = (x - 1.0).clone()                    # a pre-activation map: the kernel applies the ReLU itself
    for inp, relu in ((x, False), (pre, True)):
        src = inp.clone().requires_grad_(True)
        want = F.max_pool2d(torch.relu(src) if relu else src, 2, 2)
        got, pl = hip.maxpool2_nhwc(_nhwc(inp), relu=relu, want_plane=plane)
        assert torch.equal(got, _nhwc(want.detach()))
        gout = torch.randn(want.shape, generator=torch.Generator().manual_seed(3)).cuda()
        (want * gout).sum().backward()
        # torch: max_pool2d backward then (relu) threshold_backward; the kernel: the two fused, ReLU mask from the map
        ref = src.grad if relu else src.grad * (x > 0)
        g_in, amax = hip.maxpool2_bwd_nhwc(_nhwc(gout), None if plane else _nhwc(inp), pl, relu=relu, mask=True, shape=(n, h, w, c))
        assert torch.equal(g_in, _nhwc(ref))
        assert float(amax) == float(ref.abs().max())


def test_tap_criterion_gradient_bit_equal_and_loss_to_1e6():
    """((l1(x_k, y_k) * w_k) * weight) through torch autograd on the same features (ref losses.py:203-213); the loss of several taps in
    one launch within 1e-6 of fp64, twice the same bits"""
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(7)
    shapes = [(2, 160, 160, 64), (2, 40, 40, 256), (2, 10, 10, 512)]
    xs = [torch.randn(s, generator=g).cuda() for s in shapes]
    ys = [(x.cpu() + 0.3 * torch.randn(x.shape, generator=g)).cuda() for x in xs]
    ys[0].view(-1)[:1000] = xs[0].view(-1)[:1000]      # exact zeros of x - y: sgn 0
    ws, pw = [0.1, 1.0, 0.75], 1.7
    losses, totals = hip.tap_crit_loss(xs, ys, ws, [0, 0, 0], 'l1', (pw, 0.0))
    losses2, totals2 = hip.tap_crit_loss(xs, ys, ws, [0, 0, 0], 'l1', (pw, 0.0))
    assert torch.equal(losses, losses2) and torch.equal(totals, totals2)
    want = [float((x.double() - y.double()).abs().mean()) for x, y in zip(xs, ys)]
    np.testing.assert_allclose(losses.cpu().numpy(), want, rtol=1e-6)
    assert abs(float(totals[0]) - sum(a * b for a, b in zip(want, ws)) * pw) <= 1e-6 * abs(float(totals[0]))
    gup = torch.tensor([0.5, 0.0], device='cuda')
    for k, (x, y, w) in enumerate(zip(xs, ys, ws)):
        xr = x.clone().requires_grad_(True)
        loss = 0
        loss += F.l1_loss(xr, y) * w
        loss *= pw
        loss.backward(gup[0])
        base = torch.randn(x.shape, generator=g).cuda()
        gr = base.clone()
        amax = hip.tap_crit_grad(x, y, gr, w, 0, 'l1', (pw, 0.0), gup=gup, accumulate=True)
        assert torch.equal(gr, base + xr.grad), k
        assert float(amax) == float(gr.abs().max())
        fresh = torch.empty_like(x)
        hip.tap_crit_grad(x, y, fresh, w, 0, 'l1', (pw, 0.0), gup=gup)
        assert torch.equal(fresh, xr.grad), k


def test_tap_criterion_frobenius():
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 20, 20, 512, generator=g).cuda()
    y = torch.randn(2, 20, 20, 512, generator=g).cuda()
    losses, totals = hip.tap_crit_loss([x], [y], [0.5], [0], 'fro', (2.0, 0.0))
    want = float(torch.linalg.vector_norm(x.double() - y.double()))
    assert abs(float(losses[0]) - want) <= 1e-6 * want
    xd = x.double().clone().requires_grad_(True)
    (torch.norm(xd - y.double(), p='fro') * 0.5 * 2.0).backward()
    gr = torch.empty_like(x)
    hip.tap_crit_grad(x, y, gr, 0.5, 0, 'fro', (2.0, 0.0), norm=losses[0:1])
    err = float((gr.double() - xd.grad).norm() / xd.grad.norm())
    assert err <= 1e-6, err


# (channels, h, w): every VGG19 stage at GT 160 x 160, the odd 40 x 56 case's last stages, and each channel count
GRAM_CASES = [(64, 160, 160), (128, 80, 80), (256, 40, 40), (512, 20, 20), (512, 10, 10), (512, 5, 7), (64, 3, 3), (256, 2, 3)]


@pytest.mark.parametrize('c,h,w', GRAM_CASES)
def test_gram_and_its_backward_against_fp64(c, h, w):
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(c + h)
    n = 4
    f = torch.relu(torch.randn(n, h, w, c, generator=g)).cuda()
    fg = torch.relu(torch.randn(n, h, w, c, generator=g)).cuda()
    gram = hip.gram_nhwc(f)
    fd = f.double().reshape(n, h * w, c)
    want = fd.transpose(1, 2) @ fd / (c * h * w)
    assert torch.equal(gram, gram.transpose(1, 2))                       # upper tiles mirrored: exactly symmetric
    err = float((gram.double() - want).abs().max() / want.abs().max())
    assert err <= 1e-5, err
    assert torch.equal(gram, hip.gram_nhwc(f))                          # fixed summation order
    gg = hip.gram_nhwc(fg)
    # d/dF of ((l1(gram(F), gram(Fg)) * w) * sw) * gup: the style term of ref losses.py:216-226 in fp64 -- with the l1 derivative's
    # sign taken from the Gram matrices the kernel is given (an fp64 Gram would flip the sign of the near-ties: at c = 512, hw = 100
    # such flips alone move dF by ~1 %; the model-level effect is measured by tests/test_percep_train_gpu.py)
    wk, sw, up = 0.8, 30.0, 0.5
    fr = f.double().reshape(n, h * w, c).transpose(1, 2).clone().requires_grad_(True)    # [n, c, hw] as the reference's view
    gx = fr.bmm(fr.transpose(1, 2)) / (c * h * w)
    sgn = torch.sign(gram.double() - gg.double())
    ((gx * sgn).sum() / sgn.numel() * wk * sw * up).backward()
    want_df = fr.grad.transpose(1, 2).reshape(n, h, w, c)
    base = torch.randn(n, h, w, c, generator=g).cuda() * float(want_df.abs().max())
    df = base.clone()
    amax = hip.gram_bwd_nhwc(f, gram, gg, df, sw, wk, gup=torch.tensor([up], device='cuda'), accumulate=True)
    err = float((df.double() - base.double() - want_df).abs().max() / want_df.abs().max())
    assert err <= 1e-5, err
    assert float(amax) == float(df.abs().max())
    fresh = torch.empty_like(f)
    hip.gram_bwd_nhwc(f, gram, gg, fresh, sw, wk, gup=torch.tensor([up], device='cuda'))
    err = float((fresh.double() - want_df).abs().max() / want_df.abs().max())
    assert err <= 1e-5, err


@pytest.mark.parametrize('norm_img,use_std', [(True, True), (False, True), (True, False)])
def test_image_packing_backward_bit_equal(norm_img, use_std):
    from mrefsr_amd import hip
    g = torch.Generator().manual_seed(11)
    x = torch.rand(3, 3, 24, 40, generator=g).cuda().requires_grad_(True)
    mean = torch.tensor([0.485, 0.456, 0.406], device='cuda').view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device='cuda').view(1, 3, 1, 1)
    y = (x + 1.) * 0.5 if norm_img else x
    if use_std:
        y = (y - mean) / std
    g4 = torch.randn(3, 24, 40, 4, generator=g).cuda()
    (y * g4[..., :3].permute(0, 3, 1, 2)).sum().backward()
    got = hip.image_to_nhwc4_bwd(g4, norm_img, std if use_std else None)
    assert torch.equal(got, x.grad)
