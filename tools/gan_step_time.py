#!/usr/bin/env python3
"""What the adversarial term adds to a training step.

  python tools/gan_step_time.py [--steps 10] [--warmup 3] [--out FILE.json] [--trace]
                                [--network-d {ImageDiscriminator,VGGStyleDiscriminator,UNetDiscriminatorSN,StyleGAN2Discriminator}] [--out-size 128]

(1) MultiRefRestorationModel.optimize_parameters at B = 4, K = 5, LR 40 x 40 (GT 160 x 160) in three configurations -- L1 only,
L1 + ImageDiscriminator(3, 32) with WGAN-GP (gan_weight 1e-3, grad_penalty_weight 10), L1 + vanilla GAN -- ms per step (median of
--steps, after --warmup);
(2) the discriminator part alone on [4,3,160,160] images: the WGAN-GP D step (D on real and fake, the penalty, backward) and the G
step's D forward + backward, on the HIP kernels;
(3) for comparison, the same D step through torch's NCHW autograd of the same module (MIOpen convolutions) on the same GPU.
--network-d: the discriminator of (1)-(3): ImageDiscriminator(3, 32) (the default), VGGStyleDiscriminator(3, 64) or
UNetDiscriminatorSN(3, 64) (whose torch counterpart in (3) calls the conv modules, so torch's spectral_norm hooks run the power
iteration), for the last two of which (4) also times every convolution launch of the discriminator (forward, input gradient, weight
gradient) at B = 4, 160 x 160, as ms and TF/s.
StyleGAN2Discriminator(out_size = --out-size, 128 or 256) runs (1)-(3) at LR out_size / 4 (its input is out_size x out_size); its torch
counterpart in (3) is the module tree's own forward on the package's generic ops (MIOpen convolutions, ops.upfirdn2d, ops.fused_act),
which (1) also times as the whole WGAN-GP step (step_ms_wgan_gp_torch_miopen); (4) times every stage of conv_body.
--trace: one WGAN-GP step only (for rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

GAN = {'wgan_gp': dict(gan_type='wgan', gan_weight=1e-3, grad_penalty_weight=10.0),
       'vanilla': dict(gan_type='vanilla', gan_weight=1e-3, grad_penalty_weight=0.0)}


NETWORK_D = {'ImageDiscriminator': dict(type='ImageDiscriminator', in_nc=3, ndf=32),
             'VGGStyleDiscriminator': dict(type='VGGStyleDiscriminator', num_in_ch=3, num_feat=64),
             'UNetDiscriminatorSN': dict(type='UNetDiscriminatorSN', num_in_ch=3, num_feat=64),
             'StyleGAN2Discriminator': dict(type='StyleGAN2Discriminator', out_size=128)}


def _net_d_opt(network_d, size):
    """the network_d option; StyleGAN2Discriminator's out_size is the image size"""
    opt = dict(NETWORK_D[network_d])
    if network_d == 'StyleGAN2Discriminator':
        opt['out_size'] = size
    return opt


def _opt(gan, network_d='ImageDiscriminator', size=160):
    train = dict(lr_g=1e-4, lr_offset=1e-4, lr_relu2_offset=1e-5, lr_relu3_offset=1e-6, weight_decay_g=0, beta_g=[0.9, 0.999],
                 scheduler=dict(type='MultiStepLR', milestones=[300000], gamma=0.5), net_g_pretrain_steps=0, pixel_criterion='L1Loss',
                 pixel_weight=1.0)
    opt = dict(name='gan_time', model_type='MultiRefRestorationModel', scale=4, crop_border=4, num_gpu=1, is_train=True, dist=False,
               network_g=dict(type='MRAPARestorationNet', ngf=64, n_blocks=16, groups=8),
               network_map=dict(type='CorrespondenceGenerationArch', patch_size=3, stride=1, vgg_layer_list=['relu1_1', 'relu2_1', 'relu3_1'],
                                vgg_type='vgg19'),
               network_extractor=dict(type='ContrasMultiExtractorSep'), path={}, train=train)
    if gan:
        train.update(GAN[gan], lr_d=1e-4, beta_d=[0.9, 0.999])
        opt['network_d'] = _net_d_opt(network_d, size)
    return opt


def _model(gan, network_d='ImageDiscriminator', lr=40):
    import synth
    import synth_disc
    import synth_sg2disc
    import synth_unetdisc
    import synth_vggdisc
    from mrefsr_amd.models import build_model
    model = build_model(_opt(gan, network_d, 4 * lr))
    nets = [model.get_bare_model(model.net_g), model.net_extractor, model.net_map]
    for net in nets:
        spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()})
    if gan:
        spec = [(k, tuple(v.shape)) for k, v in model.net_d.state_dict().items()]
        sd = {'VGGStyleDiscriminator': synth_vggdisc, 'UNetDiscriminatorSN': synth_unetdisc,
              'StyleGAN2Discriminator': synth_sg2disc}.get(network_d, synth_disc).state_dict(spec)
        model.net_d.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    samples = [synth.sr_sample(f'gan_time/s{i}', 5, lr, lr) for i in range(4)]
    model.feed_data({n: torch.from_numpy(np.stack([s[n] for s in samples])) for n in samples[0]})
    return model


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def _d_step(net, real, fake, gan, gp):
    for p in net.parameters():
        p.grad = None
    loss = gan(net(real), True, is_disc=True) + gan(net(fake), False, is_disc=True) + gp(net, real, fake)
    loss.backward()


def _torch_d(net):
    """the same module run through torch's own NCHW autograd (MIOpen convolutions, native BatchNorm)"""
    if hasattr(net, 'sn_convs'):   # UNetDiscriminatorSN: the reference's forward, the conv modules' spectral-norm hooks included
        def unet(x):
            def up(t):
                return F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False)
            x0 = F.leaky_relu(net.conv0(x), 0.2)
            x1 = F.leaky_relu(net.conv1(x0), 0.2)
            x2 = F.leaky_relu(net.conv2(x1), 0.2)
            x3 = F.leaky_relu(net.conv3(x2), 0.2)
            x4 = F.leaky_relu(net.conv4(up(x3)), 0.2) + x2
            x5 = F.leaky_relu(net.conv5(up(x4)), 0.2) + x1
            x6 = F.leaky_relu(net.conv6(up(x5)), 0.2) + x0
            return net.conv9(F.leaky_relu(net.conv8(F.leaky_relu(net.conv7(x6), 0.2)), 0.2))
        return unet
    if hasattr(net, 'conv_body'):   # StyleGAN2Discriminator: the reference's forward over the module tree (generic ops)
        def sg2(x):
            out = net.conv_body(x)
            b, c, h, w = out.shape
            group = min(b, net.stddev_group)
            sd = torch.sqrt(out.view(group, -1, 1, c, h, w).var(0, unbiased=False) + 1e-8)
            sd = sd.mean([2, 3, 4], keepdims=True).squeeze(2).repeat(group, 1, h, w)
            return net.final_linear(net.final_conv(torch.cat([out, sd], 1)).view(b, -1))
        return sg2
    if hasattr(net, 'conv_bn_layers'):   # VGGStyleDiscriminator: its own forward is the reference's, written out
        def vgg(x):
            h = F.leaky_relu(net.conv0_0(x), 0.2)
            for conv, bn in net.conv_bn_layers():
                h = F.leaky_relu(bn(conv(h)), 0.2)
            return net.linear2(F.leaky_relu(net.linear1(h.reshape(h.shape[0], -1)), 0.2))
        return vgg

    def fwd(x):
        h = x
        for blk in net.blocks():
            for i in (0, 3):
                h = F.leaky_relu(blk[i + 1](blk[i](h)), 0.2)
        return net.out_block(h)
    return fwd


def _vgg_shapes(nf=64):
    out, cin, h = [], 4, 160
    chans = [nf, nf, 2 * nf, 2 * nf, 4 * nf, 4 * nf, 8 * nf, 8 * nf, 8 * nf, 8 * nf]
    for i, c in enumerate(chans):
        ks = 3 if i % 2 == 0 else 4
        out.append((f'conv{i // 2}_{i % 2}', ks, cin, c, h))
        cin, h = c, (h // 2 if ks == 4 else h)
    return out


def _unet_shapes(nf=64):
    return [('conv0', 3, 4, nf, 160), ('conv1', 4, nf, 2 * nf, 160), ('conv2', 4, 2 * nf, 4 * nf, 80), ('conv3', 4, 4 * nf, 8 * nf, 40),
            ('conv4', 3, 8 * nf, 4 * nf, 40), ('conv5', 3, 4 * nf, 2 * nf, 80), ('conv6', 3, 2 * nf, nf, 160), ('conv7', 3, nf, nf, 160),
            ('conv8', 3, nf, nf, 160), ('conv9', 3, nf, 1, 160)]


def _conv_layers(shapes, steps, warmup, b=4):
    """ms and TF/s of every convolution launch of a discriminator at [b,3,160,160] (forward, input and weight gradient); shapes:
    (name, ks, Cin, Cout, input size); Cout 1 is conv9's kernels"""
    from mrefsr_amd import hip
    out = []
    for name, ks, cin, c, h in shapes:
        x = torch.randn(b, h, h, cin, device='cuda')
        w = torch.randn(c, cin, ks, ks, device='cuda') * 0.05
        ho = h // 2 if ks == 4 else h
        dy = torch.randn(b, ho, ho, c, device='cuda')
        flop = 2.0 * b * ho * ho * c * cin * ks * ks
        row = dict(layer=name, ks=ks, cin=cin, cout=c, out=ho, gflop=flop / 1e9)
        if c == 1:
            fns = (('fwd', lambda: hip.disc_conv9(x, w, None)), ('dgrad', lambda: hip.disc_conv9_dgrad(dy, w)),
                   ('wgrad', lambda: hip.disc_conv9_wgrad(x, dy)))
        else:
            wpk, wpd = hip.disc_vconv_pack_weight(w, cin, False), hip.disc_vconv_pack_weight(w, cin, True)
            fns = (('fwd', lambda: hip.disc_vconv(x, wpk, None, ks)), ('dgrad', lambda: hip.disc_vconv_dgrad(dy, wpd, tuple(x.shape), ks)),
                   ('wgrad', lambda: hip.disc_vconv_wgrad(x, dy, cin, ks)))
        for kind, fn in fns:
            ms = _median_ms(fn, steps, warmup)
            row[f'{kind}_ms'], row[f'{kind}_tflops'] = ms, flop / ms / 1e9
        out.append(row)
    return out


def _sg2_stages(net, size, steps, warmup, b=4):
    """ms of every stage of StyleGAN2Discriminator's conv_body at [b,3,size,size]: forward, input gradient, weight gradient"""
    from mrefsr_amd import hip
    from mrefsr_amd.ops.upfirdn2d import upfirdn2d
    taps, out = net.resample_taps, []

    def conv_rows(name, x, cout, ks, lib):
        cin = x.shape[3]
        w = torch.randn(cout, cin, ks, ks, device='cuda') * 0.05
        if lib == 'vconv':
            pk, fwd, dg, wg = hip.disc_vconv_pack_weight, hip.disc_vconv, hip.disc_vconv_dgrad, hip.disc_vconv_wgrad
        else:
            pk, fwd, dg, wg = hip.disc_sg2_pack_weight, hip.disc_sg2_conv, hip.disc_sg2_conv_dgrad, hip.disc_sg2_conv_wgrad
        wpk, wpd = pk(w, cin, False), pk(w, cin, True)
        y = fwd(x, wpk, None, ks)
        dy = torch.randn_like(y)
        flop = 2.0 * y.numel() * cin * ks * ks
        row = dict(stage=name, cin=cin, cout=cout, ks=ks, out=y.shape[1], gflop=flop / 1e9)
        for kind, fn in (('fwd', lambda: fwd(x, wpk, None, ks)), ('dgrad', lambda: dg(dy, wpd, tuple(x.shape), ks)),
                         ('wgrad', lambda: wg(x, dy, cin, ks))):
            ms = _median_ms(fn, steps, warmup)
            row[f'{kind}_ms'], row[f'{kind}_tflops'] = ms, flop / ms / 1e9
        out.append(row)

    c = net.conv_body[0][0].out_channels
    conv_rows('input 1x1', torch.randn(b, size, size, 4, device='cuda'), c, 1, 'sg2')
    for n, blk in enumerate(list(net.conv_body)[1:], 1):
        co = blk.conv2[1].out_channels
        x = torch.randn(b, size, size, c, device='cuda')
        conv_rows(f'block{n} conv1 3x3', x, c, 3, 'vconv')
        for name, pad, down in (('conv2 FIR', blk.conv2[0].pad, 1), ('skip FIR /2', blk.skip[0].pad, 2)):
            y = hip.disc_sg2_fir(x, taps, pad, down)
            gy = torch.randn_like(y)
            out.append(dict(stage=f'block{n} {name}', cin=c, out=y.shape[1],
                            fwd_ms=_median_ms(lambda: hip.disc_sg2_fir(x, taps, pad, down), steps, warmup),
                            dgrad_ms=_median_ms(lambda: hip.disc_sg2_fir(gy, taps, pad, down, adjoint_shape=tuple(x.shape)), steps, warmup)))
        # the same blur as a pass of the product's generic operator (csrc/upfirdn2d.hip, NCHW): the third form the FIR could take
        xn, k2 = torch.randn(b, c, size, size, device='cuda'), blk.conv2[0].kernel.cuda()
        out.append(dict(stage=f'block{n} conv2 FIR on ops.upfirdn2d (NCHW)', cin=c, out=size + 1,
                        fwd_ms=_median_ms(lambda: upfirdn2d(xn, k2, pad=blk.conv2[0].pad), steps, warmup)))
        conv_rows(f'block{n} conv2 3x3/2', hip.disc_sg2_fir(x, taps, blk.conv2[0].pad, 1), co, 3, 'sg2')
        conv_rows(f'block{n} skip 1x1', hip.disc_sg2_fir(x, taps, blk.skip[0].pad, 2), co, 1, 'sg2')
        c, size = co, size // 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out')
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--network-d', choices=sorted(NETWORK_D), default='ImageDiscriminator')
    ap.add_argument('--out-size', type=int, default=128, help='StyleGAN2Discriminator only: its out_size (LR is out_size / 4)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    sg2 = a.network_d == 'StyleGAN2Discriminator'
    size = a.out_size if sg2 else 160
    if a.trace:
        model = _model('wgan_gp', a.network_d, size // 4)
        model.optimize_parameters(1)
        torch.cuda.synchronize()
        print('traced one WGAN-GP step')
        return
    res = {}
    for cfg in (None, 'wgan_gp', 'vanilla'):
        model = _model(cfg, a.network_d, size // 4)
        it = [0]

        def step():
            it[0] += 1
            model.optimize_parameters(it[0])
        res[f'step_ms_{cfg or "l1"}'] = _median_ms(step, a.steps, a.warmup)
        del model
        torch.cuda.empty_cache()
    from mrefsr_amd.archs import build_network
    from mrefsr_amd.losses import GANLoss, GradientPenaltyLoss
    g = torch.Generator().manual_seed(0)
    real = (torch.rand(4, 3, size, size, generator=g) * 2 - 1).cuda()
    fake = (torch.rand(4, 3, size, size, generator=g) * 2 - 1).cuda()
    net = build_network(_net_d_opt(a.network_d, size)).cuda().train()
    gan, gp = GANLoss('wgan'), GradientPenaltyLoss(10.0)
    res['d_step_wgan_gp_ms_hip'] = _median_ms(lambda: _d_step(net, real, fake, gan, gp), a.steps, a.warmup)
    fk = fake.clone().requires_grad_(True)

    def g_part():
        for p in net.parameters():
            p.requires_grad_(False)
        gan(net(fk), True).backward()
        for p in net.parameters():
            p.requires_grad_(True)
    res['g_step_d_part_ms_hip'] = _median_ms(g_part, a.steps, a.warmup)

    class TorchD(torch.nn.Module):
        def __init__(self, net):
            super().__init__()
            self.net, self.fwd = net, _torch_d(net)

        def forward(self, x):
            return self.fwd(x)
    tnet = TorchD(net)
    res['d_step_wgan_gp_ms_torch_miopen'] = _median_ms(lambda: _d_step(tnet, real, fake, gan, gp), a.steps, a.warmup)
    res['adversarial_adds_ms_wgan_gp'] = res['step_ms_wgan_gp'] - res['step_ms_l1']
    res['adversarial_adds_ms_vanilla'] = res['step_ms_vanilla'] - res['step_ms_l1']
    if sg2:
        # the whole WGAN-GP step with the discriminator on torch's autograd: the same model, net_d's forward replaced
        model = _model('wgan_gp', a.network_d, size // 4)
        model.net_d.forward = _torch_d(model.net_d)
        it = [0]

        def tstep():
            it[0] += 1
            model.optimize_parameters(it[0])
        res['step_ms_wgan_gp_torch_miopen'] = _median_ms(tstep, a.steps, a.warmup)
        del model
        torch.cuda.empty_cache()
        res['out_size'] = size
        res['layers'] = _sg2_stages(net, size, a.steps, a.warmup)
    if a.network_d == 'VGGStyleDiscriminator':
        res['layers'] = _conv_layers(_vgg_shapes(), a.steps, a.warmup)
    if a.network_d == 'UNetDiscriminatorSN':
        res['layers'] = _conv_layers(_unet_shapes(), a.steps, a.warmup)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
