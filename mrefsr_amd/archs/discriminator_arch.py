"""ImageDiscriminator (basicsr/archs/discriminator_arch.py:10-45), VGGStyleDiscriminator (:47-125), UNetDiscriminatorSN
(:127-200) and StyleGAN2Discriminator (basicsr/archs/stylegan2_arch.py:733-799): the discriminators of the adversarial training step.

Same module tree, parameter and buffer names (74 state_dict entries at ndf 32) and initialisation (srntt_init_weights, normal
0.02, BatchNorm weights N(1, 0.02)) as the reference, so its checkpoints load unchanged.  The forward runs on the kernels of
csrc/disc.hip through the autograd nodes of archs/nhwc_disc.py, which are differentiable twice (the WGAN-GP gradient penalty).
VGGStyleDiscriminator keeps the reference's attribute order and PyTorch's default initialisation, so under one torch.manual_seed it
builds the reference's exact parameters; its forward runs on csrc/disc_vgg.hip through archs/nhwc_vggdisc.py.  UNetDiscriminatorSN
does the same with torch.nn.utils.spectral_norm (weight_orig / weight_u / weight_v, torch's own state_dict hooks); its forward runs
on csrc/disc_unet.hip and disc_vgg.hip through archs/nhwc_unetdisc.py.  StyleGAN2Discriminator is built from the blocks of
archs/stylegan2_ops.py in the reference's order (torch.randn weights, zero biases, no FIR buffer); its forward runs on csrc/disc_sg2.hip
and disc_vgg.hip through archs/nhwc_sg2disc.py.
Construction and state_dict work on the CPU; forward on a CPU tensor raises NotImplementedError, as every op of the package does.
"""
import math

import torch
from torch import nn
from torch.nn.utils import spectral_norm
from torch.nn.utils.spectral_norm import SpectralNorm

from ..utils.registry import ARCH_REGISTRY
from .arch_util import srntt_init_weights
from .stylegan2_ops import ConvLayer, EqualLinear, ResBlock


@ARCH_REGISTRY.register()
class ImageDiscriminator(nn.Module):

    def __init__(self, in_nc=3, ndf=32):
        super().__init__()
        if in_nc != 3:
            raise NotImplementedError(f'ImageDiscriminator: in_nc={in_nc}; the kernels take RGB images (in_nc 3)')
        if ndf <= 0 or ndf % 16:
            raise NotImplementedError(f'ImageDiscriminator: ndf={ndf}; the convolution kernels need a multiple of 16')

        def conv_block(in_channels, out_channels):
            return nn.Sequential(
                nn.Conv2d(in_channels, out_channels, 3, 1, 1), nn.BatchNorm2d(out_channels), nn.LeakyReLU(0.2, True),
                nn.Conv2d(out_channels, out_channels, 3, 2, 1), nn.BatchNorm2d(out_channels), nn.LeakyReLU(0.2, True))

        self.conv_block1 = conv_block(in_nc, ndf)
        self.conv_block2 = conv_block(ndf, ndf * 2)
        self.conv_block3 = conv_block(ndf * 2, ndf * 4)
        self.conv_block4 = conv_block(ndf * 4, ndf * 8)
        self.conv_block5 = conv_block(ndf * 8, ndf * 16)
        self.out_block = nn.Sequential(
            nn.AdaptiveAvgPool2d(1), nn.Conv2d(ndf * 16, 1024, kernel_size=1), nn.LeakyReLU(0.2), nn.Conv2d(1024, 1, kernel_size=1),
            nn.Sigmoid())
        srntt_init_weights(self, init_type='normal', init_gain=0.02)

    def blocks(self):
        return (self.conv_block1, self.conv_block2, self.conv_block3, self.conv_block4, self.conv_block5)

    def forward(self, x):
        if not x.is_cuda:
            raise NotImplementedError('ImageDiscriminator: mrefsr_amd has no CPU path (HIP kernels only)')
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise NotImplementedError(f'ImageDiscriminator: input {tuple(x.shape)} {x.dtype}; fp32 [B,3,H,W] only')
        from . import nhwc_disc
        return nhwc_disc.discriminator(self, x)


@ARCH_REGISTRY.register()
class VGGStyleDiscriminator(nn.Module):
    """the reference's VGG-style discriminator with its default input_size of 160 (the GT crop of the training config).
    input_size 256 is refused: the reference builds conv5_* / bn5_* for it but keeps linear1 sized for a 5 x 5 map, so its forward
    cannot run."""

    def __init__(self, num_in_ch, num_feat, input_size=160):
        super().__init__()
        self.input_size = input_size
        assert self.input_size == 160 or self.input_size == 256, (f'input size must be 160 or 256, but received {input_size}')
        if input_size == 256:
            raise NotImplementedError('VGGStyleDiscriminator: input_size 256 -- the reference adds conv5_* / bn5_* but sizes linear1 for a '
                                      '5 x 5 map, which a 256 input cannot give after six halvings (its forward fails in linear1)')
        if num_in_ch != 3:
            raise NotImplementedError(f'VGGStyleDiscriminator: num_in_ch={num_in_ch}; the kernels take RGB images (num_in_ch 3)')
        if num_feat <= 0 or num_feat % 16:
            raise NotImplementedError(f'VGGStyleDiscriminator: num_feat={num_feat}; the convolution kernels need a multiple of 16')
        f = num_feat
        # the reference's attribute (and so default-initialisation) order
        self.conv0_0 = nn.Conv2d(num_in_ch, f, 3, 1, 1, bias=True)
        self.conv0_1 = nn.Conv2d(f, f, 4, 2, 1, bias=False)
        self.bn0_1 = nn.BatchNorm2d(f, affine=True)
        for i, (cin, cout) in enumerate(((f, 2 * f), (2 * f, 4 * f), (4 * f, 8 * f), (8 * f, 8 * f)), 1):
            setattr(self, f'conv{i}_0', nn.Conv2d(cin, cout, 3, 1, 1, bias=False))
            setattr(self, f'bn{i}_0', nn.BatchNorm2d(cout, affine=True))
            setattr(self, f'conv{i}_1', nn.Conv2d(cout, cout, 4, 2, 1, bias=False))
            setattr(self, f'bn{i}_1', nn.BatchNorm2d(cout, affine=True))
        self.linear1 = nn.Linear(f * 8 * 5 * 5, 100)
        self.linear2 = nn.Linear(100, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)

    def conv_bn_layers(self):
        """the nine (conv, BatchNorm) pairs after conv0_0, in forward order"""
        out = [(self.conv0_1, self.bn0_1)]
        for i in range(1, 5):
            out += [(getattr(self, f'conv{i}_0'), getattr(self, f'bn{i}_0')), (getattr(self, f'conv{i}_1'), getattr(self, f'bn{i}_1'))]
        return out

    def forward(self, x):
        assert x.size(2) == self.input_size, (f'Input size must be identical to input_size, but received {x.size()}.')
        if not x.is_cuda:
            raise NotImplementedError('VGGStyleDiscriminator: mrefsr_amd has no CPU path (HIP kernels only)')
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise NotImplementedError(f'VGGStyleDiscriminator: input {tuple(x.shape)} {x.dtype}; fp32 [B,3,H,W] only')
        for _, bn in self.conv_bn_layers():
            if not (bn.training and bn.track_running_stats and bn.momentum is not None):
                raise NotImplementedError('VGGStyleDiscriminator: BatchNorm2d runs in training mode with running statistics and a momentum '
                                          'only (the model trains net_d; eval-mode statistics have no kernel here)')
        from . import nhwc_vggdisc
        return nhwc_vggdisc.discriminator(self, x)


@ARCH_REGISTRY.register(suffix='basicsr')
class UNetDiscriminatorSN(nn.Module):
    """Real-ESRGAN's U-Net discriminator with spectral normalisation (conv1 .. conv8), registered as the reference registers it
    (UNetDiscriminatorSN_basicsr; `type: UNetDiscriminatorSN` resolves through the registry's suffix fallback).

    forward does not call the conv modules: their spectral-norm pre-hooks would run the power iteration on rocBLAS.  It runs the
    iteration on the kernels instead (once per forward in training mode, updating weight_u / weight_v in place; none in eval mode),
    so convN.weight, the attribute the hook refreshes, keeps whatever the last hook call left in it: read W_orig / sigma from
    nhwc_unetdisc.spectral_norm_weights, not from there.  Input H and W must be multiples of 8."""

    def __init__(self, num_in_ch, num_feat=64, skip_connection=True):
        super().__init__()
        if num_in_ch != 3:
            raise NotImplementedError(f'UNetDiscriminatorSN: num_in_ch={num_in_ch}; the kernels take RGB images (num_in_ch 3)')
        if num_feat <= 0 or num_feat % 16:
            raise NotImplementedError(f'UNetDiscriminatorSN: num_feat={num_feat}; the convolution kernels need a multiple of 16')
        self.skip_connection = skip_connection
        norm = spectral_norm
        f = num_feat
        # the reference's attribute (and so default-initialisation and power-iteration RNG) order
        self.conv0 = nn.Conv2d(num_in_ch, f, kernel_size=3, stride=1, padding=1)
        self.conv1 = norm(nn.Conv2d(f, f * 2, 4, 2, 1, bias=False))
        self.conv2 = norm(nn.Conv2d(f * 2, f * 4, 4, 2, 1, bias=False))
        self.conv3 = norm(nn.Conv2d(f * 4, f * 8, 4, 2, 1, bias=False))
        self.conv4 = norm(nn.Conv2d(f * 8, f * 4, 3, 1, 1, bias=False))
        self.conv5 = norm(nn.Conv2d(f * 4, f * 2, 3, 1, 1, bias=False))
        self.conv6 = norm(nn.Conv2d(f * 2, f, 3, 1, 1, bias=False))
        self.conv7 = norm(nn.Conv2d(f, f, 3, 1, 1, bias=False))
        self.conv8 = norm(nn.Conv2d(f, f, 3, 1, 1, bias=False))
        self.conv9 = nn.Conv2d(f, 1, 3, 1, 1)

    def sn_convs(self):
        return [getattr(self, f'conv{i}') for i in range(1, 9)]

    def sn_hooks(self):
        """the SpectralNorm pre-hook of each of conv1 .. conv8; refuses what the kernels do not compute"""
        hooks = []
        for i, conv in enumerate(self.sn_convs(), 1):
            found = [h for h in conv._forward_pre_hooks.values() if isinstance(h, SpectralNorm) and h.name == 'weight']
            if len(found) != 1:
                raise NotImplementedError(f'UNetDiscriminatorSN: conv{i} has no spectral norm of its weight (torch.nn.utils.spectral_norm)')
            h = found[0]
            if h.n_power_iterations != 1 or h.dim != 0:
                raise NotImplementedError(f'UNetDiscriminatorSN: conv{i} spectral norm with n_power_iterations={h.n_power_iterations}, '
                                          f'dim={h.dim}; the kernels run the reference\'s (1 iteration, dim 0)')
            hooks.append(h)
        return hooks

    def sn_eps(self):
        eps = {h.eps for h in self.sn_hooks()}
        if len(eps) != 1:
            raise NotImplementedError(f'UNetDiscriminatorSN: spectral norms with different eps {sorted(eps)}')
        return eps.pop()

    def forward(self, x):
        if not x.is_cuda:
            raise NotImplementedError('UNetDiscriminatorSN: mrefsr_amd has no CPU path (HIP kernels only)')
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise NotImplementedError(f'UNetDiscriminatorSN: input {tuple(x.shape)} {x.dtype}; fp32 [B,3,H,W] only')
        self.sn_hooks()
        from . import nhwc_unetdisc
        return nhwc_unetdisc.discriminator(self, x)


@ARCH_REGISTRY.register()
class StyleGAN2Discriminator(nn.Module):
    """the residual StyleGAN2 critic: a 1x1 input stage, one ResBlock per halving from out_size down to 4 x 4, the minibatch-stddev
    channel, final_conv and a two-layer final_linear.  The modules hold the reference's parameters under its names; forward does not
    call them (they would run on the generic ops) but archs/nhwc_sg2disc.py.  Input [B, 3, out_size, out_size]: another H x W raises
    RuntimeError naming final_linear, where the reference fails; an input that is not a 4-D RGB fp32 batch raises the siblings'
    NotImplementedError (the reference fails in its first convolution there, not in final_linear)."""

    def __init__(self, out_size, channel_multiplier=2, resample_kernel=(1, 3, 3, 1), stddev_group=4, narrow=1):
        super().__init__()
        if not isinstance(out_size, int) or out_size < 8 or out_size > 1024 or out_size & (out_size - 1):
            raise NotImplementedError(f'StyleGAN2Discriminator: out_size={out_size}; a power of two in 8 .. 1024 (the reference has channel '
                                      'counts for these sizes only, and one ResBlock per halving down to 4 x 4)')
        kernel = torch.as_tensor(resample_kernel, dtype=torch.float32)
        if kernel.ndim != 1 or not 2 <= kernel.numel() <= 4:
            raise NotImplementedError(f'StyleGAN2Discriminator: resample_kernel={resample_kernel}; the FIR kernels take a 1-D list of 2 to 4 '
                                      'magnitudes (applied as their outer product)')
        if not isinstance(stddev_group, int) or stddev_group < 1:
            raise NotImplementedError(f'StyleGAN2Discriminator: stddev_group={stddev_group}; a positive integer')
        channels = {
            '4': int(512 * narrow), '8': int(512 * narrow), '16': int(512 * narrow), '32': int(512 * narrow),
            '64': int(256 * channel_multiplier * narrow), '128': int(128 * channel_multiplier * narrow),
            '256': int(64 * channel_multiplier * narrow), '512': int(32 * channel_multiplier * narrow),
            '1024': int(16 * channel_multiplier * narrow)}
        log_size = int(math.log(out_size, 2))
        for i in range(log_size, 1, -1):
            c = channels[f'{2 ** i}']
            if c <= 0 or c % 16:
                raise NotImplementedError(f'StyleGAN2Discriminator: {c} channels at {2 ** i} x {2 ** i} (narrow={narrow}, channel_multiplier='
                                          f'{channel_multiplier}); the convolution kernels need a multiple of 16')
        # the reference's construction (and so torch.randn) order
        conv_body = [ConvLayer(3, channels[f'{out_size}'], 1, bias=True, activate=True)]
        in_channels = channels[f'{out_size}']
        for i in range(log_size, 2, -1):
            out_channels = channels[f'{2 ** (i - 1)}']
            conv_body.append(ResBlock(in_channels, out_channels, resample_kernel))
            in_channels = out_channels
        self.conv_body = nn.Sequential(*conv_body)
        self.final_conv = ConvLayer(in_channels + 1, channels['4'], 3, bias=True, activate=True)
        self.final_linear = nn.Sequential(
            EqualLinear(channels['4'] * 4 * 4, channels['4'], bias=True, bias_init_val=0, lr_mul=1, activation='fused_lrelu'),
            EqualLinear(channels['4'], 1, bias=True, bias_init_val=0, lr_mul=1, activation=None))
        self.out_size = out_size
        self.resample_taps = tuple((kernel / kernel.sum()).tolist())   # make_resample_kernel's outer product, per axis
        self.stddev_group = stddev_group
        self.stddev_feat = 1

    def forward(self, x):
        if not x.is_cuda:
            raise NotImplementedError('StyleGAN2Discriminator: mrefsr_amd has no CPU path (HIP kernels only)')
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise NotImplementedError(f'StyleGAN2Discriminator: input {tuple(x.shape)} {x.dtype}; fp32 [B,3,H,W] only')
        from . import nhwc_sg2disc
        return nhwc_sg2disc.discriminator(self, x)
