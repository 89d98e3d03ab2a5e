"""ImageDiscriminator (basicsr/archs/discriminator_arch.py:10-45), VGGStyleDiscriminator (:47-125) and UNetDiscriminatorSN
(:127-200): the discriminators of the adversarial training step.

Same module tree, parameter and buffer names (74 state_dict entries at ndf 32) and initialisation (srntt_init_weights, normal
0.02, BatchNorm weights N(1, 0.02)) as the reference, so its checkpoints load unchanged.  The forward runs on the kernels of
csrc/disc.hip through the autograd nodes of archs/nhwc_disc.py, which are differentiable twice (the WGAN-GP gradient penalty).
VGGStyleDiscriminator keeps the reference's attribute order and PyTorch's default initialisation, so under one torch.manual_seed it
builds the reference's exact parameters; its forward runs on csrc/disc_vgg.hip through archs/nhwc_vggdisc.py.  UNetDiscriminatorSN
does the same with torch.nn.utils.spectral_norm (weight_orig / weight_u / weight_v, torch's own state_dict hooks); its forward runs
on csrc/disc_unet.hip and disc_vgg.hip through archs/nhwc_unetdisc.py.
Construction and state_dict work on the CPU; forward on a CPU tensor raises NotImplementedError, as every op of the package does.
"""
import torch
from torch import nn
from torch.nn.utils import spectral_norm
from torch.nn.utils.spectral_norm import SpectralNorm

from ..utils.registry import ARCH_REGISTRY
from .arch_util import srntt_init_weights


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
