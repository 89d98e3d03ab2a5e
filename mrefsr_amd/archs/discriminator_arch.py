"""ImageDiscriminator (basicsr/archs/discriminator_arch.py:10-45): the discriminator of the adversarial training step.

Same module tree, parameter and buffer names (74 state_dict entries at ndf 32) and initialisation (srntt_init_weights, normal
0.02, BatchNorm weights N(1, 0.02)) as the reference, so its checkpoints load unchanged.  The forward runs on the kernels of
csrc/disc.hip through the autograd nodes of archs/nhwc_disc.py, which are differentiable twice (the WGAN-GP gradient penalty).
Construction and state_dict work on the CPU; forward on a CPU tensor raises NotImplementedError, as every op of the package does.
"""
import torch
from torch import nn

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
