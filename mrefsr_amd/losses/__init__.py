"""Mirror of the loss module the reference model builds its criteria from (basicsr/models/losses.py, imported by
multi_ref_restoration_model.py:17 -- not basicsr/losses/losses.py, which differs; from that newer file come GANLoss's wgan_softplus
type and r1_penalty, which every StyleGAN2Discriminator configuration sets).  Classes register in LOSS_REGISTRY under the
reference's names; ``build_loss`` selects one by ``type`` (the contract of basicsr/losses/__init__.py)."""
from copy import deepcopy

from ..utils.registry import LOSS_REGISTRY
from .losses import (CharbonnierLoss, ContextualLoss, FFTLoss, FocalFrequencyLoss, GANLoss, GradientPenaltyLoss, L1Loss, LDLLoss, MSELoss, MSSSIMLoss, PerceptualLoss, SSIMLoss, TextureLoss,
                     gradient_penalty_loss, ldl_artifact_map_torch, ldl_loss_torch, r1_penalty, ssim_loss_torch, msssim_loss_torch, msssim_planes_torch,
                     fft_loss_torch, focal_frequency_loss_torch, focal_frequency_weight_torch, contextual_loss_torch, cx_patches_torch)

__all__ = ['build_loss', 'LOSS_REGISTRY', 'L1Loss', 'MSELoss', 'CharbonnierLoss', 'PerceptualLoss', 'TextureLoss', 'SSIMLoss', 'MSSSIMLoss', 'LDLLoss', 'FFTLoss', 'FocalFrequencyLoss', 'ContextualLoss', 'GANLoss',
           'GradientPenaltyLoss', 'gradient_penalty_loss', 'r1_penalty', 'ssim_loss_torch', 'msssim_loss_torch', 'msssim_planes_torch', 'ldl_artifact_map_torch', 'ldl_loss_torch',
           'fft_loss_torch', 'focal_frequency_loss_torch', 'focal_frequency_weight_torch', 'contextual_loss_torch', 'cx_patches_torch']


def build_loss(opt):
    opt = deepcopy(opt)
    return LOSS_REGISTRY.get(opt.pop('type'))(**opt)
