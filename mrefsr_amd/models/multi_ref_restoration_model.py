"""MultiRefRestorationModel: the caller of the hot path (mirror of
basicsr/models/multi_ref_restoration_model.py:20-386 for what the shipped yml exercises).

Same option keys (network_g / network_map / network_extractor / path.* / train.*), same methods
(feed_data :190-195, optimize_parameters :197-279, test :281-294, get_current_log,
update_learning_rate, save / load of ``{'params': state_dict}`` checkpoints -- with train.ema_decay ``{'params', 'params_ema'}``), same optimiser
layout: Adam with four parameter groups chosen by name (:60-89) --
    'offset' & 'small'  -> lr_relu3_offset     'offset' & 'medium' -> lr_relu2_offset
    other 'offset'      -> lr_offset           everything else     -> lr_g
Losses (:114-165, :237-279): the pixel criterion (L1Loss, MSELoss, CharbonnierLoss), perceptual_opt and style_opt
(PerceptualLoss of losses/, its VGG19 forward and backward on the HIP kernels), texture_opt with use_weights: true (TextureLoss; its
swapped reference maps and weights, which the reference model reads but never sets, are built from the matcher's indices and values
on the kernels of csrc/texture.hip: _texture_targets), ssim_opt (SSIMLoss: 1 - SSIM on the Y or the colour planes, the quantity
validation reports, on the kernels of csrc/ssim_loss.hip; no counterpart in the reference), msssim_opt (MSSSIMLoss: its multi-scale
form over up to five levels, on the kernels of csrc/msssim.hip; val.msssim reports it in validation), ldl_opt (LDLLoss: the artifact loss of
LDL between the output, the GT and the output of net_g_ema on the same input, basicsr/models/realesrgan_model.py:211-226, on the
kernels of csrc/ldl_loss.hip; needs train.ema_decay: _ema_pass), freq_opt (FFTLoss or FocalFrequencyLoss: a distance between the
spectra of the output and the GT, on the dense-DFT kernels of csrc/freq_loss.hip; no counterpart in the reference), contextual_opt
(ContextualLoss: the non-local contextual loss between the VGG features of the output and of the GT, on the kernels of
csrc/contextual.hip; no counterpart in the reference), and the adversarial term: network_d
(ImageDiscriminator, VGGStyleDiscriminator, UNetDiscriminatorSN or StyleGAN2Discriminator, on the kernels of csrc/disc.hip, disc_vgg.hip,
disc_unet.hip and disc_sg2.hip)
with gan_type / gan_weight / grad_penalty_weight, its own Adam (optimizer_d, second in self.optimizers) and scheduler, the D step of :219-245 and l_g_gan of
:272-276.  gan_type wgan_softplus and the lazily applied R1 penalty on the real images (train.r1_reg_weight, train.net_d_reg_every) are
those of basicsr/losses/losses.py:284-318, 391-405 and basicsr/models/stylegan2_model.py:75-79, 198-221; lr_d and beta_d are used as
written (stylegan2_model.py:135-143 rescales them by every / (every + 1): left to the configuration).  train.d_augment puts
DiffAugment / ADA's differentiable colour, translation, cutout and flip operators in front of every discriminator call, on the kernels
of csrc/disc_augment.hip (_setup_d_augment, _d; no counterpart in the reference; a bad option is a ValueError that names it).
train.ref_augment, val.ref_perturb and val.match_probe put homography views of the references (views.py, csrc/warp.hip; the view
generator of ref_cufed_dataset.py:190-272 on the device) into feed_data and validation (_setup_ref_views, _match_probe_stats).
Refused, not silently skipped: texture_opt without use_weights: true (the reference cannot evaluate it either) and other
discriminators (NotImplementedError); gan_type without network_d and the
reverse, r1_reg_weight without network_d (NotImplementedError); an r1_reg_weight that is not a finite number of at least 0, a
net_d_reg_every that is not an int of at least 1 or that comes without r1_reg_weight, bools for either (ValueError); the clipping,
EMA and hip_adam options together with train.hip_graph (ValueError).

What differs underneath (SURVEY 7 "hard parts"):
  * the K references run as one k-major batch through extractor / matching / VGG19 / net_g;
  * net_extractor and net_map are frozen replicas under no_grad and are NOT wrapped in DDP (no
    gradient can reach them past the arg-max; wrapping them only adds a "unused parameter"
    failure mode); net_g is wrapped in DistributedDataParallel (RCCL all-reduce of its 94.8 MB);
  * `l.item()` logging is deferred: log_dict holds device scalars until get_current_log().
"""
import contextlib
import logging
import math
import os
from collections import OrderedDict

import torch
from torch.nn.parallel import DistributedDataParallel

from ..archs import build_network
from .. import views
from ..color_fix import color_fix, parse_color_fix
from ..utils.registry import MODEL_REGISTRY


class _MultiStepRestartLR(torch.optim.lr_scheduler._LRScheduler):
    """basicsr/models/lr_scheduler.py:6-33 (MultiStepLR with optional restarts)"""

    def __init__(self, optimizer, milestones, gamma=0.1, restarts=(0, ), restart_weights=(1, ), last_epoch=-1):
        from collections import Counter
        self.milestones, self.gamma = Counter(milestones), gamma
        self.restarts, self.restart_weights = list(restarts), list(restart_weights)
        assert len(self.restarts) == len(self.restart_weights), 'restarts and their weights do not match.'
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        if self.last_epoch in self.restarts:
            weight = self.restart_weights[self.restarts.index(self.last_epoch)]
            return [group['initial_lr'] * weight for group in self.optimizer.param_groups]
        if self.last_epoch not in self.milestones:
            return [group['lr'] for group in self.optimizer.param_groups]
        return [group['lr'] * self.gamma**self.milestones[self.last_epoch] for group in self.optimizer.param_groups]


class _CosineAnnealingRestartLR(torch.optim.lr_scheduler._LRScheduler):
    """basicsr/models/lr_scheduler.py:36-96 (cosine annealing inside each period, restarted with a weight at the period's end)"""

    def __init__(self, optimizer, periods, restart_weights=(1, ), eta_min=0, last_epoch=-1):
        self.periods, self.restart_weights, self.eta_min = list(periods), list(restart_weights), eta_min
        assert len(self.periods) == len(self.restart_weights), 'periods and restart_weights should have the same length.'
        self.cumulative_period = [sum(self.periods[0:i + 1]) for i in range(len(self.periods))]
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        # the first period whose (cumulative) end has not been passed (ref :36-54; past the last one the reference fails too)
        idx = next(i for i, period in enumerate(self.cumulative_period) if self.last_epoch <= period)
        weight, period = self.restart_weights[idx], self.periods[idx]
        nearest_restart = 0 if idx == 0 else self.cumulative_period[idx - 1]
        return [self.eta_min + weight * 0.5 * (base_lr - self.eta_min) * (1 + math.cos(math.pi * ((self.last_epoch - nearest_restart) / period)))
                for base_lr in self.base_lrs]


@MODEL_REGISTRY.register()
class MultiRefRestorationModel:

    def __init__(self, opt):
        self.opt = opt
        if opt.get('num_gpu', 1) == 0:
            raise NotImplementedError('mrefsr_amd has no CPU path: num_gpu must be >= 1')
        self.check_self_ensemble(opt.get('val'))   # (a bad value is refused before anything is built; test() reads the option)
        self.color_fix_cfg = parse_color_fix(opt.get('val'))   # None, or the checked val.color_fix configuration (refused likewise)
        self._setup_ref_views(opt)   # train.ref_augment, val.ref_perturb, val.match_probe (refused likewise)
        self.ref_select = self.check_ref_select(opt)   # None, or (top_k, score) of the ref_select option
        if self.ref_select is not None and not self._REF_POOLS:
            raise ValueError(f'ref_select: {type(self).__name__} takes one reference per sample; reference pools are '
                             "MultiRefRestorationModel's")
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.is_train = opt['is_train']
        self._setup_degradation(opt)
        self.schedulers, self.optimizers = [], []
        logger = logging.getLogger('basicsr')

        self.net_map = build_network(opt['network_map']).to(self.device).eval()
        self.net_extractor = build_network(opt['network_extractor']).to(self.device).eval()
        for net in (self.net_map, self.net_extractor):
            for p in net.parameters():
                p.requires_grad_(False)
        path = opt.get('path', {})
        if path.get('pretrain_network_feature_extractor'):
            self.load_network(self.net_extractor, path['pretrain_network_feature_extractor'], path.get('strict_load', True))

        self.net_g = build_network(opt['network_g']).to(self.device)
        if path.get('pretrain_network_g'):
            self.load_network(self.net_g, path['pretrain_network_g'], path.get('strict_load', True), path.get('param_key_g', 'params'))
        if opt.get('dist', False):
            self.net_g = DistributedDataParallel(self.net_g, device_ids=[self.device.index],
                                                 find_unused_parameters=opt.get('find_unused_parameters', False),
                                                 broadcast_buffers=opt.get('broadcast_buffers', True))
        self.log_dict = OrderedDict()
        if self.is_train:
            self._check_deterministic_options()
            self._check_update_options()
            self.net_g.train()
            train_opt = opt['train']
            self._setup_ema()
            groups = {'g': [], 'offset': [], 'relu3': [], 'relu2': []}
            for name, v in self.get_bare_model(self.net_g).named_parameters():
                if not v.requires_grad:
                    continue
                if 'offset' in name:
                    if 'small' in name:
                        logger.info(name)
                        groups['relu3'].append(v)
                    elif 'medium' in name:
                        logger.info(name)
                        groups['relu2'].append(v)
                    else:
                        groups['offset'].append(v)
                else:
                    groups['g'].append(v)
            self.optimizer_g = self._adam(
                [{'params': groups['g']},
                 {'params': groups['offset'], 'lr': train_opt['lr_offset']},
                 {'params': groups['relu3'], 'lr': train_opt['lr_relu3_offset']},
                 {'params': groups['relu2'], 'lr': train_opt['lr_relu2_offset']}],
                lr=train_opt['lr_g'], weight_decay=train_opt.get('weight_decay_g', 0), betas=train_opt['beta_g'],
                capturable=self._train_graph_wanted(),   # step counters on the device: the update can be part of a hipGraph
                # torch's fused multi-tensor Adam: the same update (ref :90-104 builds a plain torch.optim.Adam) in ~13 launches
                # instead of ~60; train.fused_adam: false keeps the per-operation foreach form (under hipGraph replay the foreach
                # form with device-side step counters costs 14 ms per step: 52.6 against 37.2 ms)
                fused=bool(train_opt.get('fused_adam', True)) and self.device.type == 'cuda')
            self._setup_grad_clip(self.optimizer_g, 'g')
            if self.net_g_ema is not None and self._hip_adam_wanted():   # the EMA is written by the pass that updates net_g
                bare, ema = dict(self.get_bare_model(self.net_g).named_parameters()), dict(self.net_g_ema.named_parameters())
                self.optimizer_g.ema_params = {bare[k]: v for k, v in ema.items()}
                self.optimizer_g.ema_decay = self.ema_decay
            self.optimizers.append(self.optimizer_g)
            self.init_training_settings()

    # ------------------------------------------------------------------ opt['degradation']: the LQ input synthesised on the device
    _GT_USM_KEYS = ('l1_gt_usm', 'percep_gt_usm', 'gan_gt_usm')
    # (the state of a model without the option; _setup_degradation sets the instance's)
    degradation = pair_pool = gt_usm = None
    _synthesise = False
    _gt_usm = dict.fromkeys(_GT_USM_KEYS, False)

    def _setup_degradation(self, opt):
        """opt['degradation'] (a dict of degradation.OPTION_KEYS: the reference yml's degradation and blur-kernel keys, plus an
        optional queue_size): training batches get their LQ input from Real-ESRGAN's second-order degradation of the GT
        (realesrgan_model.py:68-179) on the kernels of csrc/degrade.hip, see _degrade.  Validation and test() never synthesise
        (:187-191).  l1_gt_usm / percep_gt_usm / gan_gt_usm (top level, as in the reference's yml) make the pixel, SSIM, LDL and frequency
        losses / the perceptual and style losses / the discriminator's real images take the USM-sharpened GT; the texture loss has no
        GT.  They are refused without `degradation`.  train.hip_graph stays allowed: the synthesis runs in feed_data, outside the
        captured region (the sharpened GT is one more static input of the capture).  Without the option nothing changes."""
        self.degradation = self.pair_pool = self.gt_usm = None
        self._synthesise = False
        self._gt_usm = {k: bool(opt.get(k, False)) for k in self._GT_USM_KEYS}
        deg_opt = opt.get('degradation')
        if deg_opt is None or deg_opt is False:   # ({} is the option with every default)
            wanted = [k for k in self._GT_USM_KEYS if self._gt_usm[k]]
            if wanted:
                raise ValueError(f'{wanted} without the degradation option: the USM-sharpened GT is made by the degradation chain; set '
                                 'degradation or drop them')
            return
        if not self._REF_POOLS:
            raise NotImplementedError(f"degradation: {type(self).__name__} does not synthesise its input; MultiRefRestorationModel does")
        from ..degradation import HighOrderDegradation, TrainingPairPool
        if not isinstance(deg_opt, dict):
            raise ValueError(f'degradation: a dict of options expected ({{}} for the defaults), got {deg_opt!r}')
        deg_opt = dict(deg_opt)
        deg_opt.setdefault('scale', opt['scale'])
        if deg_opt['scale'] != opt['scale']:
            raise ValueError(f"degradation.scale {deg_opt['scale']} differs from the model's scale {opt['scale']}")
        self.degradation = HighOrderDegradation(deg_opt)
        if self.degradation.queue_size is not None:
            self.pair_pool = TrainingPairPool(self.degradation.queue_size)
        import numpy as np
        seed = opt.get('manual_seed')
        if seed is None:   # (from torch's global generator: reproducible behind torch.manual_seed)
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        self._degrade_rng = np.random.default_rng(seed)
        self._degrade_gen = torch.Generator(device=self.device).manual_seed(seed)
        self._pool_gen = torch.Generator().manual_seed(seed)
        self._synthesise = bool(self.is_train)

    def _degrade(self, data):
        """feed_data's dict with img_in_lq replaced by the synthesised LQ of data['img_in'] (on the 1/255 grid) and img_in_up by its
        bicubic x scale up-sampling clamped to [0, 1] -- the frozen extractor is fed from the degraded image, as it would be at
        deployment; sets gt_usm.  With queue_size the (lq, gt, references, ref_valid) of the batch go through the training pair pool
        first (realesrgan_model.py:31-66, :176-178).  The GT sides must be multiples of 4 * scale."""
        from .. import hip
        gt = data['img_in'].to(self.device, non_blocking=True).float().contiguous()
        plan = self.degradation.sample(gt.shape[0], gt.shape[2:], self._degrade_rng)
        lq, gt_usm = self.degradation.apply(gt, plan, self._degrade_gen)
        data = dict(data, img_in=gt, img_in_lq=lq)
        if self.pair_pool is not None:
            keys = [k for k in ('img_in_lq', 'img_in', 'img_ref_list', 'ref_valid') if data.get(k) is not None]
            data.update(self.pair_pool.step({k: data[k] for k in keys}, self._pool_gen))
            gt_usm = hip.degrade_usm(data['img_in'].contiguous())
        self.gt_usm = gt_usm
        with torch.no_grad():
            data['img_in_up'] = torch.clamp(hip.degrade_resize(data['img_in_lq'].contiguous(), scale_factor=self.degradation.scale,
                                                               mode='bicubic'), 0, 1)
        return data

    def _gt_for(self, which):
        """the GT of a loss family: 'l1' (pixel, SSIM, LDL, frequency), 'percep' (perceptual, style, contextual) or 'gan' (D's real images)"""
        return self.gt_usm if self._gt_usm[which + '_gt_usm'] and self.gt_usm is not None else self.gt

    # ------------------------------------------------------------------ the parameter update: train.hip_adam, train.ema_decay
    def _hip_adam_wanted(self):
        """opt['train']['hip_adam']: optimizer_g and optimizer_d are optim.HipAdam -- torch.optim.Adam's state and arithmetic, the
        update of all parameter groups as one launch of this project's kernel (csrc/optim.hip) instead of torch's fused
        multi-tensor Adam.  Off by default."""
        return bool((self.opt.get('train') or {}).get('hip_adam'))

    def _adam(self, params, **kw):
        if not self._hip_adam_wanted():
            return torch.optim.Adam(params, **kw)
        from ..optim import HipAdam
        kw.pop('fused', None)
        kw.pop('capturable', None)
        return HipAdam(params, **kw)

    def _check_update_options(self):
        """train.ema_decay and train.hip_adam are not offered together with the (experimental) hipGraph replay of the training
        step: refused, not one of them dropped.  The values of the clipping options and of train.r1_reg_weight /
        train.net_d_reg_every are checked here too."""
        train_opt = self.opt.get('train') or {}
        on = [f'train.{k}' for k in ('ema_decay', 'hip_adam') + self._CLIP_OPTIONS if train_opt.get(k)]
        if on and self._train_graph_wanted():
            raise ValueError(f"{' and '.join(on)} cannot be combined with train.hip_graph / MREFSR_TRAIN_GRAPH=1: the graph replay of the "
                             "training step is experimental and captures torch's own Adam update only; turn one of the two off")
        for k in self._CLIP_OPTIONS[:2]:
            v = train_opt.get(k)
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v > 0)):
                raise ValueError(f'train.{k}: {v!r} is not a finite number above 0 (leave the option out for no clipping)')
        v = train_opt.get('r1_reg_weight')
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v >= 0)):
            raise ValueError(f'train.r1_reg_weight: {v!r} is not a finite number of at least 0 (0 or absent: no R1 regularisation)')
        every = train_opt.get('net_d_reg_every')
        if every is not None:
            if isinstance(every, bool) or not isinstance(every, int) or every < 1:
                raise ValueError(f'train.net_d_reg_every: {every!r} is not an int of at least 1')
            if not v:
                raise ValueError('train.net_d_reg_every without train.r1_reg_weight: there is no regulariser to apply lazily; set '
                                 'r1_reg_weight above 0 or drop net_d_reg_every')
        if train_opt.get('skip_nonfinite_steps') and not train_opt.get('fused_adam', True) and not train_opt.get('hip_adam'):
            raise ValueError("train.skip_nonfinite_steps cannot be combined with train.fused_adam: false unless train.hip_adam is on: "
                             "torch's non-fused Adam has no found_inf to skip an update by")

    # ------------------------------------------------------------------ train.grad_clip_norm_g / _d, train.skip_nonfinite_steps
    _CLIP_OPTIONS = ('grad_clip_norm_g', 'grad_clip_norm_d', 'skip_nonfinite_steps')

    def _setup_grad_clip(self, optimizer, which):
        """train.grad_clip_norm_<which>: torch.nn.utils.clip_grad_norm_ (global L2 norm over all parameter groups) in front of that
        optimiser's update; train.skip_nonfinite_steps: an update whose gradient norm is inf or NaN is left out, on the device
        (parameters, moments and step counts keep their bits; the EMA update is made all the same).  Both absent: nothing is set
        up and no launch is added.  HipAdam does it inside its step; for torch's Adam, _clip_gradients runs in front of it."""
        train_opt = self.opt.get('train') or {}
        max_norm, skip = train_opt.get(f'grad_clip_norm_{which}'), bool(train_opt.get('skip_nonfinite_steps'))
        optimizer._mrefsr_clip = (max_norm, skip) if max_norm is not None or skip else None
        if optimizer._mrefsr_clip and self._hip_adam_wanted():
            optimizer.max_grad_norm, optimizer.skip_nonfinite = max_norm, skip

    def _clip_gradients(self, optimizer, which):
        """the norm (and, for torch's Adam, the scaling in place and found_inf) in front of optimizer.step(), and the log entries
        grad_norm_<which> (unclipped) / skipped_steps_<which>: views of the device state, read at get_current_log()"""
        cfg = getattr(optimizer, '_mrefsr_clip', None)
        if not cfg:
            return
        from .. import hip
        if self._hip_adam_wanted():
            state = optimizer.clip_state   # (filled by the step that has just run)
        else:
            params = [p for group in optimizer.param_groups for p in group['params'] if p.grad is not None]
            if not params:
                return
            grads = [p.grad for p in params]
            state = getattr(optimizer, 'clip_state', None)
            if state is None:
                state = optimizer.clip_state = hip.GradClipState(params[0].device)
            optimizer._clip_table = hip.optim_table(params, grads, cached=getattr(optimizer, '_clip_table', None), need_moments=False)
            hip.grad_norm_multi(optimizer._clip_table, state, cfg[0] or 0.0, cfg[1])
            if cfg[0]:
                hip.grad_scale_multi(optimizer._clip_table, state, grads)
            if cfg[1]:
                optimizer.found_inf = state.found_inf   # torch's fused Adam leaves the update out and takes its step counts back
        if state is not None:
            self.log_dict[f'grad_norm_{which}'] = state.total_norm
            self.log_dict[f'skipped_steps_{which}'] = state.skipped

    net_g_ema = None
    cri_texture = None   # TextureLoss of train.texture_opt (init_training_settings)
    cri_ssim = None      # SSIMLoss of train.ssim_opt
    cri_msssim = None    # MSSSIMLoss of train.msssim_opt
    cri_freq = None      # FFTLoss / FocalFrequencyLoss of train.freq_opt
    cri_contextual = None   # ContextualLoss of train.contextual_opt
    cri_ldl = None       # LDLLoss of train.ldl_opt
    output_ema = None    # net_g_ema's output on this step's input (steps that evaluate the LDL term)

    def _setup_ema(self):
        """train.ema_decay > 0 (sr_model.py:39-53): net_g_ema, a second network_g in eval mode without gradients, never wrapped in
        DDP (it is used for testing on one GPU and for saving), loaded from path.pretrain_network_g under the key params_ema
        (falling back to params) or else set to net_g's weights by an update with decay 0"""
        self.ema_decay = (self.opt.get('train') or {}).get('ema_decay', 0) or 0
        if not self.ema_decay > 0:
            return
        logging.getLogger('basicsr').info(f'Use Exponential Moving Average with decay: {self.ema_decay}')
        self.net_g_ema = build_network(self.opt['network_g']).to(self.device).eval()
        for p in self.net_g_ema.parameters():
            p.requires_grad_(False)
        path = self.opt.get('path') or {}
        if path.get('pretrain_network_g'):
            self.load_network(self.net_g_ema, path['pretrain_network_g'], path.get('strict_load', True), 'params_ema')
        else:
            self.model_ema(0)

    def model_ema(self, decay=0.999):
        """base_model.py:75-82: net_g_ema = decay * net_g_ema + (1 - decay) * net_g over the parameters, as ONE launch (hip.ema_multi)
        instead of a mul_ and an add_ per parameter; the job table is rebuilt only when a tensor has moved"""
        from .. import hip
        bare, ema = dict(self.get_bare_model(self.net_g).named_parameters()), dict(self.net_g_ema.named_parameters())
        emas = list(ema.values())
        self._ema_table = hip.optim_table([bare[k] for k in ema], emas=emas, cached=getattr(self, '_ema_table', None))
        hip.ema_multi(self._ema_table, decay, emas)

    def _step_g(self):
        """optimizer_g.step() and the EMA update behind it (sr_model.py:114-119); with train.hip_adam the step has written the EMA"""
        if not self._hip_adam_wanted():
            self._clip_gradients(self.optimizer_g, 'g')
        self.optimizer_g.step()
        if self._hip_adam_wanted():
            self._clip_gradients(self.optimizer_g, 'g')
        if self.net_g_ema is not None and not self._hip_adam_wanted():
            self.model_ema(self.ema_decay)

    def _step_d(self):
        """optimizer_d.step() behind train.grad_clip_norm_d / train.skip_nonfinite_steps"""
        if not self._hip_adam_wanted():
            self._clip_gradients(self.optimizer_d, 'd')
        self.optimizer_d.step()
        if self._hip_adam_wanted():
            self._clip_gradients(self.optimizer_d, 'd')

    # ------------------------------------------------------------------ set-up
    def init_training_settings(self):
        from .. import losses
        train_opt = self.opt['train']
        if train_opt.get('texture_opt') and not train_opt['texture_opt'].get('use_weights'):
            raise NotImplementedError("train.texture_opt: use_weights: true is required (without it the reference's TextureLoss.forward "
                                      'fails on a divisor it never sets; the weighted form is the one implemented)')
        net_d_opt = self.opt.get('network_d')
        if net_d_opt and net_d_opt.get('type') not in ('ImageDiscriminator', 'VGGStyleDiscriminator', 'UNetDiscriminatorSN',
                                                       'UNetDiscriminatorSN_basicsr', 'StyleGAN2Discriminator'):
            raise NotImplementedError(f"network_d: {net_d_opt.get('type')} is not implemented (ImageDiscriminator, VGGStyleDiscriminator, "
                                      "UNetDiscriminatorSN and StyleGAN2Discriminator are)")
        if net_d_opt and net_d_opt['type'].startswith('UNetDiscriminatorSN') and 'num_in_ch' not in net_d_opt:
            raise NotImplementedError(f"network_d: {net_d_opt['type']} without num_in_ch (the reference's constructor has no default for it)")
        if train_opt.get('gan_type') and not net_d_opt:
            raise NotImplementedError('train.gan_type without network_d: the reference builds a GAN loss that nothing uses (and fails on '
                                      'a missing grad_penalty_weight); give a network_d or drop gan_type')
        if net_d_opt and not train_opt.get('gan_type'):
            raise NotImplementedError('network_d without train.gan_type: the reference fails at its first D step; set gan_type')
        if train_opt.get('r1_reg_weight') and not net_d_opt:
            raise NotImplementedError('train.r1_reg_weight without network_d: R1 regularises a discriminator; give a network_d or drop '
                                      'r1_reg_weight')
        self._setup_d_augment(train_opt, net_d_opt)   # (a bad train.d_augment is refused before anything is built)
        # R1 on the real images every net_d_reg_every-th D step (stylegan2_model.py:75-79); 0: none
        self.r1_reg_weight = float(train_opt.get('r1_reg_weight') or 0)
        self.net_d_reg_every = int(train_opt.get('net_d_reg_every') or 1)
        # discriminator (ref :98-113), built and loaded before the losses
        self.net_d = self.cri_gan = self.cri_grad_penalty = None
        if net_d_opt:
            self.net_d = build_network(net_d_opt).to(self.device)
            path = self.opt.get('path') or {}
            if path.get('pretrain_network_d'):
                self.load_network(self.net_d, path['pretrain_network_d'], path.get('strict_load', True))
            if self.opt.get('dist', False):
                self.net_d = DistributedDataParallel(self.net_d, device_ids=[self.device.index],
                                                     find_unused_parameters=self.opt.get('find_unused_parameters', False),
                                                     broadcast_buffers=self.opt.get('broadcast_buffers', True))
            self.net_d.train()
            # GANLoss(gan_type, 1.0, 0.0, gan_weight) and the gradient penalty (ref :149-169: both keys are required)
            self.cri_gan = losses.GANLoss(train_opt['gan_type'], real_label_val=1.0, fake_label_val=0.0,
                                          loss_weight=train_opt['gan_weight']).to(self.device)
            if train_opt['grad_penalty_weight'] > 0:
                self.cri_grad_penalty = losses.GradientPenaltyLoss(loss_weight=train_opt['grad_penalty_weight']).to(self.device)
        if train_opt['pixel_weight'] > 0:
            name = train_opt['pixel_criterion']
            if name not in ('L1Loss', 'MSELoss', 'CharbonnierLoss'):
                raise NotImplementedError(f'pixel_criterion {name}: L1Loss, MSELoss or CharbonnierLoss')
            self.cri_pix = losses.LOSS_REGISTRY.get(name)(loss_weight=train_opt['pixel_weight'], reduction='mean').to(self.device)
        else:
            logging.getLogger('basicsr').info('Remove pixel loss.')
            self.cri_pix = None
        # two PerceptualLoss instances, each with its own VGG, as in the reference (:126-141)
        self.cri_perceptual = losses.PerceptualLoss(**train_opt['perceptual_opt']).to(self.device) if train_opt.get('perceptual_opt') else None
        self.cri_style = losses.PerceptualLoss(**train_opt['style_opt']).to(self.device) if train_opt.get('style_opt') else None
        # TextureLoss (ref :142-147); its maps and weights are built from the matcher's outputs in _texture_targets
        self.cri_texture = losses.TextureLoss(**train_opt['texture_opt']).to(self.device) if train_opt.get('texture_opt') else None
        # SSIMLoss: train.ssim_opt holds its constructor's keys (loss_weight, channel, window_size, sigma)
        self.cri_ssim = losses.SSIMLoss(**train_opt['ssim_opt']).to(self.device) if train_opt.get('ssim_opt') else None
        self.cri_msssim = self._build_msssim(train_opt)
        self.cri_ldl = self._build_ldl(train_opt)
        self.cri_freq = self._build_freq(train_opt)
        # ContextualLoss: train.contextual_opt holds its constructor's keys (layer_weights, vgg_type, use_input_norm, norm_img, band_width,
        # loss_weight, and CoBi's weight_sp, tap_stride = {layer: s}, rgb_patch = {size, stride, weight})
        self.cri_contextual = losses.ContextualLoss(**train_opt['contextual_opt']).to(self.device) if train_opt.get('contextual_opt') else None
        self.net_g_pretrain_steps = train_opt['net_g_pretrain_steps']
        self.net_d_steps = train_opt.get('net_d_steps', 1)
        self.net_d_init_steps = train_opt.get('net_d_init_steps', 0)
        if self.net_d is not None:   # ref :178-185: appended before the schedulers are made, so it gets one of its own
            self.optimizer_d = self._adam(self.net_d.parameters(), lr=train_opt['lr_d'], weight_decay=train_opt.get('weight_decay_d', 0),
                                                betas=train_opt['beta_d'],
                                                fused=bool(train_opt.get('fused_adam', True)) and self.device.type == 'cuda')
            self._setup_grad_clip(self.optimizer_d, 'd')
            self.optimizers.append(self.optimizer_d)
        sched = dict(train_opt['scheduler'])
        stype = sched.pop('type')
        if stype not in ('MultiStepLR', 'MultiStepRestartLR', 'CosineAnnealingRestartLR'):   # base_model.py:113-124
            raise NotImplementedError(f'Scheduler {stype} is not implemented yet.')
        for optimizer in self.optimizers:
            self.schedulers.append((_CosineAnnealingRestartLR if stype == 'CosineAnnealingRestartLR' else _MultiStepRestartLR)(optimizer, **sched))

    # ------------------------------------------------------------------ train.d_augment: the augmentation in front of every D call
    d_augment = d_adaptive = _d_aug_gen = None   # (the state of a model without the option)

    def _setup_d_augment(self, train_opt, net_d_opt):
        """train.d_augment {policy: [color, translation, cutout, flip] (a list or a comma-separated string; color = brightness,
        saturation and contrast), p: 1.0, brightness: 0.25, saturation: [0, 2], contrast: [0.5, 1.5], translation: 0.125, cutout: 0.5,
        adaptive: {target: 0.6, interval: 4, speed_kimg: 500}}: DiffAugment / ADA's pixel and colour operators on the kernels of
        csrc/disc_augment.hip, see archs/d_augment.py (parse_d_augment names what is refused; sample_d_augment the order of draws).
        The parameters come from a host generator seeded from manual_seed or, without one, from torch's global generator, as
        _pool_gen is.  No claim about image quality is made: only random-init weights were available offline."""
        from ..archs import d_augment as da
        self.d_augment = da.parse_d_augment(train_opt.get('d_augment'), has_net_d=bool(net_d_opt), gan_type=train_opt.get('gan_type'))
        self.d_adaptive = self._d_aug_gen = None
        if self.d_augment is None:
            return
        seed = self.opt.get('manual_seed')
        if seed is None:   # (from torch's global generator: reproducible behind torch.manual_seed)
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        self._d_aug_gen = torch.Generator().manual_seed(seed)
        if self.d_augment['adaptive'] is not None:
            self.d_adaptive = da.AdaptiveP(self.d_augment['p'], **self.d_augment['adaptive'])

    @property
    def _d(self):
        """what every discriminator call of the training step goes through.  Without train.d_augment it is net_d itself: the same
        object is called and handed to the gradient penalty.  With it, _d_augmented."""
        return self.net_d if self.d_augment is None else self._d_augmented

    def _d_augmented(self, x):
        """net_d(T(x)): a fresh set of parameters per call (one torch.rand on the host generator, one small upload), independently
        and in program order -- the D step's real images, its fake images, the WGAN-GP interpolate, the R1 real batch on regularised
        steps (the penalty's gradient is taken with respect to the images before the augmentation, as ADA does), the G step's fake
        images.  A range-fallback re-run of the G step calls this again and so draws again."""
        from ..archs import d_augment as da
        b, _, h, w = x.shape
        p = self.d_augment['p'] if self.d_adaptive is None else self.d_adaptive.p
        params = da.sample_d_augment(b, h, w, self.d_augment, p, self._d_aug_gen).to(x.device)
        return self.net_d(da.d_augment(x, params))

    @staticmethod
    def _build_msssim(train_opt):
        """train.msssim_opt holds MSSSIMLoss's constructor's keys (loss_weight, channel, weights, window_size, sigma) -> the criterion,
        or None without the option.  Unknown keys are refused by name."""
        from .. import losses
        msssim_opt = train_opt.get('msssim_opt')
        if not msssim_opt:
            return None
        unknown = sorted(set(msssim_opt) - {'loss_weight', 'channel', 'weights', 'window_size', 'sigma'})
        if unknown:
            raise ValueError(f'train.msssim_opt: unknown keys {unknown}; loss_weight, channel, weights, window_size, sigma')
        return losses.MSSSIMLoss(**msssim_opt)

    @staticmethod
    def _build_freq(train_opt):
        """train.freq_opt {type: FFTLoss | FocalFrequencyLoss, ...its constructor's keys} -> the criterion, or None without the option"""
        from .. import losses
        freq_opt = dict(train_opt.get('freq_opt') or {})
        if not freq_opt:
            return None
        kind = freq_opt.pop('type', None)
        if kind not in ('FFTLoss', 'FocalFrequencyLoss'):
            raise ValueError(f'train.freq_opt: type {kind!r}; FFTLoss or FocalFrequencyLoss')
        return losses.LOSS_REGISTRY.get(kind)(**freq_opt)

    @staticmethod
    def _build_ldl(train_opt):
        """train.ldl_opt in basicsr's form {type: L1Loss, loss_weight, reduction: mean} (sr_model.py builds an L1Loss that
        realesrgan_model.py:211-226 applies to the weighted images), plus an optional ksize: 7 -> LDLLoss, or None without the
        option.  It needs the EMA network: refused here, not at the first step, without train.ema_decay > 0."""
        from .. import losses
        ldl_opt = train_opt.get('ldl_opt')
        if not ldl_opt:
            return None
        unknown = sorted(set(ldl_opt) - {'type', 'loss_weight', 'reduction', 'ksize'})
        if unknown:
            raise ValueError(f'train.ldl_opt: unknown key(s) {unknown} (type, loss_weight, reduction and ksize are the options)')
        if ldl_opt.get('type', 'L1Loss') != 'L1Loss':
            raise NotImplementedError(f"train.ldl_opt: type {ldl_opt.get('type')!r}; the artifact loss is implemented as the L1 form "
                                      "(type: L1Loss) of the LDL paper and of basicsr's configurations")
        if ldl_opt.get('reduction', 'mean') != 'mean':
            raise NotImplementedError(f"train.ldl_opt: reduction {ldl_opt.get('reduction')!r}; only 'mean' is implemented")
        if not (train_opt.get('ema_decay') or 0) > 0:
            raise ValueError('train.ldl_opt without train.ema_decay > 0: the artifact loss compares the output with that of net_g_ema; '
                             'set ema_decay (e.g. 0.999) or drop ldl_opt')
        return losses.LDLLoss(loss_weight=ldl_opt.get('loss_weight', 1.0), ksize=ldl_opt.get('ksize', 7))

    @staticmethod
    def get_bare_model(net):
        return net.module if isinstance(net, DistributedDataParallel) else net

    # ------------------------------------------------------------------ data
    ref_valid_bits = None   # per-sample reference masks of the current batch: int32 [B] on the device (bit k = reference k present), None = all

    @staticmethod
    def check_ref_valid(ref_valid, b, k):
        """the host check of data['ref_valid'] ([B,K] bool / uint8): ValueError for a wrong shape or a sample without a valid
        reference; -> the packed int32 [B] words (host), or None for an all-true mask (archs/arch_util.ref_valid_words)"""
        from ..archs.arch_util import ref_valid_words
        return ref_valid_words(ref_valid, b, k)

    # ------------------------------------------------------------------ ref_select: each sample's K best of a pool of N references
    _REF_POOLS = True
    ref_pool = None        # the fed pool of a batch with N > top_k: dict(stack [N*B,3,H,W] n-major, bits int32 [B] / None, full, n)
    ref_selection = None   # after a pass over a pool: int32 [B,K] on the device, the chosen candidates in ascending n, -1 = unused slot
    ref_scores = None      # ... and fp32 [B,N], the candidates' scores (-inf: absent)

    @staticmethod
    def check_ref_select(opt):
        """opt['ref_select']: absent or None -> None; {top_k: int in 1..16, score: 'mean' (default) | 'wins'} -> (top_k, score);
        anything else -- a bool or non-int top_k, one outside 1..16, an unknown score, unknown keys -- is a ValueError"""
        rs = (opt or {}).get('ref_select')
        if rs is None:
            return None
        if not isinstance(rs, dict):
            raise ValueError(f'ref_select: {rs!r} is not a mapping with top_k (and optionally score)')
        unknown = sorted(set(rs) - {'top_k', 'score'})
        if unknown:
            raise ValueError(f'ref_select: unknown key(s) {unknown} (top_k and score are the options)')
        k = rs.get('top_k')
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f'ref_select.top_k: {k!r} is not an int of at least 1')
        if k > 16:
            raise ValueError(f'ref_select.top_k: {k} > 16, the limit of the reference masks')
        score = rs.get('score', 'mean')
        if score not in ('mean', 'wins'):
            raise ValueError(f"ref_select.score: {score!r} is not 'mean' or 'wins'")
        return k, score

    @staticmethod
    def check_ref_pool_valid(ref_valid, b, n):
        """check_ref_valid for a pool: [B,N] with N <= 32 -> the packed int32 [B] words (host; candidate 31 is the sign bit) or None
        for an all-true mask (archs/arch_util.ref_pool_words)"""
        from ..archs.arch_util import ref_pool_words
        return ref_pool_words(ref_valid, b, n)

    _pool_eager_logged = False

    def _pool_batch(self, what):
        """True for a batch with a reference pool: it does not take the hipGraph paths (the selection changes the pass's inputs)"""
        if self.ref_pool is None:
            return False
        if not MultiRefRestorationModel._pool_eager_logged:
            MultiRefRestorationModel._pool_eager_logged = True
            logging.getLogger('basicsr').info(f'{what}: batches with a reference pool (ref_select) run eagerly (no hipGraph capture or replay)')
        return True

    def _feed_pool(self, data, top_k):
        """feed_data's reference part for img_ref_list [B,N,...] with N > top_k: the pool is kept n-major, absent candidates as
        zero images; what a pass reads (img_ref_stack, num_refs, ref_valid_bits) is written by the selection of that pass"""
        b, n = data['img_ref_list'].shape[:2]
        if n > 32:
            raise ValueError(f'ref_select: a pool of N={n} candidate references > 32')
        words, full = None, True
        if data.get('ref_valid') is not None:
            words = self.check_ref_pool_valid(data['ref_valid'], b, n)
        if words is not None:   # does every sample fill its top_k slots?  (known here: the pass reads nothing back)
            full = min(bin(w & 0xffffffff).count('1') for w in words.tolist()) >= top_k
        bits = None if words is None else words.to(self.device)
        refs = data['img_ref_list'].to(self.device, non_blocking=True)
        if bits is not None:
            valid = ((bits[:, None] >> torch.arange(n, device=self.device, dtype=torch.int32)) & 1).bool()
            refs = torch.where(valid[:, :, None, None, None], refs, refs.new_zeros(()))
        self.ref_pool = dict(stack=refs.transpose(0, 1).reshape(-1, *refs.shape[2:]).contiguous(), bits=bits, full=full, n=n)
        self.num_refs, self.ref_valid_bits, self.img_ref_stack, self.img_ref_list = top_k, None, None, []

    def _select_from_pool(self):
        """extractor and matcher on the whole pool [N*B], scores and the per-sample choice on the device (hip.ref_select), the chosen
        images gathered to the k-major stack [K*B] with zeros in unused slots: sets img_ref_stack / img_ref_list / ref_valid_bits (None
        when every sample fills its K slots) / ref_selection / ref_scores -> (max_idx, max_val of the pool, for the caller to gather; the match maps' (h, w))"""
        from .. import hip
        pool, (k, score) = self.ref_pool, self.ref_select
        with torch.no_grad():
            f1, f2 = self.net_extractor.forward_stacked(self.match_img_in, pool['stack'])
            idx, val = self.net_map.match(f1, f2)
            idx, val = idx.contiguous(), val.contiguous()
            sel, slot_bits, scores = hip.ref_select(val.view(pool['n'], -1, *val.shape[1:]), pool['bits'], k, score)
            refs = hip.ref_gather(pool['stack'], sel, pool['n'])
        self.ref_selection, self.ref_scores = sel, scores
        self.num_refs, self.ref_valid_bits = k, None if pool['full'] else slot_bits
        self.img_ref_stack = refs
        self.img_ref_list = list(refs.view(k, -1, *refs.shape[1:]).unbind(0))
        return idx, val, f1.shape[2:]

    def _forward_pool(self):
        """_forward over a reference pool: offsets, VGG19 maps and net_g run on the K chosen references of each sample only"""
        from .. import hip
        hip.amax_pool_reset()
        idx, val, (h, w) = self._select_from_pool()
        k, n = self.num_refs, self.ref_pool['n']
        with torch.no_grad():
            self.max_idx, self.max_val = hip.ref_gather(idx, self.ref_selection, n), hip.ref_gather(val, self.ref_selection, n)
            pre_offset = self.net_map.offsets_from_idx(self.max_idx, h, w)
            img_ref_feat = self.net_map.vgg(self.img_ref_stack)
            if self.cri_texture is not None:
                self.img_ref_feat = img_ref_feat
        if self.ref_valid_bits is not None:
            return self._run_net_g(self.img_in_lq, pre_offset, img_ref_feat, k=k, ref_valid=self.ref_valid_bits)
        return self._run_net_g(self.img_in_lq, pre_offset, img_ref_feat, k=k)

    _masked_eager_logged = False

    def _masked_batch(self, what):
        """True for a batch with an absent reference: it does not take the hipGraph paths (the mask is not part of a capture key)"""
        if self.ref_valid_bits is None:
            return False
        if not MultiRefRestorationModel._masked_eager_logged:
            MultiRefRestorationModel._masked_eager_logged = True
            logging.getLogger('basicsr').info(f'{what}: batches with a ref_valid mask run eagerly (no hipGraph capture or replay)')
        return True

    def feed_data(self, data):
        """data: img_in_lq (B,3,h,w), img_in_up (B,3,4h,4w), img_ref_list (B,K,3,4h,4w), img_in (B,3,4h,4w)
        (the dict of multi_ref_dataset.py:127-134); optionally ref_valid (B,K) bool / uint8: reference k of sample b is absent
        where it is false -- the sample is restored from its valid references alone, whatever the loader put in the absent slot.
        With the ref_select option and K = N > top_k (N <= 32) the references are a pool: every pass picks each sample's top_k best
        present candidates on the device (_forward_pool) and restores from those."""
        self.ref_pool = self.ref_selection = self.ref_scores = None
        self.gt_usm = None
        self.valid_sizes = self._valid_sizes_of(data)
        self._gt_fed = 'img_in' in data   # (self.gt may be an earlier batch's)
        if self._synthesise:   # opt['degradation'], training batches only: img_in_lq and img_in_up are made from img_in
            data = self._degrade(data)
        if self.ref_select is not None and data['img_ref_list'].shape[1] > self.ref_select[0]:
            self._feed_pool(data, self.ref_select[0])   # (checked on the host before anything is launched)
            self.ref_pool['stack'] = self._ref_views(self.ref_pool['stack'], self.ref_pool['n'])
            self.img_in_lq = data['img_in_lq'].to(self.device, non_blocking=True)
            if 'img_in' in data:
                self.gt = data['img_in'].to(self.device, non_blocking=True)
            self.match_img_in = data['img_in_up'].to(self.device, non_blocking=True)
            return
        words = None
        if data.get('ref_valid') is not None:   # (checked on the host before anything is launched)
            words = self.check_ref_valid(data['ref_valid'], *data['img_ref_list'].shape[:2])
        self.ref_valid_bits = None if words is None else words.to(self.device)
        self.img_in_lq = data['img_in_lq'].to(self.device, non_blocking=True)
        refs = data['img_ref_list'].to(self.device, non_blocking=True)
        self.num_refs = refs.shape[1]
        if words is not None:
            # absent references become zero images (a select, not a product: NaN filler goes too), so that the frozen networks, the
            # fp16-range flag and the batch-wide input scales do not depend on the loader's filler
            valid = ((self.ref_valid_bits[:, None] >> torch.arange(self.num_refs, device=self.device, dtype=torch.int32)) & 1).bool()
            refs = torch.where(valid[:, :, None, None, None], refs, refs.new_zeros(()))
        # k-major stack [K*B,3,H,W]; the reference's list(torch.unbind(dim=1)) is its K slices
        self.img_ref_stack = self._ref_views(refs.transpose(0, 1).reshape(-1, *refs.shape[2:]).contiguous(), self.num_refs)
        self.img_ref_list = list(self.img_ref_stack.view(self.num_refs, -1, *refs.shape[2:]).unbind(0))
        if 'img_in' in data:
            self.gt = data['img_in'].to(self.device, non_blocking=True)
        self.match_img_in = data['img_in_up'].to(self.device, non_blocking=True)

    # ------------------------------------------------------------------ the hot path
    def _forward(self):
        if self.ref_pool is not None:
            return self._forward_pool()
        k = self.num_refs
        from .. import hip
        hip.amax_pool_reset()   # the max |out| words of this pass's launches (archs/nhwc.py: Winograd input scales): zeroed, slot 0
        with torch.no_grad():
            f1, f2 = self.net_extractor.forward_stacked(self.match_img_in, self.img_ref_stack)
            pre_offset, img_ref_feat = self._match(f1, f2, self.img_ref_stack)
        if self.ref_valid_bits is not None:
            return self._run_net_g(self.img_in_lq, pre_offset, img_ref_feat, k=k, ref_valid=self.ref_valid_bits)
        return self._run_net_g(self.img_in_lq, pre_offset, img_ref_feat, k=k)

    def _run_net_g(self, *args, **kwargs):
        """net_g on what the frozen networks produced; with an LDL loss the arguments are kept for the EMA pass of this step
        (_ema_pass), as _match keeps the reference maps for the texture loss"""
        if self.cri_ldl is not None:
            self._net_g_inputs = (args, kwargs)
        return self.net_g(*args, **kwargs)

    def _ema_pass(self):
        """net_g_ema, in eval mode and without a graph, on the inputs net_g has just had in this step's _forward: the same LR
        images, pre_offset, reference VGG maps, k and ref_valid words (the matcher is frozen: recomputing them, as
        realesrgan_model.py:211-226 does, would give the same tensors) -> its output, the bits test() would produce for this batch.
        It runs on the inference engine with the weights net_g_ema has BEFORE this step's update; their packed copies come from
        the versioned cache of hip.packed_weight, re-packed here because the last step's EMA update moved every version.
        Left alone: net_g (its train mode, the _offset_count guards of its DynAgg modules -- net_g_ema has its own) and the
        max |out| words of the recorded forward: the pass takes fresh slots of hip's pool behind them, without resetting it."""
        from .. import hip
        if self.net_g_ema is None:
            raise RuntimeError('train.ldl_opt: there is no net_g_ema (train.ema_decay > 0 is required)')
        args, kwargs = self._net_g_inputs
        with torch.no_grad(), hip.amax_ring(self.device).one_half('train.ldl_opt'):
            out = self.net_g_ema(*args, **kwargs)
        return out.detach()

    def _match(self, f1, f2, refs):
        """net_map on the extractor's features and the reference images: -> (pre_offset, the references' VGG maps); max_idx is kept,
        and with a texture loss also max_val and the maps (_texture_targets reads them)"""
        if self.cri_texture is not None:
            pre_offset, self.max_idx, self.max_val = self.net_map.offsets(f1, f2, want_val=True)
        else:
            pre_offset, self.max_idx = self.net_map.offsets(f1, f2)
        img_ref_feat = self.net_map.vgg(refs)
        if self.cri_texture is not None:
            self.img_ref_feat = img_ref_feat
        return pre_offset, img_ref_feat

    range_fallbacks = 0   # batches re-run on the range-free kernels because an activation left the fp16 range

    def _range_tripped(self, what):
        """the default kernels split fp32 operands into fp16 pairs (|activation| < 65504) and raise a device flag
        otherwise: one 4-byte readback per batch; True -> the caller re-runs the batch under hip.range_free()"""
        from .. import hip
        if not hip.conv_range_tripped():
            return False
        self.range_fallbacks += 1
        logging.getLogger('basicsr').warning(
            f'{what}: an activation left the fp16 range of the split kernels; batch re-run on the bf16 three-term kernels '
            f'(no range limit, ~1.5x slower); {self.range_fallbacks} such batch(es) so far')
        return True

    def _rerun_range_free(self, what, body, default=None, zero_grad=False, frozen_d=False, reset_scales=True, tripped=None):
        """the fallback of every pass that reads the fp16-range flag: if it is set (``tripped`` None: read here, one 4-byte readback;
        test() has read it already), the cached weight scales are dropped (not in test(): it trains nothing), net_g's gradients are
        zeroed on request, body() runs again under hip.range_free() -- with D's running statistics frozen when the D step has already
        been taken -- and the flag is read once more to clear it.  Returns body()'s value, or ``default`` when nothing tripped."""
        from .. import hip
        from ..archs import nhwc_disc, nhwc_train
        if not (self._range_tripped(what) if tripped is None else tripped):
            return default
        if reset_scales:
            nhwc_train.reset_scales()
        if zero_grad:
            self.optimizer_g.zero_grad()
        with hip.range_free(), (nhwc_disc.frozen_statistics() if frozen_d else contextlib.nullcontext()):
            out = body()
        hip.conv_range_tripped()
        return out

    def _texture_targets(self):
        """(maps, weights) of TextureLoss.forward, which the reference model reads and never sets: per match position
        the present reference with the largest match value (hip.texture_select), weights = that value, maps = its matched 3s x 3s
        patches of net_map.vgg's reference maps pasted at the position, overlaps averaged (hip.texture_swap_nhwc, on the maps where
        they lie).  maps: {layer: [B,C,s h,s w]} (NCHW views of channels-last storage), weights [B,1,h-2,w-2]."""
        from .. import hip
        from ..archs.nhwc_train import TEXTURE_LAYERS
        k = self.num_refs
        idx = self.max_idx.reshape(k, -1, *self.max_idx.shape[1:]).contiguous()
        val = self.max_val.reshape(idx.shape).contiguous()
        with torch.no_grad():
            sel, weights, pidx = hip.texture_select(idx, val, self.ref_valid_bits)
            maps = {}
            for name in self.cri_texture.vgg.layer_name_list:
                feat = self.img_ref_feat[name].permute(0, 2, 3, 1).contiguous()   # (no copy: the engine's maps are channels-last)
                maps[name] = hip.texture_swap_nhwc(feat, sel, pidx, k, TEXTURE_LAYERS[name][0]).permute(0, 3, 1, 2)
        return maps, weights

    def _loss_and_backward(self, step):
        """net_g's losses of ref :197-279 and their backward: returns True when a gradient was produced (the optimiser may step)"""
        if step <= self.net_g_pretrain_steps:
            l_pix = self.cri_pix(self.output, self._gt_for('l1'))
            l_pix.backward()
            self.log_dict['l_pix'] = l_pix.detach()
            return True
        if (step - self.net_g_pretrain_steps) % self.net_d_steps == 0 and \
                (step - self.net_g_pretrain_steps) > self.net_d_init_steps:
            l_g_total = 0
            if self.cri_pix is not None:
                l_g_pix = self.cri_pix(self.output, self._gt_for('l1'))
                l_g_total = l_g_total + l_g_pix
                self.log_dict['l_g_pix'] = l_g_pix.detach()
            if self.cri_perceptual is not None:
                l_g_percep, _ = self.cri_perceptual(self.output, self._gt_for('percep'))
                l_g_total = l_g_total + l_g_percep
                self.log_dict['l_g_percep'] = l_g_percep.detach()
            if self.cri_style is not None:
                _, l_g_style = self.cri_style(self.output, self._gt_for('percep'))
                l_g_total = l_g_total + l_g_style
                self.log_dict['l_g_style'] = l_g_style.detach()
            if self.cri_texture is not None:   # ref :265-269
                l_g_texture = self.cri_texture(self.output, *self._texture_targets())
                l_g_total = l_g_total + l_g_texture
                self.log_dict['l_g_texture'] = l_g_texture.detach()
            if self.cri_contextual is not None:
                l_g_contextual = self.cri_contextual(self.output, self._gt_for('percep'))
                l_g_total = l_g_total + l_g_contextual
                self.log_dict['l_g_contextual'] = l_g_contextual.detach()
            if self.cri_ssim is not None:
                l_g_ssim = self.cri_ssim(self.output, self._gt_for('l1'))
                l_g_total = l_g_total + l_g_ssim
                self.log_dict['l_g_ssim'] = l_g_ssim.detach()
            if self.cri_msssim is not None:
                l_g_msssim = self.cri_msssim(self.output, self._gt_for('l1'))
                l_g_total = l_g_total + l_g_msssim
                self.log_dict['l_g_msssim'] = l_g_msssim.detach()
            if self.cri_ldl is not None:   # realesrgan_model.py:211-226
                self.output_ema = self._ema_pass()
                l_g_ldl = self.cri_ldl(self.output, self._gt_for('l1'), self.output_ema)
                l_g_total = l_g_total + l_g_ldl
                self.log_dict['l_g_ldl'] = l_g_ldl.detach()
            if self.cri_freq is not None:
                l_g_freq = self.cri_freq(self.output, self._gt_for('l1'))
                l_g_total = l_g_total + l_g_freq
                self.log_dict['l_g_freq'] = l_g_freq.detach()
            if self.net_d is not None:   # ref :272-276 (D's parameters are frozen: no weight gradient of D is computed)
                fake_g_pred = self._d(self.output)
                l_g_gan = self.cri_gan(fake_g_pred, True, is_disc=False)
                l_g_total = l_g_total + l_g_gan
                self.log_dict['l_g_gan'] = l_g_gan.detach()
            l_g_total.backward()
            return True
        return False

    def _forward_backward(self, step):
        self.output = self._forward()
        return self._loss_and_backward(step)

    # ------------------------------------------------------------------ hipGraph replay of the training step
    def _train_graph_wanted(self):
        """opt['train']['hip_graph'] or MREFSR_TRAIN_GRAPH=1 (EXPERIMENTAL, off by default: 1-2 % at the shipped patch size; see the
        fence at the end of _optimize_graphed): forward + backward are captured once per input shape and replayed; the Adam update is
        a second graph, replayed after the fp16-range flag has been read.  Single process only (a DDP all-reduce is not captured), and
        not with a perceptual, style or texture loss (their VGG node is not captured), an SSIM or MS-SSIM loss, an LDL loss (its EMA pass is not
        captured), a frequency-domain loss, a contextual loss (a VGG node again), nor with a discriminator."""
        train_opt = self.opt.get('train') or {}
        return (bool(train_opt.get('hip_graph')) or os.environ.get('MREFSR_TRAIN_GRAPH', '0') == '1') \
            and not self.opt.get('dist', False) and not train_opt.get('perceptual_opt') and not train_opt.get('style_opt') \
            and not train_opt.get('texture_opt') and not train_opt.get('ssim_opt') and not train_opt.get('msssim_opt') \
            and not train_opt.get('ldl_opt') \
            and not train_opt.get('freq_opt') and not train_opt.get('contextual_opt') \
            and not self.opt.get('network_d')

    _TRAIN_INPUTS = ('img_in_lq', 'match_img_in', 'img_ref_stack', 'gt')

    def _train_inputs(self):
        """the tensors a captured training step reads: with a synthesised batch the USM-sharpened GT as well"""
        return self._TRAIN_INPUTS + (('gt_usm',) if self.gt_usm is not None else ())
    _GRAPH_WARMUP = 3   # eager steps per input shape before capture (lazy kernel attributes, workspaces, MIOpen find results)

    def _optimize_graphed(self, step):
        """True when the step was taken by graph replay"""
        from .. import hip
        from ..archs import nhwc_train
        if step <= self.net_g_pretrain_steps or self.net_d_steps != 1 or step <= self.net_g_pretrain_steps + self.net_d_init_steps:
            return False   # (the phases of ref :197-279 differ in what they run and log: only the steady one is captured)
        # (the learning rates are NOT part of the key: the captured update reads them from device tensors, refreshed below when a
        # scheduler has moved them -- update_learning_rate with warm-up, base_model.py:172-193, moves them every iteration)
        key = (self._train_inputs(), tuple(tuple(getattr(self, n).shape) for n in self._train_inputs()), self.num_refs, hip.packed_epoch(), nhwc_train.scale_epoch())
        st = self.__dict__.setdefault('_tgraph', {'key': None})
        if st['key'] != key:
            changes = st.get('changes', 0) + (st['key'] is not None)
            st.clear()
            st.update(key=key, eager=0, fb=None, changes=changes)
            hip.release_capture_workspaces()
            if changes == 8:   # e.g. a scheduler that moves the learning rate every iteration: the key never settles
                logging.getLogger('basicsr').warning(
                    'hip_graph (training): the capture key (input shapes, weight scales) keeps changing; steps run eagerly.')
        if st['fb'] is None:
            if st['eager'] < self._GRAPH_WARMUP:
                st['eager'] += 1
                return False
            static = {n: getattr(self, n).clone() for n in self._train_inputs()}
            for n, t in static.items():
                setattr(self, n, t)
            dyn = [m for m in self.net_g.modules() if hasattr(m, '_offset_count')]
            before = [m._offset_count for m in dyn]
            # nothing may keep the eager steps' autograd graphs (and their AccumulateGrad nodes, bound to the eager stream) alive
            self.output = None
            self.optimizer_g.zero_grad(set_to_none=True)
            import gc
            gc.collect()
            logging.getLogger('basicsr').warning(
                'hip_graph (training) is EXPERIMENTAL: hipStreamSynchronize is called behind every replayed update (without it the runtime of '
                'ROCm 7.2 faults after 25-50 graph launches: profiles/r5_train_graph_replay_fault.txt)')
            fb, upd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            lr_val = [float(pg['lr']) for pg in self.optimizer_g.param_groups]
            lr_dev = [torch.tensor(v, device=self.device, dtype=torch.float32) for v in lr_val]
            try:
                with torch.cuda.graph(fb):
                    nhwc_train.begin_step()   # the packed weight copies are refreshed by the graph itself (one launch)
                    self._forward_backward(step)
                for pg, t in zip(self.optimizer_g.param_groups, lr_dev):
                    pg['lr'] = t           # the captured update reads its learning rates from device memory ...
                with torch.cuda.graph(upd, pool=fb.pool()):
                    self.optimizer_g.step()
            finally:
                for pg, v in zip(self.optimizer_g.param_groups, lr_val):
                    pg['lr'] = v       # ... while the schedulers keep working on plain numbers
            keep, ptrs = nhwc_train.capture_state()
            # the graphs have baked in addresses of eagerly allocated buffers that global caches own (pack job table, packed copies,
            # workspaces, zero chunks): they live as long as the graphs, and a replay is refused once any of them has moved
            st.update(fb=fb, upd=upd, static=static, out=self.output, idx=self.max_idx, log=dict(self.log_dict), dyn=dyn,
                      counts=[m._offset_count - b for m, b in zip(dyn, before)], keep=(keep, hip.capture_refs()), ptrs=ptrs, lr_val=lr_val, lr_dev=lr_dev)
        else:
            if nhwc_train.capture_state()[1] != st['ptrs']:   # (an eager pass in between rebuilt the pack table / a parameter moved)
                logging.getLogger('basicsr').warning('hip_graph (training): a buffer the captured step reads has moved; recapturing')
                st.clear()
                st.update(key=None)
                return False
            for n in self._train_inputs():
                st['static'][n].copy_(getattr(self, n))
                setattr(self, n, st['static'][n])
            for m, c in zip(st['dyn'], st['counts']):
                m._offset_count += c
        for i, pg in enumerate(self.optimizer_g.param_groups):   # a scheduler has moved a learning rate: one 4-byte fill, the graphs stay
            v = float(pg['lr'])
            if v != st['lr_val'][i]:
                st['lr_dev'][i].fill_(v)
                st['lr_val'][i] = v
        st['fb'].replay()
        self.output, self.max_idx = st['out'], st['idx']
        self.log_dict.update(st['log'])
        # rare: redo this step eagerly on the range-free kernels (None: nothing tripped)
        stepped = self._rerun_range_free('optimize_parameters', lambda: self._forward_backward(step), zero_grad=True)
        if stepped is not None:
            if stepped:
                self._step_g()
            return True
        st['upd'].replay()
        # hipStreamSynchronize behind the update graph.  Without it a run of replayed steps ends in a GPU memory access fault after
        # 25-50 replays (ROCm 7.2; never in eager mode).  It is not an ordering fence: an event recorded here and waited for on the
        # host (the GPU provably idle at the next launch), or a 20-ms sleep, do NOT remove the fault, hipStreamSynchronize /
        # hipDeviceSynchronize do; the update graph in a pool of its own, or forward + backward + update as ONE executable, fault
        # alike; every fault address is page 0x37 / 0x38 of a 2-MB block (220 KB = the kernel-argument segments of one launch of this
        # ~700-node graph).  What the call does is make the runtime retire its per-launch bookkeeping of completed graph launches
        # (profiles/r5_train_graph_replay_fault.txt, profiles/r4_train_graph_replay_fault.txt).  Cost: ~0.2 ms of host work not
        # overlapped.
        torch.cuda.current_stream().synchronize()
        return True

    def _discriminator_step(self, step):
        """ref :219-245: D on the GT and on the detached output, the gradient penalty, backward, optimizer_d.step().  With
        train.r1_reg_weight, on the steps that net_d_reg_every divides, the R1 lines of stylegan2_model.py:208-219 stand between that
        backward and the one optimizer_d.step(): the update, its clipping and its non-finite check see the sum of both gradients.
        The extra forward on the real images moves ImageDiscriminator's and VGGStyleDiscriminator's BatchNorm running statistics and
        UNetDiscriminatorSN's power-iteration vectors once more, as the torch modules would under the same lines.  log_dict holds
        l_d_r1 after a regularised step only: a plain step takes the last one's value out (stylegan2_model.py builds its log anew
        every iteration)."""
        self.optimizer_d.zero_grad()
        for p in self.net_d.parameters():
            p.requires_grad = True
        gan_gt = self._gt_for('gan')
        real_d_pred = self._d(gan_gt)
        if self.d_adaptive is not None:   # (two words on the device; read back every adaptive.interval-th step below)
            self.d_adaptive.accumulate(real_d_pred)
        l_d_real = self.cri_gan(real_d_pred, True, is_disc=True)
        self.log_dict['l_d_real'] = l_d_real.detach()
        self.log_dict['out_d_real'] = torch.mean(real_d_pred.detach())
        fake_d_pred = self._d(self.output.detach())
        l_d_fake = self.cri_gan(fake_d_pred, False, is_disc=True)
        self.log_dict['l_d_fake'] = l_d_fake.detach()
        self.log_dict['out_d_fake'] = torch.mean(fake_d_pred.detach())
        l_d_total = l_d_real + l_d_fake
        if self.cri_grad_penalty is not None:
            l_grad_penalty = self.cri_grad_penalty(self._d, gan_gt, self.output)
            self.log_dict['l_grad_penalty'] = l_grad_penalty.detach()
            l_d_total = l_d_total + l_grad_penalty
        l_d_total.backward()
        if self.r1_reg_weight > 0 and step % self.net_d_reg_every == 0:
            from ..losses import r1_penalty
            real_img = gan_gt.detach().requires_grad_(True)   # a leaf of its own on the GT's storage (D only reads it)
            real_pred = self._d(real_img)
            l_d_r1 = r1_penalty(real_pred, real_img)
            # (0 * real_pred[0]: every output of D takes part in this backward, which is what DDP's reducer asks for)
            l_d_r1 = self.r1_reg_weight / 2 * l_d_r1 * self.net_d_reg_every + 0 * real_pred[0]
            self.log_dict['l_d_r1'] = l_d_r1.detach().mean()
            l_d_r1.backward()
        elif self.r1_reg_weight > 0:
            self.log_dict.pop('l_d_r1', None)   # a plain step of the lazy schedule: not the value of an earlier regularised step
        self._step_d()
        if self.d_adaptive is not None:
            self.d_adaptive.step()
            self.log_dict['d_aug_p'] = self.d_adaptive.p
            if self.d_adaptive.rt is not None:
                self.log_dict['d_aug_rt'] = self.d_adaptive.rt
        for p in self.net_d.parameters():   # ref :249-251, before the G step
            p.requires_grad = False

    # ------------------------------------------------------------------ bit-reproducible steps
    def _deterministic_wanted(self):
        """opt['train']['deterministic'], or the process-wide switch (hip.set_deterministic / torch.use_deterministic_algorithms):
        net_g's gradient reductions are added in a fixed order, two runs from one seed produce the same bits"""
        from .. import hip
        return bool((self.opt.get('train') or {}).get('deterministic')) or hip.is_deterministic()

    def _check_deterministic_options(self):
        """the deterministic mode and the (experimental) hipGraph replay of the training step are not offered together: refused, not
        one of them dropped"""
        if self._deterministic_wanted() and self._train_graph_wanted():
            raise ValueError('train.deterministic (or torch.use_deterministic_algorithms(True)) cannot be combined with train.hip_graph / '
                             'MREFSR_TRAIN_GRAPH=1: the graph replay of the training step is experimental and is not covered by the '
                             'bit-reproducibility tests; turn one of the two off')

    _deterministic_logged = False

    def optimize_parameters(self, step):
        from .. import hip
        if not self._deterministic_wanted():
            return self._optimize_parameters(step)
        self._check_deterministic_options()   # (torch's flag may have been set after construction)
        if not self._deterministic_logged:
            self._deterministic_logged = True
            logging.getLogger('basicsr').info('deterministic training step: the bias / PReLU / per-channel gradient sums of net_g are added '
                                              'in a fixed order (bitwise reproducible from run to run)')
        with hip.deterministic(True):   # (the range-fallback re-run of the step happens inside)
            return self._optimize_parameters(step)

    def _optimize_parameters(self, step):
        from ..archs import nhwc_train
        if self.cri_msssim is not None:   # (on the host, before anything is launched: a GT too small for the levels is an error)
            self.cri_msssim.check_size(*self._gt_for('l1').shape[2:])
        nhwc_train.check_scales()   # cached fp16 weight scales of the training convolutions still valid? (device side)
        if self._train_graph_wanted() and not self._pool_batch('train.hip_graph') and not self._masked_batch('train.hip_graph') \
                and self._optimize_graphed(step):
            return
        self.optimizer_g.zero_grad()
        nhwc_train.begin_step()     # every packed copy of net_g's weights refreshed in one launch (they changed in optimizer_g.step())
        self.output = self._forward()
        adversarial = getattr(self, 'net_d', None) is not None and step > self.net_g_pretrain_steps
        if adversarial:
            # The fp16-range flag is read right after net_g's forward (one 4-byte readback), so that a forward re-run on the range-free
            # kernels happens before the D step: D's Adam step and each BatchNorm's running statistics are updated once per D forward
            # of the reference.  Should net_g's backward trip the flag below, the G step is re-run with D's running statistics left as
            # they are (the D step is not repeated).
            self.output = self._rerun_range_free('optimize_parameters', self._forward, self.output)
            self._discriminator_step(step)
        stepped = self._loss_and_backward(step)
        # (the frozen feature networks and the DCN forward run on the split kernels too)
        stepped = self._rerun_range_free('optimize_parameters', lambda: self._forward_backward(step), stepped, zero_grad=True,
                                         frozen_d=adversarial)
        if stepped:
            self._step_g()

    def test(self):
        run = self._test_self_ensemble if self.check_self_ensemble(self.opt.get('val')) else self._test
        if self.net_g_ema is None:
            run()
        else:
            net_g, self.net_g = self.net_g, self.net_g_ema   # sr_model.py:121-125: the EMA weights are the ones tested (and shipped)
            try:
                run()
            finally:
                self.net_g = net_g
        self._apply_color_fix()

    # ------------------------------------------------------------------ val.color_fix: the output's colours from the LQ image
    _color_fix_logged = False
    color_fix_cfg = valid_sizes = None   # (set by __init__ / feed_data)

    @staticmethod
    def _valid_sizes_of(data):
        """the un-padded image sizes of a fed batch: with a truthy ``padding`` and an ``original_size`` -- (h, w[, ...]), each an int
        or one value per sample, as MultiRefCUFEDSet reports them and a DataLoader collates them -- B pairs [h_b, w_b]; else None"""
        pad = data.get('padding')
        if pad is None or data.get('original_size') is None or not bool(torch.as_tensor(pad).any()):
            return None
        b = data['img_in_lq'].shape[0]
        h, w = (torch.as_tensor(v).reshape(-1).tolist() for v in tuple(data['original_size'])[:2])
        if len(h) not in (1, b) or len(w) not in (1, b):
            raise ValueError(f'original_size: (h, w) with one value or {b} values each expected for a batch of {b}, got '
                             f'{data["original_size"]!r}')
        return [[int(h[i % len(h)]), int(w[i % len(w)])] for i in range(b)]

    def _apply_color_fix(self):
        """val.color_fix (color_fix.py): the last step of test(), once, on the final output -- behind the range fallback, the
        packed-weights re-run, the merge of val.self_ensemble and a replayed hipGraph (it is not part of the capture) -- with
        match_img_in, the bicubic-upsampled LQ, as the colour source and the batch's un-padded sizes as the valid rectangles.
        Without the option nothing is launched and the output keeps its bits."""
        if self.color_fix_cfg is None:
            return
        if not MultiRefRestorationModel._color_fix_logged:
            MultiRefRestorationModel._color_fix_logged = True
            logging.getLogger('basicsr').info(f'val.color_fix: test() takes the colours of its output from the LQ image ({self.color_fix_cfg})')
        with torch.no_grad():
            self.output = color_fix(self.output, self.match_img_in, self.color_fix_cfg, self.valid_sizes)

    # ------------------------------------------------------------------ homography views of the references (views.py, csrc/warp.hip)
    ref_augment = ref_perturb_cfg = match_probe_cfg = _ref_aug_gen = None   # (the state of a model without the options)
    _validating = False   # inside validation: training-side options are off, validation-side options on
    _view_index = 0       # images fed since validation began: what the seeded views of val.ref_perturb / val.match_probe count
    _view_base = 0        # ... and the index of the fed batch's first image
    _gt_fed = False       # the fed batch had an img_in (feed_data)

    def _setup_ref_views(self, opt):
        """Three options on hip.warp_perspective; each is parsed here, at construction (views.parse_* name what is refused), and
        without them no launch of feed_data, test(), validation or the training step changes.

        train.ref_augment {p: 0.5, perturb: [5, 20], window: null, interp: bicubic}: in feed_data of TRAINING batches only
        (validation leaves it out, the way it puts _synthesise back), each (sample, reference) image is replaced with probability
        p by its view under a random corner homography (views.sample_corner_homographies: the reference's
        image_pair_generation_perspective), clamped to [0, 1].  It acts on the k-major stack, or on the pool stack under ref_select,
        after absent references have been zeroed (a zero image stays zero); one launch and one small upload per batch, none when no
        image was chosen.  The matrices come from a host generator seeded from manual_seed or, without one, from torch's global
        generator, as _d_aug_gen is (views.sample_ref_augment states the order of draws).  The input, the GT and img_in_up are
        untouched.

        val.ref_perturb {scale: 1.0, rotate: 0} or {perturb: [lo, hi], seed: 0, window: null} (either with interp): the references
        of every validation / test batch (a model that is not training, or validation of one that is) are replaced in feed_data,
        before anything else runs, by their view scaled and rotated about the image centre (views.similarity; degrees) or under a
        corner homography that depends on (seed, image index, k) only -- image index counted from 0 since validation began, 0 for
        the first image of a batch fed outside validation.  Clamped to [0, 1].  Metrics and logs are the usual ones.

        val.match_probe {perturb: [5, 20], window: null, thresholds: [1, 2], margin: 3, source: gt | lq_up, seed: 0, interp: bicubic}
        (or true): see _match_probe_stats.

        No claim about image or matching quality is made: only random-init weights were available offline."""
        self.ref_perturb_cfg = views.parse_ref_perturb(opt.get('val'))
        self.match_probe_cfg = views.parse_match_probe(opt.get('val'))
        self.ref_augment = views.parse_ref_augment(opt.get('train'))   # (refused in a test-only configuration too ...)
        if not opt.get('is_train'):
            self.ref_augment = None   # (... and used by a training model only)
        self._ref_aug_gen = None
        if self.ref_augment is not None:
            seed = opt.get('manual_seed')
            if seed is None:   # (from torch's global generator: reproducible behind torch.manual_seed)
                seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
            self._ref_aug_gen = torch.Generator().manual_seed(seed)

    def _ref_views(self, stack, k):
        """feed_data's reference stack [k*B,3,H,W] (k-major) -> the stack the batch is run on: under train.ref_augment (training
        batches) or val.ref_perturb (validation / test batches) its views, else the stack itself.  Also notes the batch's place in
        the count of validation images."""
        from .. import hip
        n, _, h, w = stack.shape
        b = n // k
        training = bool(self.is_train) and not self._validating
        self._view_base = self._view_index
        if self._validating:
            self._view_index += b
        if training:
            if self.ref_augment is None:
                return stack
            cfg = self.ref_augment
            sampling = views.sample_ref_augment(n, h, w, cfg, self._ref_aug_gen)
            if sampling is None:
                return stack
        else:
            if self.ref_perturb_cfg is None:
                return stack
            cfg = self.ref_perturb_cfg
            if cfg['kind'] == 'similarity':
                sampling = views.similarity(h, w, cfg['scale'], cfg['rotate'])
            else:   # image b of the batch: the k matrices of its own generator; entry k' * B + b of the k-major stack
                per_image = [views.indexed_corner_homographies(cfg['seed'], self._view_base + i, k, h, w, cfg['perturb'], cfg['window'])
                             for i in range(b)]
                sampling = torch.stack(per_image, dim=1).reshape(n, 3, 3)
        with torch.no_grad():
            return hip.warp_perspective(stack.contiguous(), sampling, interp=cfg['interp'], clamp=True)

    def _extract_pair(self, image1, images2):
        """the frozen extractor's two stacks: image1 [B,...] through the LR stack, images2 [B,...] through the reference stack"""
        if hasattr(self.net_extractor, 'forward_stacked'):
            return self.net_extractor.forward_stacked(image1, images2)
        f = self.net_extractor(image1, images2)
        return f['dense_features1'], f['dense_features2']

    def _match_probe_stats(self, cfg, sampling=None):
        """val.match_probe: the extractor + top-1 matcher pair against a known answer on the fed batch -> [B, 2 + T] float64 ON THE
        DEVICE (hip.match_stats: count, sum of end-point errors, hits per threshold); nothing is read back.
        A view V = warp(source, S) is made of every image (clamped to [0, 1]): source the GT, or with source: lq_up match_img_in,
        the bicubic-upsampled LQ; S from ``sampling`` (one 3 x 3 sampling matrix or B of them) or, without it, the corner
        homography of (seed, image index) (views.indexed_corner_homographies: checkpoints are compared on the same views).  The
        extractor's LR stack runs on match_img_in, its reference stack on V, the matcher on both, and the indices are scored
        against views.to_feature_coords(S) with the batch's un-padded sizes (padding / original_size) bounding the valid maps.
        The passes do not read the fp16-range flag: match_probe() reads it and repeats the probe on the range-free kernels,
        validation reads it once behind its loop and reports NaN (_probe_out_of_range)."""
        from .. import hip
        src = self.match_img_in if cfg['source'] == 'lq_up' else (self.gt if self._gt_fed else None)
        if src is None:
            raise ValueError('val.match_probe.source: gt, but the fed batch has no img_in (use source: lq_up)')
        b, _, h, w = src.shape
        if tuple(self.match_img_in.shape[2:]) != (h, w):
            raise ValueError(f'val.match_probe: the source is {h} x {w}, match_img_in {tuple(self.match_img_in.shape[2:])}')
        if sampling is None:
            sampling = torch.stack([views.indexed_corner_homographies(cfg['seed'], self._view_base + i, 1, h, w, cfg['perturb'],
                                                                      cfg['window'])[0] for i in range(b)])
        sampling = torch.as_tensor(sampling, dtype=torch.float64).expand(b, 3, 3)
        to_ref = views.to_feature_coords(sampling)
        for vh, vw in self.valid_sizes or []:
            if vh // 4 < 3 or vw // 4 < 3:
                raise ValueError(f'val.match_probe: the un-padded image of {vh} x {vw} has no 3 x 3 patch of conv3_1 cells '
                                 '(at least 12 x 12 pixels needed)')
        hip.amax_pool_reset()
        with torch.no_grad():
            view = hip.warp_perspective(src.contiguous(), sampling, interp=cfg['interp'], clamp=True)
            f1, f2 = self._extract_pair(self.match_img_in, view)
            idx = self.net_map.match(f1, f2)[0].contiguous()
            if self.valid_sizes is None:
                return hip.match_stats(idx, to_ref, cfg['thresholds'], cfg['margin'])
            # (a padded batch: each image against its own valid rectangle, in conv3_1 cells)
            return torch.cat([hip.match_stats(idx[i:i + 1], to_ref[i:i + 1], cfg['thresholds'], cfg['margin'], (vh // 4, vw // 4))
                              for i, (vh, vw) in enumerate(self.valid_sizes)])

    def match_probe(self, sampling=None):
        """one probe on the fed batch with the val.match_probe configuration (its defaults without the option) -> {count, match_epe,
        match_pck<t> per threshold}: the number of counted queries, their mean end-point error in feature pixels and the fraction of
        them within each threshold.  ``sampling``: explicit sampling matrices instead of the seeded ones (_match_probe_stats)"""
        cfg = self.match_probe_cfg if self.match_probe_cfg is not None else views.parse_match_probe({'match_probe': True})
        stats = self._match_probe_stats(cfg, sampling)
        again = self._rerun_range_free('match_probe', lambda: self._match_probe_stats(cfg, sampling), reset_scales=False)
        stats = stats if again is None else again
        return views.probe_numbers(stats.sum(0).cpu().tolist(), cfg['thresholds'])

    def _probe_out_of_range(self, probe):
        """behind validation's loop: the one read of the fp16-range flag for all of the probe's passes.  Set (by a probe, or by one
        that the next image's test() then took for its own and answered with a re-run): some probe ran on features outside the range
        of the split kernels, the pooled numbers are not to be trusted and become NaN; said so in the log.  Nothing is re-run."""
        from .. import hip
        if not hip.conv_range_tripped():
            return probe
        logging.getLogger('basicsr').warning(
            'val.match_probe: an activation of the extractor left the fp16 range of the split kernels during a probe; the probe is '
            'not re-run inside validation, its numbers are reported as NaN (model.match_probe() on the batch repeats it range-free)')
        return {k: (v if k == 'count' else float('nan')) for k, v in probe.items()}

    def _test(self):
        self.net_g.eval()
        with torch.no_grad():
            self.output = self._test_pass()
        if self.net_g is not self.net_g_ema:   # (net_g_ema stays in eval mode)
            self.net_g.train()

    def _test_pass(self, eager=False):
        """one inference pass on the fed tensors -> the output; ``eager``: the hipGraph replay is not taken whatever the options say"""
        from .. import hip
        hip.verify_packed(self.device)   # packed weight copies still match their parameters? (one launch, read with the range flag)
        out = self._forward_graphed() if (not eager and self._use_graph() and not self._pool_batch('val.hip_graph')
                                          and not self._masked_batch('val.hip_graph')) else self._forward()
        tripped = self._range_tripped('test')
        if hip.packed_stale():   # a parameter was edited through .data: drop every packed copy and repeat the pass
            logging.getLogger('basicsr').warning('test: a parameter changed without a version bump (.data write?); packed weights rebuilt')
            hip.invalidate_packed()
            out = self._forward()
            tripped = self._range_tripped('test')
        if tripped:
            out = self._rerun_range_free('test', self._forward, reset_scales=False, tripped=True)
        return out

    # ------------------------------------------------------------------ val.self_ensemble: the x8 geometric self-ensemble of test()
    @staticmethod
    def check_self_ensemble(val_opt):
        """opt['val']['self_ensemble']: absent, None or False -> False, True -> True; anything else (ints and strings too) is a
        ValueError: the ensemble has eight members, there is no other size to ask for"""
        v = (val_opt or {}).get('self_ensemble')
        if v is None or v is False:
            return False
        if v is True:
            return True
        raise ValueError(f'val.self_ensemble: {v!r} is not true or false (true: test() averages the eight flipped / transposed copies)')

    _FED = ('img_in_lq', 'match_img_in', 'img_ref_stack', 'img_ref_list', 'img_ref', 'ref_valid_bits')
    _self_ensemble_logged = _self_ensemble_eager_logged = False

    def _test_self_ensemble(self):
        """test() under val.self_ensemble (the "+" protocol of EDSR): copy j in 0..3 of group tr in (0, 1) is the input flipped
        along W if j & 1, along H if j & 2, then transposed if tr (data/multi_ref_dataset.py: augment).  Each group is ONE
        ordinary pass of batch 4 B -- images in the order j B + b, the reference stack [K][4][B], the ref_valid words repeated --
        on tensors written by hip.dihedral_expand; hip.dihedral_merge undoes the transforms and averages the eight outputs in a
        fixed order.  Two passes also for square inputs; both eager (the groups differ in shape, the graph cache keeps one).
        Afterwards the fed tensors are back in place and max_idx holds the rows of the identity copy."""
        from .. import hip
        if not MultiRefRestorationModel._self_ensemble_logged:
            MultiRefRestorationModel._self_ensemble_logged = True
            logging.getLogger('basicsr').info('val.self_ensemble: test() runs the x8 geometric self-ensemble (two passes of four '
                                              'copies per sample)')
        if self._use_graph() and not MultiRefRestorationModel._self_ensemble_eager_logged:
            MultiRefRestorationModel._self_ensemble_eager_logged = True
            logging.getLogger('basicsr').info('val.hip_graph: the passes of val.self_ensemble run eagerly (no hipGraph capture or replay)')
        pool = self.ref_pool
        if pool is not None:   # a matching pre-pass over the pool, once, on the untransformed batch: the ensemble runs on its choice
            hip.amax_pool_reset()
            self._select_from_pool()
            self._rerun_range_free('test', self._select_from_pool, reset_scales=False)   # (the extractor left the fp16 range: choose again)
        fed = {n: self.__dict__[n] for n in self._FED if n in self.__dict__}
        k, b = self.num_refs, self.img_in_lq.shape[0]
        outs, max_idx = [], None
        self.net_g.eval()
        try:
            self.ref_pool = None
            with torch.no_grad():
                for tr in (0, 1):
                    self.img_in_lq = hip.dihedral_expand(fed['img_in_lq'].contiguous(), tr)
                    self.match_img_in = hip.dihedral_expand(fed['match_img_in'].contiguous(), tr)
                    self.img_ref_stack = hip.dihedral_expand(fed['img_ref_stack'].contiguous(), tr, outer=k)
                    self.img_ref_list = list(self.img_ref_stack.view(k, 4 * b, *self.img_ref_stack.shape[1:]).unbind(0))
                    if 'img_ref' in fed:
                        self.img_ref = self.img_ref_stack
                    if fed.get('ref_valid_bits') is not None:
                        self.ref_valid_bits = fed['ref_valid_bits'].repeat(4)
                    outs.append(self._test_pass(eager=True).contiguous())
                    if tr == 0:
                        max_idx = self.max_idx
                self.output = hip.dihedral_merge(*outs)
                self.max_idx = max_idx.view(k, 4, b, *max_idx.shape[1:])[:, 0].reshape(k * b, *max_idx.shape[1:])
        finally:
            for n, t in fed.items():
                setattr(self, n, t)
            self.ref_pool = pool
            if self.net_g is not self.net_g_ema:
                self.net_g.train()

    # ------------------------------------------------------------------ hipGraph replay of the inference pass
    _INPUTS = ('img_in_lq', 'match_img_in', 'img_ref_stack')

    def _use_graph(self):
        """opt['val']['hip_graph'] or MREFSR_GRAPH=1: the whole inference pass (240 launches) is captured once per
        input shape and parameter version into a hipGraph and replayed, taking ~50 us of host work per launch off
        the critical path.  Off by default: measured on MI355X it changes nothing, neither at the benchmark shape
        (GPU-bound) nor at LR 40x40 (12.5 ms per sample either way: there each convolution launch is bound by the
        serial K loop of a single block, ~60 us for a 256-channel layer, not by the host) -- it only helps when
        the host is the slower side."""
        return bool((self.opt.get('val') or {}).get('hip_graph')) or os.environ.get('MREFSR_GRAPH', '0') == '1'

    def _graph_key(self):
        from ..archs import nhwc
        from .. import hip
        versions = tuple((p._version, p.data_ptr()) for net in (self.net_g, self.net_extractor, self.net_map) for p in net.parameters())
        shapes = tuple(tuple(getattr(self, n).shape) for n in self._INPUTS)
        return shapes, self.num_refs, nhwc.TERMS, nhwc.BF16, hip.packed_epoch(), hash(versions)

    def _forward_graphed(self):
        key = self._graph_key()
        cache = self.__dict__.setdefault('_graphs', {})
        entry = cache.get(key)
        if entry is None:
            cache.clear()                              # one shape / parameter version at a time: graphs pin their buffers
            from .. import hip
            hip.release_capture_workspaces()
            static = {n: getattr(self, n).clone() for n in self._INPUTS}
            for n, t in static.items():
                setattr(self, n, t)
            dyn = [m for m in self.net_g.modules() if hasattr(m, '_offset_count')]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):              # eager warm-up: weight packing, workspaces, lazy kernel attributes
                self._forward()
            torch.cuda.current_stream().wait_stream(side)
            before = [m._offset_count for m in dyn]
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self._forward()
            counts = [m._offset_count - b for m, b in zip(dyn, before)]
            entry = cache[key] = (graph, static, out, self.max_idx, dyn, counts)
            graph.replay()                             # (capture does not execute)
        else:
            graph, static, out, max_idx, dyn, counts = entry
            for n in self._INPUTS:
                static[n].copy_(getattr(self, n))
            graph.replay()
            for m, c in zip(dyn, counts):
                m._offset_count += c
        self.max_idx = entry[3].clone()
        return entry[2].clone()

    def check_numeric_range(self):
        """test() and optimize_parameters() already handle the fp16-split range flag themselves (re-run on the range-free
        kernels, counted in ``range_fallbacks``); this raises FloatingPointError if the flag is (still) set, for callers
        that launch parts of the path directly"""
        from .. import hip
        hip.check_conv_range()

    # ------------------------------------------------------------------ validation (ref :310-386)
    def validation(self, dataloader, current_iter, tb_logger, save_img=False):
        if self.opt.get('dist', False):
            return self.dist_validation(dataloader, current_iter, tb_logger, save_img)
        return self.nondist_validation(dataloader, current_iter, tb_logger, save_img)

    def dist_validation(self, dataloader, current_iter, tb_logger, save_img):
        if self.opt.get('rank', 0) == 0:  # rank 0 only, like the reference (:312-314)
            return self.nondist_validation(dataloader, current_iter, tb_logger, save_img)

    def _metrics_on_device(self):
        """opt['val']['metrics_on_device'] (off by default): validation's PSNR, PSNR-Y and SSIM-Y on the HIP kernels of
        csrc/metrics.hip (metrics.validation_metrics) instead of numpy on the host; the same numbers, logs and return value"""
        return bool((self.opt.get('val') or {}).get('metrics_on_device'))

    def nondist_validation(self, dataloader, current_iter, tb_logger, save_img):
        """validation never synthesises its input (realesrgan_model.py:187-191): the flag is put back behind it"""
        synthesise, self._synthesise = self._synthesise, False
        self._validating, self._view_index = True, 0   # (train.ref_augment is left out likewise; the views count images from 0)
        try:
            return self._nondist_validation(dataloader, current_iter, tb_logger, save_img)
        finally:
            self._synthesise = synthesise
            self._validating, self._view_index = False, 0

    def _nondist_validation(self, dataloader, current_iter, tb_logger, save_img):
        """per image: feed_data -> test -> uint8 image -> crop the dataset's zero padding -> [PNG] -> PSNR (RGB), PSNR (Y),
        SSIM (Y) with crop_border from the options (ref :324-386); with val.match_probe also the matcher's score on a known view of
        every image (_match_probe_stats; logged, sent to tb_logger and returned as match_epe / match_pck<t>); with val.msssim also five-level MS-SSIM (Y)
        (metrics.calculate_msssim; logged as MS-SSIM_Y, tb scalar and result key msssim_y).  save_img writes
        path.visualization/<img>/<img>_<iter>.png while training, path.visualization/<dataset>/<img>_<name>[_suffix].png when testing.
        With val.metrics_on_device the metrics run on the GPU and only their scalars (and, for save_img, the image) come back; an
        image with non-finite values in its output or GT takes the numpy path."""
        from ..metrics import calculate_msssim, calculate_psnr, calculate_ssim, imwrite, tensor2img, validation_metrics
        logger = logging.getLogger('basicsr')
        dataset_name = getattr(getattr(dataloader, 'dataset', None), 'opt', {}).get('name', 'val')
        on_device = self._metrics_on_device()
        want_msssim = bool((self.opt.get('val') or {}).get('msssim'))
        psnrs, psnrs_y, ssims_y, msssims_y = [], [], [], []
        probe_acc = None   # val.match_probe: the summed statistics, on the device until the loop is over
        for idx, val_data in enumerate(dataloader):
            lq_path = val_data.get('lq_path', [f'{idx:04d}'])
            img_name = os.path.splitext(os.path.basename(lq_path[0] if isinstance(lq_path, (list, tuple)) else lq_path))[0]
            self.feed_data(val_data)
            self.test()
            if self.match_probe_cfg is not None:
                stats = self._match_probe_stats(self.match_probe_cfg).sum(0)
                probe_acc = stats if probe_acc is None else probe_acc + stats
            cb = self.opt['crop_border']
            size = None
            if 'padding' in val_data and val_data['padding']:
                size = [int(v) for v in val_data['original_size']][:2]
            dev = None
            if on_device:
                dev = validation_metrics(self.output[:1], self.gt[:1], cb, sizes=None if size is None else [size], return_img=save_img,
                                         **(dict(msssim=True) if want_msssim else {}))
                dev = dev if dev['finite'][0] else None
            if dev is not None:
                sr_img = None
                if save_img:
                    img = dev['img'][0]
                    sr_img = (img if size is None else img[:size[0], :size[1]]).cpu().numpy()
                psnr, psnr_y, ssim_y = dev['psnr'][0], dev['psnr_y'][0], dev['ssim_y'][0]
                if want_msssim:
                    msssims_y.append(dev['msssim_y'][0])
            else:
                sr_img = tensor2img(self.output[:1])
                gt_img = tensor2img(self.gt[:1])
                if size is not None:
                    oh, ow = size
                    sr_img, gt_img = sr_img[:oh, :ow], gt_img[:oh, :ow]
                psnr = calculate_psnr(sr_img, gt_img, crop_border=cb)
                psnr_y = calculate_psnr(sr_img, gt_img, crop_border=cb, test_y_channel=True)
                ssim_y = calculate_ssim(sr_img, gt_img, crop_border=cb, test_y_channel=True)
                if want_msssim:
                    msssims_y.append(calculate_msssim(sr_img, gt_img, crop_border=cb, test_y_channel=True))
            if save_img:
                vis = self.opt['path']['visualization']
                if self.opt['is_train']:
                    save_path = os.path.join(vis, img_name, f'{img_name}_{current_iter}.png')
                else:
                    suffix = f"_{self.opt['suffix']}" if self.opt.get('suffix') else ''
                    save_path = os.path.join(vis, dataset_name, f"{img_name}_{self.opt['name']}{suffix}.png")
                imwrite(sr_img, save_path)
            psnrs.append(psnr)
            psnrs_y.append(psnr_y)
            ssims_y.append(ssim_y)
            if not self.is_train:
                ms = f' # MS-SSIM_Y: {msssims_y[-1]:.4e}' if want_msssim else ''
                logger.info(f'# img {img_name} # PSNR: {psnrs[-1]:.4e} # PSNR_Y: {psnrs_y[-1]:.4e} # SSIM_Y: {ssims_y[-1]:.4e}{ms}.')
        n = max(len(psnrs), 1)
        avg_psnr, avg_psnr_y, avg_ssim_y = sum(psnrs) / n, sum(psnrs_y) / n, sum(ssims_y) / n
        avg_msssim_y = sum(msssims_y) / n
        ms = f' # MS-SSIM_Y: {avg_msssim_y:.4e}' if want_msssim else ''
        logger.info(f'# Validation {dataset_name} # PSNR: {avg_psnr:.4e} # PSNR_Y: {avg_psnr_y:.4e} # SSIM_Y: {avg_ssim_y:.4e}{ms}.')
        if tb_logger:
            tb_logger.add_scalar('psnr', avg_psnr, current_iter)
            tb_logger.add_scalar('psnr_y', avg_psnr_y, current_iter)
            tb_logger.add_scalar('ssim_y', avg_ssim_y, current_iter)
            if want_msssim:
                tb_logger.add_scalar('msssim_y', avg_msssim_y, current_iter)
        result = dict(psnr=avg_psnr, psnr_y=avg_psnr_y, ssim_y=avg_ssim_y)
        if want_msssim:
            result['msssim_y'] = avg_msssim_y
        if probe_acc is not None:   # the one readback of the probe
            probe = self._probe_out_of_range(views.probe_numbers(probe_acc.cpu().tolist(), self.match_probe_cfg['thresholds']))
            count = probe.pop('count')
            logger.info(f'# Validation {dataset_name} # match probe over {count} queries # '
                        + ' # '.join(f'{k}: {v:.4e}' for k, v in probe.items()) + '.')
            if tb_logger:
                for k, v in probe.items():
                    tb_logger.add_scalar(k, v, current_iter)
            result.update(probe)
        return result

    def save(self, epoch, current_iter):
        """net_g (and net_d) checkpoints as {'params': state_dict} under path.models (ref :304-308, base_model.py:198-226)"""
        models_dir = self.opt.get('path', {}).get('models')
        if models_dir and self.opt.get('rank', 0) == 0:
            name = 'latest' if current_iter == -1 else current_iter
            if self.net_g_ema is not None:   # sr_model.py:227-228: both sets in one file
                self.save_network([self.net_g, self.net_g_ema], os.path.join(models_dir, f'net_g_{name}.pth'), param_key=['params', 'params_ema'])
            else:
                self.save_network(self.net_g, os.path.join(models_dir, f'net_g_{name}.pth'))
            if getattr(self, 'net_d', None) is not None:
                self.save_network(self.net_d, os.path.join(models_dir, f'net_d_{name}.pth'))

    def save_training_state(self, epoch, current_iter):
        """optimizer / scheduler states as {epoch, iter, optimizers, schedulers} in
        path.training_states/<iter>.state (base_model.py:309-338); rank 0 only"""
        states_dir = self.opt.get('path', {}).get('training_states')
        if current_iter == -1 or not states_dir or self.opt.get('rank', 0) != 0:
            return
        state = {'epoch': epoch, 'iter': current_iter, 'optimizers': [o.state_dict() for o in self.optimizers],
                 'schedulers': [s.state_dict() for s in self.schedulers]}
        if self.d_adaptive is not None:   # train.d_augment.adaptive: p and the pending accumulator
            state['d_augment'] = self.d_adaptive.state_dict()
        os.makedirs(states_dir, exist_ok=True)
        torch.save(state, os.path.join(states_dir, f'{current_iter}.state'))

    def resume_training(self, resume_state):
        """reload optimizers and schedulers from a save_training_state dict (base_model.py:343-356)"""
        resume_optimizers, resume_schedulers = resume_state['optimizers'], resume_state['schedulers']
        assert len(resume_optimizers) == len(self.optimizers), 'Wrong lengths of optimizers'
        assert len(resume_schedulers) == len(self.schedulers), 'Wrong lengths of schedulers'
        for o, state in zip(self.optimizers, resume_optimizers):
            o.load_state_dict(state)
        for sch, state in zip(self.schedulers, resume_schedulers):
            sch.load_state_dict(state)
        if self.d_adaptive is not None and resume_state.get('d_augment') is not None:   # (a state without it: the option's p)
            self.d_adaptive.load_state_dict(resume_state['d_augment'], device=self.device)

    # ------------------------------------------------------------------ bookkeeping
    def get_current_log(self):
        log = OrderedDict((k, v.item() if torch.is_tensor(v) else v) for k, v in self.log_dict.items())
        for which in ('g', 'd'):   # (HipAdam.state_dict() moves the device's count of skipped steps into its host counters)
            if f'skipped_steps_{which}' in log:
                log[f'skipped_steps_{which}'] += getattr(getattr(self, f'optimizer_{which}'), 'skipped_folded', 0)
        return log

    def get_current_visuals(self):
        out = OrderedDict(img_in_lq=self.img_in_lq.detach().cpu(), rlt=self.output.detach().cpu())
        if hasattr(self, 'gt'):
            out['gt'] = self.gt.detach().cpu()
        return out

    def offset_guards(self):
        """mean |learned offset| of the three DynAgg since the last call (ref :70-73 warning)."""
        dar = self.get_bare_model(self.net_g).dyn_agg_restore
        return {n: getattr(dar, n).offset_guard() for n in ('small_dyn_agg', 'medium_dyn_agg', 'large_dyn_agg')}

    def update_learning_rate(self, current_iter, warmup_iter=-1):
        if current_iter > 1:
            for scheduler in self.schedulers:
                scheduler.step()
        if current_iter < warmup_iter:
            for optimizer, scheduler in zip(self.optimizers, self.schedulers):
                for group in optimizer.param_groups:
                    group['lr'] = group['initial_lr'] / warmup_iter * current_iter

    def get_current_learning_rate(self):
        return [param_group['lr'] for param_group in self.optimizers[0].param_groups]

    def save_network(self, net, path, param_key='params'):
        """one network under one key, or lists of both (base_model.py:198-226)"""
        nets, keys = (net, param_key) if isinstance(net, list) else ([net], [param_key])
        assert len(nets) == len(keys), 'The lengths of net and param_key should be the same.'
        save = {key: OrderedDict((k[7:] if k.startswith('module.') else k, v.cpu()) for k, v in self.get_bare_model(n).state_dict().items())
                for n, key in zip(nets, keys)}
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(save, path)

    def load_network(self, net, load_path, strict=True, param_key='params'):
        """base_model.py:280-306: the state dict under ``param_key`` of the file; a file without that key but with 'params' gives
        those (a checkpoint written without an EMA, asked for 'params_ema').  A file with neither is taken as a flat state dict."""
        logger = logging.getLogger('basicsr')
        load_net = torch.load(load_path, map_location='cpu')
        if param_key is not None:
            if param_key not in load_net and 'params' in load_net:
                param_key = 'params'
                logger.info('Loading: params_ema does not exist, use params.')
            if param_key in load_net:
                load_net = load_net[param_key]
                logger.info(f'Loading {self.get_bare_model(net).__class__.__name__} model from {load_path}, with param key: [{param_key}].')
        load_net = OrderedDict((k[7:] if k.startswith('module.') else k, v) for k, v in load_net.items())
        self.get_bare_model(net).load_state_dict(load_net, strict=strict)


@MODEL_REGISTRY.register()
class RefRestorationModel(MultiRefRestorationModel):
    """Single-reference twin (basicsr/models/ref_restoration_model.py:20-375): `network_g` = RestorationNet,
    `network_extractor` = ContrasExtractorSep, data dict with one `img_ref` (B,3,4h,4w) (:190-194).  Same
    optimizer groups, schedulers, losses, validation and checkpoint layout as the multi-reference model."""
    _INPUTS = ('img_in_lq', 'match_img_in', 'img_ref')
    _REF_POOLS = False   # (the ref_select option is refused at construction)

    def feed_data(self, data):
        self.valid_sizes = self._valid_sizes_of(data)
        self._gt_fed = 'img_in' in data   # (self.gt may be an earlier batch's)
        self.img_in_lq = data['img_in_lq'].to(self.device, non_blocking=True)
        self.img_ref = self._ref_views(data['img_ref'].to(self.device, non_blocking=True), 1)
        self.num_refs = 1
        self.img_ref_stack = self.img_ref
        self.img_ref_list = [self.img_ref]
        if 'img_in' in data:
            self.gt = data['img_in'].to(self.device, non_blocking=True)
        self.match_img_in = data['img_in_up'].to(self.device, non_blocking=True)

    def _forward(self):
        with torch.no_grad():   # frozen feature networks (:197-199, :278-280)
            features = self.net_extractor(self.match_img_in, self.img_ref)
            pre_offset, img_ref_feat = self._match(features['dense_features1'], features['dense_features2'], self.img_ref)
        return self._run_net_g(self.img_in_lq, pre_offset, img_ref_feat)
