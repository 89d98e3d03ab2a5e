#!/usr/bin/env python3
"""Generate tests/golden/e2e_c2_percep.npz: the reference's own MultiRefRestorationModel.optimize_parameters(1) at BASELINE
configs[2]'s per-GPU shape (B = 4, K = 5, LR 40 x 40 -> GT 160 x 160) with a perceptual and a style loss next to the L1 pixel
loss (basicsr/models/multi_ref_restoration_model.py:114-165, 237-279; basicsr/models/losses.py:141-238).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_percep.py
The three nets are built and loaded exactly as gen_golden._build_model does (synthetic weights, the inputs of e2e_c2); both
perceptual VGG19 stacks take synth.state_dict(spec) weights, and their spec is stored so that the GPU test rebuilds them
without the reference.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import synth  # noqa: E402

R = G.R
LAYERS = {'conv1_2': 0.1, 'conv2_2': 0.1, 'conv3_4': 1.0, 'conv4_4': 1.0, 'conv5_4': 1.0}
PERCEPTUAL_OPT = dict(layer_weights=LAYERS, vgg_type='vgg19', use_input_norm=True, perceptual_weight=1.0, style_weight=0.0,
                      norm_img=True, criterion='l1')
STYLE_OPT = dict(layer_weights=LAYERS, vgg_type='vgg19', use_input_norm=True, perceptual_weight=0.0, style_weight=100.0,
                 norm_img=True, criterion='l1')


def _full_vgg19(pretrained=False, **kw):
    """torchvision.models.vgg19's layer stack (the stub of _refimport builds only the first three stages, the perceptual loss
    slices up to conv5_4); the weights are replaced by synth.state_dict below"""
    from torch import nn
    layers, cin = [], 3
    for v in R._VGG_CFG['vgg19']:
        if v == 'M':
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    net = nn.Module()
    net.features = nn.Sequential(*layers)
    return net


def main():
    R.install()
    sys.modules['torchvision.models.vgg'].vgg19 = _full_vgg19
    mm = R.ref_module('basicsr.models.multi_ref_restoration_model')
    init = mm.MultiRefRestorationModel.__init__

    def with_losses(self, opt):
        opt['train'].update(perceptual_opt=PERCEPTUAL_OPT, style_opt=STYLE_OPT)
        init(self, opt)
    mm.MultiRefRestorationModel.__init__ = with_losses
    torch.set_grad_enabled(True)
    try:
        model, specs, data = G._build_model(True, 4, 5, 40, 40, 'e2e_c2')
    finally:
        mm.MultiRefRestorationModel.__init__ = init
    vgg_spec = G.spec_of(model.cri_perceptual)
    assert vgg_spec == G.spec_of(model.cri_style)
    sd = synth.state_dict(vgg_spec)
    for cri in (model.cri_perceptual, model.cri_style):
        cri.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    # range check: the largest activation of the synthetic VGG on these images, against the fp16 range of the split kernels
    with torch.no_grad():
        feats = model.cri_perceptual.vgg((data['img_in'] + 1.0) * 0.5)
        tap_max = {k: float(v.abs().max()) for k, v in feats.items()}
        x = (data['img_in'] + 1.0) * 0.5
        x = (x - model.cri_perceptual.vgg.mean) / model.cri_perceptual.vgg.std
        act_max = 0.0
        for layer in model.cri_perceptual.vgg.vgg_net:
            x = layer(x)
            act_max = max(act_max, float(x.abs().max()))
    print('tap max |x|:', tap_max, 'largest activation:', act_max)
    assert act_max < 1000.0, act_max
    model.feed_data(data)
    model.optimize_parameters(1)
    logs = {k: float(model.log_dict[k]) for k in ('l_g_pix', 'l_g_percep', 'l_g_style')}
    print('losses:', logs)
    names, gsum, gabs, psum = [], [], [], []
    for n, p in model.net_g.named_parameters():
        names.append(n)
        g = p.grad.detach().double() if p.grad is not None else torch.zeros(1, dtype=torch.float64)
        gsum.append(float(g.sum()))
        gabs.append(float(g.abs().sum()))
        psum.append(float(p.detach().double().sum()))
    groups = [[float(g['lr']), len(g['params'])] for g in model.optimizer_g.param_groups]
    torch.set_grad_enabled(False)
    arrays = dict(b=np.array(4), k=np.array(5), lr_hw=np.array([40, 40]), key=np.array('e2e_c2'),
                  chk=np.array(synth.checksum(*[data[n].numpy() for n in ('img_in_lq', 'img_in_up', 'img_ref_list', 'img_in')])),
                  loss=np.array(logs['l_g_pix']), l_g_pix=np.array(logs['l_g_pix']), l_g_percep=np.array(logs['l_g_percep']),
                  l_g_style=np.array(logs['l_g_style']), param_names=np.array(names), grad_sum=np.array(gsum), grad_abs=np.array(gabs),
                  param_sum_after=np.array(psum), opt_groups=np.array(groups),
                  layer_names=np.array(list(LAYERS)), layer_weights=np.array(list(LAYERS.values())),
                  perceptual_weight=np.array(PERCEPTUAL_OPT['perceptual_weight']), style_weight=np.array(STYLE_OPT['style_weight']),
                  vgg_act_max=np.array(act_max))
    for nm, spec in list(specs.items()) + [('vgg', vgg_spec)]:
        sa = G.spec_arrays(spec)
        arrays[f'{nm}_spec_keys'], arrays[f'{nm}_spec_shapes'] = sa['spec_keys'], sa['spec_shapes']
    G.save('e2e_c2_percep', **arrays)


if __name__ == '__main__':
    main()
