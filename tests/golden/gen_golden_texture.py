#!/usr/bin/env python3
"""Generate tests/golden/texture.npz: the reference's own TextureLoss(use_weights=True).forward(x, maps, weights)
(basicsr/models/losses.py:430-532) in fp64 on the CPU, for B = 2 and a 48 x 32 image (relu3_1 map 12 x 8, match grid 10 x 6).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_texture.py
The VGG19 stack takes synth.state_dict(spec) weights, and the spec is stored so that the GPU test rebuilds them without the
reference.  maps = vgg(y) of a second stored image, so that the file holds two small images instead of three feature maps; the
images are multiples of 1/255 (exact in fp32, one byte each in the file).  Stored in fp64: the loss, the three per-layer terms
(each from a one-layer TextureLoss: its value times 3 / loss_weight) and d loss / d x.
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
LAYERS = ('relu1_1', 'relu2_1', 'relu3_1')
LOSS_WEIGHT = 1.0
B, H, W = 2, 48, 32


def _loss(ml, layers):
    cri = ml.TextureLoss(use_weights=True, loss_weight=LOSS_WEIGHT, layer_weights={k: 1.0 for k in layers})
    spec = G.spec_of(cri)
    cri.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(spec).items()}, strict=True)
    return cri.double(), spec


def main():
    R.install()
    ml = R.ref_module('basicsr.models.losses')
    x8 = np.stack([np.round(synth.image(f'texture/x{b}', 3, H, W) * 255.0) for b in range(B)]).astype(np.uint8)
    y8 = np.stack([np.round(synth.image(f'texture/y{b}', 3, H, W) * 255.0) for b in range(B)]).astype(np.uint8)
    weights = (synth.rand('texture/weights', (B, 1, H // 4 - 2, W // 4 - 2)) * 3.0).astype(np.float32)
    x = torch.from_numpy(x8.astype(np.float64) / 255.0)
    y = torch.from_numpy(y8.astype(np.float64) / 255.0)
    wt = torch.from_numpy(weights).double()
    torch.set_grad_enabled(True)
    cri, spec = _loss(ml, LAYERS)
    with torch.no_grad():
        maps = cri.vgg(y)
        act_max = max(float(v.abs().max()) for v in maps.values())
    assert act_max < 1000.0, act_max     # (far inside the fp16 range of the engine's split convolution kernels)
    xg = x.clone().requires_grad_(True)
    loss = cri(xg, {k: v.clone() for k, v in maps.items()}, wt)   # (the reference multiplies the maps it is given in place)
    loss.backward()
    terms = []
    for name in LAYERS:
        one, _ = _loss(ml, (name,))
        with torch.no_grad():
            terms.append(float(one(x, {name: maps[name].clone()}, wt)) * 3.0 / LOSS_WEIGHT)
    torch.set_grad_enabled(False)
    print('loss', float(loss), 'terms', terms, 'sum / 3', sum(terms) / 3.0 * LOSS_WEIGHT, '|grad| max', float(xg.grad.abs().max()))
    assert abs(sum(terms) / 3.0 * LOSS_WEIGHT - float(loss)) <= 1e-12 * abs(float(loss))
    sa = G.spec_arrays(spec)
    G.save('texture', x=x8, y=y8, weights=weights, loss=np.array(float(loss)), terms=np.array(terms), grad=xg.grad.numpy(),
           layer_names=np.array(LAYERS), loss_weight=np.array(LOSS_WEIGHT), vgg_act_max=np.array(act_max),
           vgg_spec_keys=sa['spec_keys'], vgg_spec_shapes=sa['spec_shapes'])


if __name__ == '__main__':
    main()
