"""CPU: train.d_augment without a GPU -- option parsing and its refusals, the sampler, d_augment_torch against a literal transcription
of DiffAugment's operators, the adjoint identity, AdaptiveP's arithmetic and the all-reduce of its two words over gloo."""
import os
import socket

import pytest
import torch
import torch.nn.functional as F

from mrefsr_amd.archs import d_augment as da

FULL = dict(policy=['color', 'translation', 'cutout', 'flip'])


# ------------------------------------------------------------------ the option
def test_option_defaults_and_forms():
    assert da.parse_d_augment(None) is None and da.parse_d_augment(False) is None
    cfg = da.parse_d_augment(dict(FULL))
    assert cfg['ops'] == ('brightness', 'saturation', 'contrast', 'translation', 'cutout', 'flip') and cfg['p'] == 1.0
    assert (cfg['brightness'], cfg['saturation'], cfg['contrast'], cfg['translation'], cfg['cutout']) == (0.25, (0.0, 2.0), (0.5, 1.5), 0.125, 0.5)
    assert cfg['adaptive'] is None
    assert da.parse_d_augment(dict(policy='color, cutout'))['ops'] == ('brightness', 'saturation', 'contrast', 'cutout')
    assert da.parse_d_augment(dict(policy=['flip'], p=0))['p'] == 0.0
    ada = da.parse_d_augment(dict(FULL, p=0.25, adaptive={}), gan_type='hinge')['adaptive']
    assert ada == dict(target=0.6, interval=4, speed_kimg=500.0)
    for gan_type in da.ADAPTIVE_GAN_TYPES:
        assert da.parse_d_augment(dict(FULL, adaptive=dict(target=0.5, interval=2, speed_kimg=100)), gan_type=gan_type)['adaptive']['interval'] == 2


@pytest.mark.parametrize('opt,word', [
    (dict(FULL, strength=1), 'strength'),
    (dict(policy=[]), 'policy'),
    (dict(policy=''), "''"),
    (dict(p=1.0), 'policy'),
    (dict(policy=['color', 'rotate']), 'rotate'),
    (dict(FULL, p=1.5), 'd_augment.p'),
    (dict(FULL, p=-0.1), 'd_augment.p'),
    (dict(FULL, p=float('nan')), 'd_augment.p'),
    (dict(FULL, brightness=float('inf')), 'brightness'),
    (dict(FULL, saturation=[2.0, 0.0]), 'saturation'),
    (dict(FULL, saturation=[0.0, float('nan')]), 'saturation'),
    (dict(FULL, contrast=[1.5, 0.5]), 'contrast'),
    (dict(FULL, contrast=1.0), 'contrast'),
    (dict(FULL, translation=float('nan')), 'translation'),
    (dict(FULL, cutout=-0.5), 'cutout'),
    (dict(FULL, adaptive=dict(goal=1)), 'goal'),
    (dict(FULL, adaptive=dict(interval=0)), 'interval'),
    (dict(FULL, adaptive=dict(speed_kimg=0)), 'speed_kimg'),
])
def test_option_refusals_name_the_key(opt, word):
    with pytest.raises(ValueError, match=word):
        da.parse_d_augment(opt, gan_type='vanilla')


def test_option_needs_a_discriminator_and_a_zero_boundary_for_adaptive():
    with pytest.raises(ValueError, match='network_d'):
        da.parse_d_augment(dict(FULL), has_net_d=False)
    for gan_type in ('wgan', 'lsgan'):
        with pytest.raises(ValueError, match=gan_type):
            da.parse_d_augment(dict(FULL, adaptive={}), gan_type=gan_type)
        assert da.parse_d_augment(dict(FULL), gan_type=gan_type)['adaptive'] is None   # (the fixed-p form is allowed)


# ------------------------------------------------------------------ the sampler
def _gen(seed=3):
    return torch.Generator().manual_seed(seed)


def test_sampler_p0_is_identity():
    par = da.sample_d_augment(5, 37, 53, da.parse_d_augment(dict(FULL)), 0.0, _gen())
    ident = da.identity_params(5)
    assert torch.equal(par.packed, ident.packed) and not par.contrast
    assert par.fpar.tolist() == [[0.0, 1.0, 1.0, 0.0]] * 5 and par.ipar.tolist() == [[0] * 8] * 5


def test_sampler_p1_ranges_and_boxes():
    h, w, b = 37, 53, 400
    cfg = da.parse_d_augment(dict(FULL, brightness=0.2, saturation=[0.5, 1.75], contrast=[0.75, 1.25], translation=0.125, cutout=0.5))
    par = da.sample_d_augment(b, h, w, cfg, 1.0, _gen())
    db, s, c = par.fpar[:, 0], par.fpar[:, 1], par.fpar[:, 2]
    assert db.abs().max() <= 0.2 and db.min() < -0.15 and db.max() > 0.15
    assert s.min() >= 0.5 and s.max() <= 1.75 and s.max() - s.min() > 1.0
    assert c.min() >= 0.75 and c.max() <= 1.25 and c.max() - c.min() > 0.4 and par.contrast
    flip, ty, tx, y0, y1, x0, x1 = (par.ipar[:, k] for k in range(7))
    assert set(flip.tolist()) == {0, 1}
    ry, rx = round(h * 0.125), round(w * 0.125)
    assert set(ty.tolist()) == set(range(-ry, ry + 1)) and set(tx.tolist()) == set(range(-rx, rx + 1))
    ch, cw = round(h * 0.5), round(w * 0.5)
    assert bool(((0 <= y0) & (y0 < y1) & (y1 <= h) & (0 <= x0) & (x0 < x1) & (x1 <= w)).all())   # clipped, inside, never empty
    assert int((y1 - y0).max()) == ch and int((x1 - x0).max()) == cw
    assert int(y0.min()) == 0 and int(y1.max()) == h and int(x0.min()) == 0 and int(x1.max()) == w
    # a policy without an operator leaves it at its identity and the others where they were
    only = da.sample_d_augment(b, h, w, da.parse_d_augment(dict(policy='translation')), 1.0, _gen())
    assert torch.equal(only.ipar[:, 1:3], par.ipar[:, 1:3]) and not only.contrast
    assert only.fpar[:, :3].tolist() == [[0.0, 1.0, 1.0]] * b and int(only.ipar[:, 3:].abs().sum()) == 0 and int(only.ipar[:, 0].sum()) == 0


def test_cut_box_centre_range_follows_the_parity_of_the_side():
    cfg = da.parse_d_augment(dict(policy='cutout', cutout=0.5))
    even = da.sample_d_augment(600, 8, 8, cfg, 1.0, _gen()).ipar    # 4 x 4 box: centres 0 .. 8, boxes [c - 2, c + 2)
    assert set((even[:, 3] + even[:, 4]).tolist()) >= {2, 14} and int(even[:, 4].min()) == 2 and int(even[:, 3].max()) == 6
    odd = da.sample_d_augment(600, 6, 6, cfg, 1.0, _gen()).ipar     # 3 x 3 box: centres 0 .. 5, boxes [c - 1, c + 2)
    assert int(odd[:, 4].min()) == 2 and int(odd[:, 3].max()) == 4
    assert da.cut_box(8, 8, 4, 4, 8, 0) == (6, 8, 0, 2) and da.cut_box(6, 6, 3, 3, 5, 0) == (4, 6, 0, 2)


def test_sampler_is_pinned_by_the_seed_and_by_nothing_else():
    cfg = da.parse_d_augment(dict(FULL))
    a, b = da.sample_d_augment(4, 64, 64, cfg, 0.7, _gen(5)), da.sample_d_augment(4, 64, 64, cfg, 0.7, _gen(5))
    assert torch.equal(a.packed, b.packed)
    assert not torch.equal(a.packed, da.sample_d_augment(4, 64, 64, cfg, 0.7, _gen(6)).packed)
    more = da.sample_d_augment(7, 64, 64, cfg, 0.7, _gen(5))     # row i is sample i: a larger batch leaves the earlier samples alone
    assert torch.equal(more.fpar[:4], a.fpar) and torch.equal(more.ipar[:4], a.ipar)
    g = _gen(5)
    first, second = da.sample_d_augment(4, 64, 64, cfg, 0.7, g), da.sample_d_augment(4, 64, 64, cfg, 0.7, g)
    assert torch.equal(first.packed, a.packed) and not torch.equal(second.packed, a.packed)   # every call draws anew


# ------------------------------------------------------------------ d_augment_torch against DiffAugment's operators
def _diffaugment(x, db, s, c, flip, t_y, t_x, ch, cw, off_y, off_x):
    """DiffAugment_pytorch.py transcribed with the random draws as arguments (per-sample tensors): the three colour lines,
    torch.flip, the pad-and-gather translation (its translation_x is the first spatial axis) and the mask-multiply cutout"""
    b, _, h, w = x.shape
    x = x + db.view(b, 1, 1, 1)                                               # rand_brightness
    x_mean = x.mean(dim=1, keepdim=True)                                      # rand_saturation
    x = (x - x_mean) * s.view(b, 1, 1, 1) + x_mean
    x_mean = x.mean(dim=[1, 2, 3], keepdim=True)                              # rand_contrast
    x = (x - x_mean) * c.view(b, 1, 1, 1) + x_mean
    x = torch.where(flip.view(b, 1, 1, 1) != 0, torch.flip(x, [3]), x)
    grid_batch, grid_x, grid_y = torch.meshgrid(torch.arange(b), torch.arange(h), torch.arange(w), indexing='ij')   # rand_translation
    grid_x = torch.clamp(grid_x + t_y.view(b, 1, 1) + 1, 0, h + 1)
    grid_y = torch.clamp(grid_y + t_x.view(b, 1, 1) + 1, 0, w + 1)
    x_pad = F.pad(x, [1, 1, 1, 1, 0, 0, 0, 0])
    x = x_pad.permute(0, 2, 3, 1).contiguous()[grid_batch, grid_x, grid_y].permute(0, 3, 1, 2)
    grid_batch, grid_x, grid_y = torch.meshgrid(torch.arange(b), torch.arange(ch), torch.arange(cw), indexing='ij')   # rand_cutout
    grid_x = torch.clamp(grid_x + off_y.view(b, 1, 1) - ch // 2, min=0, max=h - 1)
    grid_y = torch.clamp(grid_y + off_x.view(b, 1, 1) - cw // 2, min=0, max=w - 1)
    mask = torch.ones(b, h, w, dtype=x.dtype)
    mask[grid_batch, grid_x, grid_y] = 0
    return x * mask.unsqueeze(1)


def _drawn(b, h, w, seed):
    """DiffAugment's draws at its defaults (brightness halved: images in [0, 1]) and the tables they mean here: the transcription
    shifts by +t (out[y] = in[y + t]), the tables hold ty = -t"""
    g = torch.Generator().manual_seed(seed)
    db = (torch.rand(b, generator=g, dtype=torch.float64) - 0.5) * 0.5
    s = torch.rand(b, generator=g, dtype=torch.float64) * 2
    c = torch.rand(b, generator=g, dtype=torch.float64) + 0.5
    db, s, c = (v.float().double() for v in (db, s, c))   # (the tables are fp32)
    flip = torch.randint(0, 2, (b, ), generator=g)
    ry, rx = int(h * 0.125 + 0.5), int(w * 0.125 + 0.5)
    t_y, t_x = torch.randint(-ry, ry + 1, (b, ), generator=g), torch.randint(-rx, rx + 1, (b, ), generator=g)
    ch, cw = int(h * 0.5 + 0.5), int(w * 0.5 + 0.5)
    off_y = torch.randint(0, h + (1 - ch % 2), (b, ), generator=g)
    off_x = torch.randint(0, w + (1 - cw % 2), (b, ), generator=g)
    raw = (db, s, c, flip, t_y, t_x, ch, cw, off_y, off_x)
    ipar = [[int(flip[i]), -int(t_y[i]), -int(t_x[i]), *da.cut_box(h, w, ch, cw, int(off_y[i]), int(off_x[i]))] for i in range(b)]
    return raw, da.AugmentParams.from_tables(torch.stack([db, s, c], 1).tolist(), ipar)


@pytest.mark.parametrize('shape', [(2, 3, 11, 13), (1, 3, 8, 8)])
def test_reference_matches_the_diffaugment_operators(shape):
    b, _, h, w = shape
    worst = 0.0
    for seed in range(40):   # (forty sets of draws per shape: every shift, both parities of the flip, boxes at every border)
        x = torch.rand(shape, generator=torch.Generator().manual_seed(100 + seed), dtype=torch.float64)
        raw, par = _drawn(b, h, w, seed)
        want, got = _diffaugment(x, *raw), da.d_augment_torch(x, par)
        assert got.dtype == torch.float64 and got.shape == x.shape
        assert bool(((want == 0) == (got == 0)).all())    # the zeros are the same pixels
        worst = max(worst, float((got - want).abs().max()))
    # float64, a dozen operations on values below 4: the two forms differ by rounding only
    assert worst <= 64 * 2.0 ** -53 * 4, worst


def test_reference_identity_and_bias():
    x = torch.rand(2, 3, 11, 13, dtype=torch.float64)
    assert torch.equal(da.d_augment_torch(x, da.identity_params(2)), x)
    _, par = _drawn(2, 11, 13, 1)
    lin = da.d_augment_torch(x, par, bias=False)
    zero = da.d_augment_torch(torch.zeros_like(x), par)            # T(0) = b
    assert float((da.d_augment_torch(x, par) - (lin + zero)).abs().max()) <= 1e-14
    assert float(da.d_augment_torch(torch.zeros_like(x), par, bias=False).abs().max()) == 0.0


@pytest.mark.parametrize('shape', [(2, 3, 11, 13), (1, 3, 8, 8)])
def test_adjoint_identity(shape):
    """<T_lin x, g> = <x, T_lin^T g> in float64, the right side through torch.autograd.grad of d_augment_torch"""
    b, _, h, w = shape
    for seed in range(8):
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(shape, generator=gen, dtype=torch.float64).requires_grad_(True)
        g = torch.randn(shape, generator=gen, dtype=torch.float64)
        _, par = _drawn(b, h, w, seed)
        y = da.d_augment_torch(x, par)                                   # (the bias does not enter the gradient)
        gx, = torch.autograd.grad(y, x, g)
        lhs, rhs = (da.d_augment_torch(x.detach(), par, bias=False) * g).sum(), (x.detach() * gx).sum()
        assert abs(lhs.item() - rhs.item()) <= 1e-12 * max(1.0, abs(lhs.item())), (lhs.item(), rhs.item())


def test_wrappers_refuse_cpu_tensors():
    with pytest.raises(NotImplementedError):
        da.d_augment(torch.zeros(1, 3, 8, 8), da.identity_params(1))


# ------------------------------------------------------------------ AdaptiveP
def test_adaptive_p_arithmetic():
    ada = da.AdaptiveP(0.5, target=0.6, interval=4, speed_kimg=500)
    p, rt = ada.update(0.5, 6.0, 8.0)                   # r_t = 0.75 > 0.6: up by 8 / 500000
    assert rt == 0.75 and p == 0.5 + 8.0 / 500000.0
    p, rt = ada.update(0.5, -2.0, 8.0)                  # r_t = -0.25: down
    assert rt == -0.25 and p == 0.5 - 8.0 / 500000.0
    assert da.AdaptiveP(0.5, target=0.5).update(0.5, 4.0, 8.0) == (0.5, 0.5)   # on the target exactly: no move
    assert ada.update(0.5, 48.0, 64.0)[0] == 0.5 + 64.0 / 500000.0          # the step is weighted by the count
    fast = da.AdaptiveP(0.5, target=0.6, interval=1, speed_kimg=0.001)      # one image per unit of p
    assert fast.update(0.75, 8.0, 8.0)[0] == 1.0 and fast.update(0.25, -8.0, 8.0)[0] == 0.0   # clamps
    assert fast.update(0.25, 0.0, 0.0) == (0.25, None)                      # nothing accumulated: nothing moves


def test_adaptive_p_steps_reads_once_per_interval_and_round_trips():
    ada = da.AdaptiveP(0.5, target=0.0, interval=3, speed_kimg=1.0)
    reads = []
    real_read = ada.read
    ada.read = lambda: reads.append(1) or real_read()
    for step in range(1, 7):
        ada.accumulate(torch.tensor([[1.0], [2.0], [-1.0], [3.0]]))      # sign sum 2 of 4 images: r_t = 0.5 > 0
        if step == 2:
            twin = da.AdaptiveP(0.9, target=0.0, interval=3, speed_kimg=1.0)
            twin.load_state_dict(ada.state_dict())
            assert twin.p == 0.5 and twin.steps == 1 and twin.acc.tolist() == [4.0, 8.0]   # (saved behind step 2's accumulate)
        assert ada.step() == (step % 3 == 0)
    assert len(reads) == 2 and ada.rt == 0.5 and ada.p == 0.5 + 2 * 12.0 / 1000.0 and ada.acc is None
    # several outputs per image: an image counts once, with the mean sign of its outputs
    ada.accumulate(torch.tensor([[1.0, 1.0, -1.0, 1.0], [-1.0, -1.0, -1.0, -1.0]]))
    assert ada.acc.tolist() == [-0.5, 2.0]


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from mrefsr_amd import dist_util
    from mrefsr_amd.archs import d_augment as da
    dist_util.init_dist('pytorch', backend='gloo')
    words = da.all_reduce_words(torch.tensor([1.0 + rank, 4.0], dtype=torch.float64))
    ada = da.AdaptiveP(0.5, target=0.0, interval=1, speed_kimg=1.0)
    ada.accumulate(torch.full((4, 1), 1.0 if rank == 0 else -1.0))      # rank 0: +4 of 4, rank 1: -4 of 4 -> r_t = 0 on both
    ada.accumulate(torch.full((2, 1), 1.0))                             # +2 of 2 on both: r_t = 4 / 12
    ada.step()
    q.put((rank, words.tolist(), ada.p, ada.rt))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_of_the_two_words_world_size_2_gloo():
    import torch.multiprocessing as mp
    assert da.all_reduce_words(torch.tensor([1.0, 2.0])).tolist() == [1.0, 2.0]   # no process group: unchanged
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in res:
        assert r[1] == [3.0, 8.0] and r[3] == 4.0 / 12.0 and r[2] == 0.5 + 12.0 / 1000.0   # every rank holds the same p
