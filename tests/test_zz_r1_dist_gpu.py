"""GPU: the lazily regularised D step with net_d inside DistributedDataParallel over a one-rank RCCL group (made in-process, which is
why this file sorts to the end of the run, next to test_zz_bench_dist_gpu.py).  R1's second backward of an iteration reaches every
parameter of D only through the `0 * real_pred[0]` term (the biases behind the last activation do not shape d D / d x): without it
DDP's reducer raises at the next forward."""
import socket

import pytest
import torch

from test_r1_train_gpu import _batch, _d_state, _small

pytestmark = pytest.mark.gpu

OPTIONS = dict(r1_reg_weight=10.0, net_d_reg_every=2, deterministic=True)


def _two_steps(model, data):
    model.feed_data(data)
    out = []
    for step in (1, 2):   # a plain step, then a regularised one
        model.optimize_parameters(step)
        out.append(_d_state(model))
    torch.cuda.synchronize()
    return out, model.get_current_log()


def test_ddp_wrapped_d_step_with_r1_equals_the_unwrapped_one():
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel
    import test_optim_train_gpu as T
    data = _batch()
    want, want_log = _two_steps(_small(OPTIONS), data)
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=1)
    saved = T._opt
    try:
        T._opt = lambda *a, **kw: dict(saved(*a, **kw), dist=True)
        model = _small(OPTIONS)
        assert isinstance(model.net_d, DistributedDataParallel) and isinstance(model.net_g, DistributedDataParallel)
        got, log = _two_steps(model, data)   # (a reducer error would be raised here)
    finally:
        T._opt = saved
        dist.destroy_process_group()
    assert log['l_d_r1'] == want_log['l_d_r1'] and log['l_d_r1'] > 0
    for (g1, p1), (g0, p0) in zip(got, want):
        for n in g0:
            assert torch.equal(g1[n], g0[n]) and torch.equal(p1[n], p0[n]), n
