"""CPU suite: the host-side combine of SyncBN (jtsm_amd/layers/batch_norm.py: combine_statistics,
combine_gradient_sums) with world_size 2 on gloo.  The kernels cannot run without a GPU, so the per-rank
(count, mean, M2) and (sum dy, sum dy * xhat) come from torch ops here, on UNEQUAL shards (3 and 5 rows of an
(8, 6, 4, 4) batch): after the exchange, statistics, output and dx of each rank are the full-batch fp64 batch norm's
rows at 1e-4, and both ranks hold identical running statistics."""
import os
import socket

import torch
import torch.multiprocessing as mp

import deeplab_ref as R

REL = 1e-4
EPS, MOMENTUM = 1e-5, 0.1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _batch():
    g = torch.Generator().manual_seed(21)
    x = torch.randn(8, 6, 4, 4, generator=g) * 0.5 + 20.0          # mean large against the spread
    dy = torch.randn(8, 6, 4, 4, generator=g)
    gamma, beta = torch.rand(6, generator=g) + 0.5, torch.randn(6, generator=g)
    return x, dy, gamma, beta


def _worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from jtsm_amd.layers.batch_norm import combine_gradient_sums, combine_statistics

    dist.init_process_group("gloo", rank=rank, world_size=world)
    x, dy, gamma, beta = _batch()
    rows = slice(0, 3) if rank == 0 else slice(3, 8)
    x, dy = x[rows], dy[rows]
    count = x.numel() // x.shape[1]
    mean = x.mean(dim=(0, 2, 3))
    m2 = ((x - mean.view(1, -1, 1, 1)) ** 2).sum(dim=(0, 2, 3))
    total, mean_all, m2_all = combine_statistics(count, mean, m2)
    assert mean_all.dtype == mean.dtype and isinstance(total, float)
    invstd = torch.rsqrt(m2_all / total + EPS)
    running_mean = (1 - MOMENTUM) * torch.zeros(6) + MOMENTUM * mean_all
    running_var = (1 - MOMENTUM) * torch.ones(6) + MOMENTUM * m2_all / (total - 1)
    xhat = (x - mean_all.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    y = xhat * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    sums = torch.stack([dy.sum(dim=(0, 2, 3)), (dy * xhat).sum(dim=(0, 2, 3))])
    tot = combine_gradient_sums(sums)
    assert tot.dtype == sums.dtype
    dx = (gamma * invstd).view(1, -1, 1, 1) * (dy - tot[0].view(1, -1, 1, 1) / total
                                               - xhat * tot[1].view(1, -1, 1, 1) / total)
    out[rank] = (total, mean_all, m2_all, running_mean, running_var, y, dx)
    dist.destroy_process_group()


def test_world2_gloo_statistics_output_and_dx_are_the_full_batch():
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    x, dy, gamma, beta = _batch()
    want = R.batch_norm_train(x, gamma, beta, dy, eps=EPS, momentum=MOMENTUM)
    for rank, rows in ((0, slice(0, 3)), (1, slice(3, 8))):
        total, mean, m2, rm, rv, y, dx = out[rank]
        assert total == 8 * 16
        assert R.max_rel(mean, want["mean"]) <= REL
        assert R.max_rel(m2 / total, want["var"]) <= REL
        assert R.max_rel(rm, want["running_mean"]) <= REL and R.max_rel(rv, want["running_var"]) <= REL
        assert R.max_rel(y, want["y"][rows]) <= REL
        assert R.max_rel(dx, want["dx"][rows]) <= REL
    for a, b in zip(out[0][:5], out[1][:5]):       # count, statistics and running statistics: the same bits on both ranks
        assert a == b if isinstance(a, float) else torch.equal(a, b)
