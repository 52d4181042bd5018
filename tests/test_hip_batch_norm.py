"""GPU suite: the trainable batch norm of csrc/batch_norm.hip (layers/batch_norm.py: BatchNorm2d) against the fp64
restatement tests/deeplab_ref.py: batch_norm_train (F.batch_norm, stock torch, CPU), max-norm relative 1e-4 — the bar
that already holds GroupNorm and the single operators."""
import pytest
import torch
import torch.nn.functional as F

import deeplab_ref as R

pytestmark = pytest.mark.gpu

from jtsm_amd.layers.batch_norm import BatchNorm2d, FrozenBatchNorm2d, get_norm  # noqa: E402
from jtsm_amd.layers.wrappers import Conv2d  # noqa: E402

REL = 1e-4
CL = torch.channels_last


@pytest.fixture
def f32_math():
    from jtsm_amd.layers import conv as K
    before = K.MATH
    K.set_math("f32")
    yield
    K.set_math(before)


def _map(case, gen, offset=0.0, spread=1.0):
    """The case's input map on the CPU (channels-last; `slice`: a [:, :24] view of a 32-channel map)."""
    if case == "slice":
        wide = (torch.randn(2, 32, 6, 5, generator=gen) * spread + offset).contiguous(memory_format=CL)
        return wide[:, :24]
    return (torch.randn(*case, generator=gen) * spread + offset).contiguous(memory_format=CL)


CASES = [(2, 24, 9, 7), (1, 256, 1, 5), (3, 4, 33, 40), "slice"]


def _run(x_cpu, relu, with_res, gen, cuda, norm="BN"):
    c = x_cpu.shape[1]
    bn = get_norm(norm, c).to(cuda)
    assert isinstance(bn, BatchNorm2d)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=gen) * 0.3)
        bn.running_mean.copy_(torch.randn(c, generator=gen))
        bn.running_var.copy_(torch.rand(c, generator=gen) + 0.5)
    start = {k: v.detach().cpu().clone() for k, v in bn.state_dict().items()}
    dy = torch.randn(*x_cpu.shape, generator=gen).contiguous(memory_format=CL)
    res = torch.randn(*x_cpu.shape, generator=gen).contiguous(memory_format=CL) if with_res else None
    # the device copy keeps the CPU tensor's strides (the slice stays a slice of a wider map)
    if x_cpu.stride(3) != c and x_cpu.shape[3] > 1:
        wide = x_cpu._base.to(cuda)
        x = wide[:, :c].detach().requires_grad_(True)
    else:
        x = x_cpu.to(cuda).requires_grad_(True)
    r = res.to(cuda).requires_grad_(True) if with_res else None
    bn.train()
    y = bn.fused(x, relu, r)
    y.backward(dy.to(cuda))
    torch.cuda.synchronize()
    got = {"y": y, "dx": x.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "dres": r.grad if with_res else None,
           "running_mean": bn.running_mean, "running_var": bn.running_var}
    want = R.batch_norm_train(x_cpu, start["weight"], start["bias"], dy, res, relu, bn.eps, bn.momentum,
                              start["running_mean"], start["running_var"])
    return got, want, bn, start


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else c)
def test_batch_norm_matches_fp64(case, relu, with_res, cuda):
    gen = torch.Generator().manual_seed(7)
    x_cpu = _map(case, gen)
    if case == "slice":
        assert x_cpu.stride(3) == 32 and x_cpu.shape[1] == 24      # leading dimension != C
    got, want, bn, start = _run(x_cpu, relu, with_res, gen, cuda)
    for key in ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var") + (("dres",) if with_res else ()):
        err = R.max_rel(got[key], want[key])
        print(key, err)
        assert err <= REL, (key, err)
    assert int(bn.num_batches_tracked) == int(start["num_batches_tracked"]) + 1
    assert sorted(bn.state_dict()) == ["bias", "num_batches_tracked", "running_mean", "running_var", "weight"]


def test_large_mean_small_spread_keeps_its_variance(cuda):
    """x = randn * 0.25 + 30: one-pass fp32 E[x^2] - E[x]^2 is off by 1.7e-3 here, torch's fp32 batch norm by 1.4e-6."""
    gen = torch.Generator().manual_seed(11)
    x_cpu = _map((2, 24, 9, 7), gen, offset=30.0, spread=0.25)
    naive = x_cpu.float()
    one_pass = (naive * naive).mean(dim=(0, 2, 3)) - naive.mean(dim=(0, 2, 3)) ** 2
    assert R.max_rel(one_pass, x_cpu.double().var(dim=(0, 2, 3), unbiased=False)) > 1e-4   # the naive form does fail here
    got, want, _, _ = _run(x_cpu, True, True, gen, cuda)
    for key in ("y", "dx", "dgamma", "dbeta", "dres", "running_mean", "running_var"):
        err = R.max_rel(got[key], want[key])
        print(key, err)
        assert err <= REL, (key, err)


def test_two_runs_give_identical_bits(cuda):
    outs = []
    for _ in range(2):
        gen = torch.Generator().manual_seed(5)
        got, _, _, _ = _run(_map((3, 4, 33, 40), gen), True, True, gen, cuda)
        outs.append({k: v.detach().clone() for k, v in got.items()})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_syncbn_at_world_size_one_is_bn(cuda):
    a, b = [], []
    for norm, out in (("BN", a), ("SyncBN", b)):
        gen = torch.Generator().manual_seed(3)
        got, _, bn, _ = _run(_map((2, 24, 9, 7), gen), True, False, gen, cuda, norm)
        assert bn.sync == (norm == "SyncBN")
        out.extend(got[k].detach().clone() for k in ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var"))
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for name in ("nnSyncBN", "naiveSyncBN"):
        assert get_norm(name, 8).sync


def test_eval_mode_folds_into_the_convolution_and_freezing_keeps_the_bits(cuda, f32_math):
    gen = torch.Generator().manual_seed(9)
    conv = Conv2d(16, 24, kernel_size=3, padding=1, bias=False, norm=get_norm("BN", 24), activation=F.relu).to(cuda)
    with torch.no_grad():
        conv.norm.weight.copy_(torch.rand(24, generator=gen) + 0.5)
        conv.norm.bias.copy_(torch.randn(24, generator=gen))
        conv.norm.running_mean.copy_(torch.randn(24, generator=gen))
        conv.norm.running_var.copy_(torch.rand(24, generator=gen) + 0.5)
    x = torch.randn(2, 16, 9, 7, generator=gen).contiguous(memory_format=CL)
    conv.eval()
    with torch.no_grad():
        y = conv(x.to(cuda))
    bn = conv.norm
    w64 = conv.weight.detach().double().cpu().contiguous()
    scale = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.double().cpu() + bn.eps)
    want = F.conv2d(x.double(), w64, padding=1) * scale.view(1, -1, 1, 1) + \
        (bn.bias.detach().double().cpu() - bn.running_mean.double().cpu() * scale).view(1, -1, 1, 1)
    assert R.max_rel(y, F.relu(want)) <= REL
    FrozenBatchNorm2d.convert_frozen_batchnorm(conv)
    assert isinstance(conv.norm, FrozenBatchNorm2d)
    with torch.no_grad():
        y2 = conv(x.to(cuda))
    assert torch.equal(y, y2)


def test_conv2d_trains_through_the_live_norm(cuda, f32_math):
    """Conv2d with a live BatchNorm2d: contraction, then the fused norm + residual + ReLU pass, against fp64."""
    gen = torch.Generator().manual_seed(13)
    conv = Conv2d(16, 24, kernel_size=1, bias=False, norm=get_norm("BN", 24), activation=F.relu).to(cuda)
    x = torch.randn(2, 16, 9, 7, generator=gen).contiguous(memory_format=CL)
    skip = torch.randn(2, 24, 9, 7, generator=gen).contiguous(memory_format=CL)
    conv.train()
    xg, sg = x.to(cuda).requires_grad_(True), skip.to(cuda).requires_grad_(True)
    y = conv(xg, residual=sg)
    y.sum().backward()
    x64, s64 = x.double().requires_grad_(True), skip.double().requires_grad_(True)
    w64 = conv.weight.detach().double().cpu().contiguous().requires_grad_(True)
    ref = F.relu(F.batch_norm(F.conv2d(x64, w64), None, None, torch.ones(24, dtype=torch.float64),
                              torch.zeros(24, dtype=torch.float64), True, 0.1, 1e-5) + s64)
    ref.sum().backward()
    assert R.max_rel(y, ref) <= REL
    assert R.max_rel(xg.grad, x64.grad) <= REL and R.max_rel(sg.grad, s64.grad) <= REL
    assert R.max_rel(conv.weight.grad, w64.grad) <= REL
    assert int(conv.norm.num_batches_tracked) == 1
