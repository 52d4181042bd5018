"""GPU suite: the fused GroupNorm(+ReLU) of csrc/semseg_ops.hip (layers/elementwise.py: group_norm_relu, what
wrappers.Conv2d calls for an nn.GroupNorm) against stock torch in fp64 on the CPU (F.group_norm, F.relu), max-norm
relative 1e-4, at every branch of its launch plan: slabs of 256 pixels, a forward fold of 16 slices, a backward fold of
1024 / pad64(C) slices, chunks of 4 channels of which 256 / (C/4) threads own one."""
import pytest
import torch
import torch.nn.functional as F

import deeplab_ref as R

pytestmark = pytest.mark.gpu

from jtsm_amd.layers.elementwise import group_norm_relu  # noqa: E402

REL = 1e-4
EPS = 1e-5
CL = torch.channels_last
KEYS = ("y", "dx", "dgamma", "dbeta")


def gn_geom(hw, c, groups):
    """The launch plan of jtsm_group_norm_forward_f32 / _backward_f32 restated: the class of a case."""
    slabs = -(-hw // 256)
    cpad = -(-c // 64) * 64
    return {"slabs": slabs, "fwd_trips": -(-slabs // 16), "bwd_slices": 1024 // cpad,
            "bwd_trips": -(-slabs // (1024 // cpad)), "chunks": c // 4, "chunks_per_group": c // 4 // groups,
            "fold_lanes": (c, cpad)}


def _inputs(case, gen, offset=0.5, spread=2.0):
    n, c, g, h, w = case
    x = torch.randn(n, c, h, w, generator=gen) * spread + offset
    ga, be = torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen) * 0.3
    dy = torch.randn(n, c, h, w, generator=gen)
    return x, ga, be, dy


def _reference(x, ga, be, dy, groups, relu, dtype=torch.float64, gate=None):
    """Stock F.group_norm (+ F.relu) and its gradients for the upstream `dy`.  `gate`: a boolean map that stands for the
    ReLU's own y > 0 in the backward (see test_large_mean_small_spread_keeps_its_variance); "z" is the pre-activation."""
    xr, gr, br = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, ga, be))
    z = F.group_norm(xr, groups, gr, br, EPS)
    y = (F.relu(z) if gate is None else z * gate.to(dtype)) if relu else z
    y.backward(dy.to(dtype))
    return {"y": F.relu(z.detach()) if relu else z.detach(), "z": z.detach(), "dx": xr.grad, "dgamma": gr.grad,
            "dbeta": br.grad}


def _device(x, ga, be, dy, groups, relu, cuda):
    xd = x.to(cuda).contiguous(memory_format=CL).requires_grad_(True)
    gd, bd = ga.to(cuda).requires_grad_(True), be.to(cuda).requires_grad_(True)
    y = group_norm_relu(xd, gd, bd, groups, EPS, relu)
    y.backward(dy.to(cuda))
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": xd.grad, "dgamma": gd.grad, "dbeta": bd.grad}


def _compare(got, want, tag="", keys=KEYS):
    for key in keys:
        err = R.max_rel(got[key], want[key])
        print(tag, key, err)
        assert err <= REL, (tag, key, err)


# (N, C, G, H, W) and the class each is meant to hit
CASES = {
    (2, 128, 32, 65, 64): {"slabs": 17, "fwd_trips": 2, "bwd_slices": 8},           # the second trip of the forward fold
    (1, 256, 32, 70, 64): {"slabs": 18, "fwd_trips": 2, "bwd_slices": 4, "bwd_trips": 5},
    (2, 4, 1, 9, 7): {"chunks": 1, "slabs": 1, "fold_lanes": (4, 64)},              # one thread folds all 256
    (1, 1024, 32, 5, 3): {"chunks": 256, "bwd_slices": 1},                           # one backward slice
    (1, 1024, 64, 3, 3): {"chunks": 256, "chunks_per_group": 4},                     # the group limit
    (2, 16, 4, 33, 40): {"slabs": 6, "fold_lanes": (16, 64)},                        # 16 of 64 padded fold lanes live
    (2, 64, 2, 9, 7): {"chunks_per_group": 8},
    (3, 128, 32, 1, 1): {"slabs": 1, "chunks_per_group": 1},                         # one pixel
}


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "x".join(map(str, c)))
def test_group_norm_matches_fp64(case, relu, cuda):
    n, c, g, h, w = case
    cls = gn_geom(h * w, c, g)
    print(case, cls)
    for key, value in CASES[case].items():
        assert cls[key] == value, (key, cls)
    gen = torch.Generator().manual_seed(41)
    x, ga, be, dy = _inputs(case, gen)
    _compare(_device(x, ga, be, dy, g, relu, cuda), _reference(x, ga, be, dy, g, relu))


@pytest.mark.parametrize("case", [(2, 128, 32, 33, 40), (2, 128, 32, 9, 7)], ids=lambda c: "x".join(map(str, c)))
def test_large_mean_small_spread_keeps_its_variance(case, cuda):
    """x = randn * 0.25 + 30, as the batch-norm file's test of this name.  Stock fp32 F.group_norm on the CPU is within the
    bar here (2.8e-6 and 4.0e-6 on y), so a failure is the kernels': one-pass fp32 sums of x and x^2 with var = E[x^2] -
    E[x]^2 lose the variance (on the MI355X y was off by 7.3e-4 and 1.1e-3 here before the statistics were accumulated
    about a shift, 1.2e-6 after).

    Behind the ReLU: x near 30 is spaced 1.9e-6 apart and the mean is stored in fp32, so xhat is known to ~4e-6 only, and
    among 338k pixels some pre-activation lies closer to 0 than that: its gate is not decided in fp32 (stock fp32 is off
    by 0.26 on dx for this reason and its backward's own sums), and one flipped gate moves dx by a whole dy.  So the
    gradients are compared with the fp64 gradients UNDER THE KERNEL'S OWN GATE (y > 0), and the gate may differ from
    fp64's only where fp64's pre-activation is within the bar of 0."""
    groups = case[2]
    gen = torch.Generator().manual_seed(11)
    x, ga, be, dy = _inputs(case, gen, offset=30.0, spread=0.25)
    want = _reference(x, ga, be, dy, groups, True)
    stock = _reference(x, ga, be, dy, groups, True, torch.float32)
    _compare(stock, want, "stock fp32", ("y",))
    print("stock fp32, not asserted:", {k: R.max_rel(stock[k], want[k]) for k in KEYS[1:]})
    got = _device(x, ga, be, dy, groups, True, cuda)
    gate = got["y"].cpu() > 0
    flipped = gate != (want["z"] > 0)
    print("gates that differ from fp64's:", int(flipped.sum()), "of", flipped.numel())
    assert float(want["z"][flipped].abs().max() if flipped.any() else 0.0) <= REL * float(want["y"].abs().max())
    _compare(got, _reference(x, ga, be, dy, groups, True, gate=gate), "kernel")


def test_zero_affine_channels(cuda):
    """gamma = beta = 0 on a whole group and on single channels of others, with the ReLU: y, dgamma and dbeta are 0
    there, and dx is 0 on the dead group."""
    case = (2, 64, 4, 9, 7)
    gen = torch.Generator().manual_seed(43)
    x, ga, be, dy = _inputs(case, gen)
    dead = torch.zeros(64, dtype=torch.bool)
    dead[16:32] = True
    dead[[0, 37, 63]] = True
    ga[dead], be[dead] = 0.0, 0.0
    got, want = _device(x, ga, be, dy, 4, True, cuda), _reference(x, ga, be, dy, 4, True)
    assert float(want["y"][:, dead].abs().max()) == 0.0 and float(want["dx"][:, 16:32].abs().max()) == 0.0
    for key in ("y", "dgamma", "dbeta"):
        t = got[key].cpu()
        assert float((t[:, dead] if t.dim() == 4 else t[dead]).abs().max()) <= REL * float(want[key].abs().max()), key
    assert float(got["dx"][:, 16:32].abs().max()) <= REL * float(want["dx"].abs().max())
    _compare(got, want)


@pytest.mark.parametrize("case", [(2, 64, 4, 9, 7), (1, 128, 32, 65, 64)], ids=lambda c: "x".join(map(str, c)))
def test_constant_group(case, cuda):
    """x = 30 on every channel of one group: variance 0, rstd = 1 / sqrt(eps), y = beta there; dx there is
    rstd * (gamma * dy - mean(gamma * dy)), 1 / sqrt(eps) larger than elsewhere, so the two parts of y and dx are held
    to the bar separately."""
    n, c, g, h, w = case
    gen = torch.Generator().manual_seed(47)
    x, ga, be, dy = _inputs(case, gen)
    const = torch.zeros(c, dtype=torch.bool)
    const[c // g:2 * (c // g)] = True
    x[:, const] = 30.0
    got, want = _device(x, ga, be, dy, g, False, cuda), _reference(x, ga, be, dy, g, False)
    got = {k: v.cpu() for k, v in got.items()}
    assert R.max_rel(got["y"][:, const], be[const].view(1, -1, 1, 1).expand(n, -1, h, w)) <= REL
    assert float(want["dx"][:, const].abs().max()) > 10.0
    for name, sel in (("constant", const), ("others", ~const)):
        _compare({k: got[k][:, sel] for k in ("y", "dx")}, {k: want[k][:, sel] for k in ("y", "dx")}, name, ("y", "dx"))
    _compare(got, want, "", ("dgamma", "dbeta"))


def test_two_runs_give_identical_bits(cuda):
    outs = []
    for _ in range(2):
        gen = torch.Generator().manual_seed(5)
        x, ga, be, dy = _inputs((2, 128, 32, 65, 64), gen)
        outs.append(_device(x, ga, be, dy, 32, True, cuda))
    for k in KEYS:
        assert torch.equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("c,groups", [(96, 8), (32, 32), (1024, 128)], ids=["C4_24_of_256", "one_channel_groups", "128_groups"])
def test_unsupported_shapes_are_refused_before_a_launch(c, groups, cuda):
    """C/4 = 24 does not divide 256, one channel per group, and more than 64 groups: an error from the layer, an error
    code from both C entry points, and every prefilled output and the workspace keep their bits."""
    from jtsm_amd import _lib as L
    gen = torch.Generator().manual_seed(53)
    x = torch.randn(2, c, 5, 3, generator=gen).to(cuda).contiguous(memory_format=CL)
    ga, be = torch.ones(c, device=cuda), torch.zeros(c, device=cuda)
    with pytest.raises((RuntimeError, ValueError)):
        group_norm_relu(x, ga, be, groups, EPS, True)
    lib, p = L.lib(), L.ptr
    maps = torch.full((2,) + tuple(x.shape), 777.0, device=cuda).contiguous()       # y, dx
    small = torch.full((4, max(2 * groups, c)), 777.0, device=cuda)                  # mean, rstd, dgamma, dbeta
    ws = torch.full((max(lib.jtsm_group_norm_workspace_bytes(2, 15, c), 16) // 4 + 4,), 777.0, device=cuda)
    rc = lib.jtsm_group_norm_forward_f32(p(x), p(ga), p(be), p(maps[0]), p(small[0]), p(small[1]), p(ws), 2, 15, c,
                                         groups, EPS, 1, L.stream())
    rc2 = lib.jtsm_group_norm_backward_f32(p(x), p(x), p(ga), p(be), p(small[0]), p(small[1]), p(maps[1]), None, None,
                                           p(small[2]), p(small[3]), p(ws), 2, 15, c, groups, 1, L.stream())
    torch.cuda.synchronize()
    assert rc != 0 and rc2 != 0
    with pytest.raises(RuntimeError):
        L.check(rc, "group_norm_forward")
    for name, t in (("maps", maps), ("vectors", small), ("workspace", ws)):
        assert bool((t == 777.0).all()), name
