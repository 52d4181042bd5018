"""GPU suite: the fused up-sampling + hard-pixel-mining cross-entropy (csrc/deeplab_loss.hip,
layers/elementwise.py: deeplab_cross_entropy) against DeepLabCE restated with stock torch in fp64
(tests/deeplab_ref.py: F.interpolate, F.cross_entropy, torch.topk), max-norm relative 1e-4."""
import math

import pytest
import torch

import deeplab_ref as R

pytestmark = pytest.mark.gpu

from jtsm_amd.layers.elementwise import deeplab_cross_entropy, semseg_cross_entropy  # noqa: E402

REL = 1e-4
IGNORE = 255


def _inputs(shape, seed, ignored=0.1, zero_logits=False):
    """(wide channels-last logits map on the CPU whose [:, :C] slice is the input, target, weights)."""
    n, c, hs, ws, s = shape
    g = torch.Generator().manual_seed(seed)
    wide = (torch.randn(n, c + 5, hs, ws, generator=g) * 3).contiguous(memory_format=torch.channels_last)
    if zero_logits:
        wide[:, :c] = 0
    target = torch.randint(0, c, (n, hs * s, ws * s), generator=g)
    target[torch.rand(n, hs * s, ws * s, generator=g) < ignored] = IGNORE
    weights = torch.rand(n, hs * s, ws * s, generator=g) + 0.5
    return wide, target, weights


def _device_run(wide, c, target, weights, scale, frac, cuda):
    w = wide.to(cuda).requires_grad_(True)
    z = w[:, :c]
    assert z.stride(1) == 1 and (z.shape[3] == 1 or z.stride(3) == c + 5)   # a slice of a wider channels-last map
    loss, maps = deeplab_cross_entropy(z, target.to(cuda), scale, IGNORE, frac,
                                       weights.to(cuda) if weights is not None else None, return_maps=True)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), w.grad, maps


PARITY = [(2, 19, 8, 12, 4), (2, 19, 2, 3, 16), (1, 7, 5, 3, 2), (1, 19, 1, 1, 4),        # (N, C, Hs, Ws, scale)
          # scales whose reciprocal is not exact in fp32, odd ones among them (the gather window's spare rows and columns)
          (1, 7, 5, 3, 3), (2, 19, 4, 6, 5), (1, 19, 3, 5, 6), (1, 5, 2, 3, 7), (1, 19, 1, 1, 3), (1, 7, 1, 4, 5)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", PARITY, ids=lambda v: "x".join(map(str, v)))
def test_matches_topk_on_fp64_pixel_losses(shape, weighted, cuda):
    c, scale = shape[1], shape[4]
    for s in range(64):      # the first seed whose fp64 losses satisfy the precondition
        wide, target, weights = _inputs(shape, s)
        weights = weights if weighted else None
        want, dz, pl, k = R.deeplab_ce(wide[:, :c], target, scale, IGNORE, 0.2, weights)
        if R.kth_gap(pl, k) >= 1e-3:
            break
    # precondition: fp32 per-pixel losses are within ~2e-6 of fp64 here, so the selected set cannot differ
    assert k == int(0.2 * target.numel()) >= 1 and R.kth_gap(pl, k) >= 1e-3, (k, R.kth_gap(pl, k))
    loss, grad, maps = _device_run(wide, c, target, weights, scale, 0.2, cuda)
    print("loss", float(loss), float(want), "pixel-loss error", float((maps[1].cpu().double().view(-1) - pl).abs().max()))
    assert R.max_rel(maps[1].view(-1), pl) <= REL
    assert R.max_rel(loss, want) <= REL
    assert R.max_rel(grad[:, :c], dz) <= REL
    assert float(grad[:, c:].abs().max()) == 0.0                    # the padding channels' gradient is exactly 0
    assert int((maps[2] != 0).sum()) <= k


def test_ties_at_the_cut_take_the_lower_flat_index_first(cuda):
    shape = (2, 19, 8, 12, 4)
    c, scale = shape[1], shape[4]
    wide, target, _ = _inputs(shape, 2, zero_logits=True)
    k = int(0.2 * target.numel())
    valid = (target != IGNORE).view(-1)
    n_valid = int(valid.sum())
    assert n_valid > k                                              # the cut lies inside the ties
    first_k = valid & (torch.cumsum(valid.long(), 0) <= k)          # the first k non-ignored pixels in flat order
    want, dz, _, _ = R.deeplab_ce(wide[:, :c], target, scale, IGNORE, 0.2, selected=first_k)
    loss, grad, maps = _device_run(wide, c, target, None, scale, 0.2, cuda)
    assert abs(float(loss) - math.log(c) * min(k, n_valid) / k) <= REL * math.log(c)
    assert R.max_rel(loss, want) <= REL
    assert torch.equal((maps[2] != 0).view(-1).cpu(), first_k)
    assert R.max_rel(grad[:, :c], dz) <= REL


def test_ties_at_the_cut_above_256_workgroups(cuda):
    """304 x 432 = 131328 pixels are 513 tiles of 256: chunks of 512 pixels and 257 workgroups, so the finishing kernel's
    first thread folds two chunks and the tie scan crosses them.  Zero logits and weights of 2 and 1 give two loss
    values, 2 log 3 and log 3, and the cut lies inside the second."""
    shape = (1, 3, 19, 27, 16)
    c, scale = shape[1], shape[4]
    wide, target, _ = _inputs(shape, 7, zero_logits=True)
    g = torch.Generator().manual_seed(8)
    heavy = torch.rand(target.shape, generator=g) < 0.1
    weights = torch.where(heavy, 2.0, 1.0)
    k = int(0.2 * target.numel())
    valid = (target != IGNORE).view(-1)
    two, one = valid & heavy.view(-1), valid & ~heavy.view(-1)
    m = int(two.sum())
    assert target.numel() == 131328 and m < k < m + int(one.sum()), (m, k, int(one.sum()))
    chosen = two | (one & (torch.cumsum(one.long(), 0) <= k - m))  # every 2 log 3, then the first k - m log 3 in flat order
    want, dz, _, _ = R.deeplab_ce(wide[:, :c], target, scale, IGNORE, 0.2, weights, selected=chosen)
    loss, grad, maps = _device_run(wide, c, target, weights, scale, 0.2, cuda)
    assert torch.equal((maps[2] != 0).view(-1).cpu(), chosen)
    assert R.max_rel(loss, want) <= REL
    assert R.max_rel(grad[:, :c], dz) <= REL


def test_cut_inside_the_zeros(cuda):
    shape = (2, 19, 8, 12, 4)
    c, scale = shape[1], shape[4]
    wide, target, _ = _inputs(shape, 3, ignored=0.9)
    k = int(0.2 * target.numel())
    assert int((target != IGNORE).sum()) < k                        # k exceeds the number of positive losses
    z = wide[:, :c].double().contiguous().requires_grad_(True)
    pl = R.pixel_losses(z, target, scale, IGNORE)
    want = pl.sum() / k                                             # sum of all / k: every valid pixel over k
    want.backward()
    loss, grad, _ = _device_run(wide, c, target, None, scale, 0.2, cuda)
    assert R.max_rel(loss, want) <= REL
    assert R.max_rel(grad[:, :c], z.grad) <= REL


def test_fraction_one_is_the_mean_over_all_pixels(cuda):
    shape = (2, 19, 8, 12, 4)
    c, scale = shape[1], shape[4]
    wide, target, _ = _inputs(shape, 4)
    want, dz, pl, k = R.deeplab_ce(wide[:, :c], target, scale, IGNORE, 1.0)
    assert k == target.numel() and float(want) == float(pl.mean())
    loss, grad, _ = _device_run(wide, c, target, None, scale, 1.0, cuda)
    assert R.max_rel(loss, want) <= REL
    assert R.max_rel(grad[:, :c], dz) <= REL
    # NOT semseg_cross_entropy's mean over the non-ignored count
    other = semseg_cross_entropy(wide.to(cuda)[:, :c], target.to(cuda), scale, IGNORE)
    n_valid = int((target != IGNORE).sum())
    assert n_valid < target.numel()
    assert abs(float(other) * n_valid / target.numel() - float(loss)) <= REL * float(loss)
    assert abs(float(other) - float(loss)) > 1e-2 * float(loss)


def test_nan_logit_gives_nan_loss(cuda):
    shape = (1, 7, 5, 3, 2)
    wide, target, _ = _inputs(shape, 5, ignored=0.0)
    wide[0, 2, 1, 1] = float("nan")
    loss = deeplab_cross_entropy(wide.to(cuda)[:, :7], target.to(cuda), 2, IGNORE, 0.2)
    assert math.isnan(float(loss))
    want, _, _, _ = R.deeplab_ce(wide[:, :7], target, 2, IGNORE, 0.2)
    assert math.isnan(float(want))                                  # as torch.topk: NaN sorts as largest


def test_two_runs_give_identical_bits(cuda):
    shape = (2, 19, 8, 12, 4)
    wide, target, weights = _inputs(shape, 6)
    runs = [_device_run(wide, 19, target, weights, 4, 0.2, cuda) for _ in range(2)]
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
