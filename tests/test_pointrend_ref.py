"""The host restatement (tests/pointrend_ref.py) against the vectors recorded from the reference
(tests/golden/pointrend_reference_cases.npz): float quantities within the recorded bars, chosen sets equal on every roi
that is not ambiguous within the recorded margin, at most 5 % of a case's rois ambiguous."""
import numpy as np
import pytest

import pointrend_ref as PR

Z, META = PR.golden()


def _sets_equal(mine, recorded, amb):
    assert amb.mean() <= META["ambiguous_cap"]
    for r in range(len(mine)):
        if not amb[r]:
            assert np.array_equal(np.sort(mine[r]), recorded[r]), r


@pytest.mark.parametrize("name", list(PR.GATHER_CASES))
def test_gather(name):
    fine, scales, coarse, boxes, roi_image, points = PR.gather_inputs(name, int(Z["gather_%s_seed" % name]))
    rows, coords = PR.gather(fine, scales, coarse, boxes, roi_image, points)
    assert rows.shape == Z["gather_%s_rows" % name].shape
    assert np.abs(rows - Z["gather_%s_rows" % name]).max() <= META["gather_bar"]
    assert np.abs(coords - Z["gather_%s_coords" % name]).max() <= META["coords_bar"]


def test_gather_float32_order_is_within_the_bar():
    fine, scales, coarse, boxes, roi_image, points = PR.gather_inputs("two", int(Z["gather_two_seed"]))
    rows, _ = PR.gather(fine, scales, coarse, boxes, roi_image, points, PR.F32)
    assert rows.dtype == np.float32
    assert np.abs(rows - Z["gather_two_rows"]).max() <= META["gather_bar"]


def test_gather_adjoint_is_the_transpose():
    fine, scales, coarse, boxes, roi_image, points = PR.gather_inputs("one", 5)
    rows, _ = PR.gather(fine, scales, coarse, boxes, roi_image, points)
    g = np.random.RandomState(0).randn(*rows.shape)
    df, dc = PR.gather_adjoint(g, [f.shape for f in fine], scales, coarse.shape, boxes, roi_image, points)
    lhs = (rows * g).sum()
    rhs = sum((d * f).sum() for d, f in zip(df, fine)) + (dc * coarse).sum()
    assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), 1.0)


def test_grid_orders():
    plain, s2d = PR.grid_points(14), PR.grid_points(14, True)
    q = np.arange(196)
    blk = q >> 2
    y, x = 2 * (blk // 7) + ((q >> 1) & 1), 2 * (blk % 7) + (q & 1)
    assert np.array_equal(s2d, plain[y * 14 + x])
    assert np.allclose(plain[15], [(1 + 0.5) / 14, (1 + 0.5) / 14])


@pytest.mark.parametrize("name", list(PR.SELECT_CASES))
def test_select(name):
    coarse, classes, cand, rand, P, U = PR.select_inputs(name, int(Z["select_%s_seed" % name]))
    pts, chosen, u = PR.select(coarse, classes, cand, rand, U)
    assert pts.shape == (coarse.shape[0], P, 2)
    amb = PR.ambiguous(u, U, META["select_margin"])
    _sets_equal(chosen, Z["select_%s_chosen" % name], amb)
    for r in range(len(u)):        # the order is ours: uncertainty descending, index ascending
        v = u[r, chosen[r]]
        assert np.all((v[:-1] > v[1:]) | ((v[:-1] == v[1:]) & (chosen[r][:-1] < chosen[r][1:])))
    # the random rest is the second draw, as the reference attaches it
    assert np.array_equal(pts[:, U:], Z["select_%s_coords" % name][:, U:])


def test_select_ties_go_to_the_lower_index():
    # a constant map of zeros: every candidate samples exactly 0 whatever its taps and weights, so all uncertainties tie
    # (a non-zero constant would not do: the zero padding and the weights' rounding tell the candidates apart)
    coarse, classes, cand, rand, P, U = PR.select_inputs("p8c5", 1)
    _, chosen, _ = PR.select(np.zeros_like(coarse), classes, cand, rand, U)
    assert np.array_equal(chosen, np.tile(np.arange(U), (coarse.shape[0], 1)))


@pytest.mark.parametrize("name", list(PR.LOSS_CASES))
def test_loss(name):
    args = PR.loss_inputs(name, int(Z["loss_%s_seed" % name]))
    loss, grad, targets, accurate = PR.point_loss(*args)
    assert abs(loss - float(Z["loss_%s_loss" % name])) <= META["loss_bar"]
    assert np.abs(grad - Z["loss_%s_grad" % name]).max() <= META["loss_grad_bar"] * np.abs(grad).max()
    assert np.abs(targets - Z["loss_%s_targets" % name]).max() <= META["target_bar"]
    assert accurate == int(Z["loss_%s_accurate" % name])
    assert targets.min() >= 0 and targets.max() <= 1 + 1e-12 and (targets == 0).any() and (targets >= 1 - 1e-9).any()


def test_loss_without_rois_is_zero():
    loss, grad, _, accurate = PR.point_loss(np.zeros((0, 5), np.float32), np.zeros(0, np.int64), [None], np.zeros(0, np.int32),
                                            np.zeros(0, np.int32), np.zeros((0, 7, 2), np.float32), 7)
    assert loss == 0.0 and grad.shape == (0, 5) and accurate == 0


@pytest.mark.parametrize("name", list(PR.SUBDIV_CASES))
def test_subdivide(name):
    m, N = PR.subdiv_inputs(name, int(Z["subdiv_%s_seed" % name]))
    n = PR.step_points(m.shape[1], m.shape[2], N)
    up, idx, coords = PR.subdivide(m, n)
    s = int(Z["subdiv_%s_stride" % name])
    assert np.abs(up[:, ::s, ::s] - Z["subdiv_%s_up" % name]).max() <= META["up_bar"]
    if n == 0:
        assert idx is None and name == "s7"
        return
    amb = PR.ambiguous(-np.abs(up).reshape(len(m), -1), idx.shape[1], META["subdiv_margin"])
    _sets_equal(idx, Z["subdiv_%s_chosen" % name], amb)
    W = up.shape[-1]
    assert np.allclose(coords[..., 0], (idx % W + 0.5) / W) and np.allclose(coords[..., 1], (idx // W + 0.5) / up.shape[-2])


def test_one_channel_loop_equals_the_predicted_channel_of_all_channels():
    rng = np.random.RandomState(3)
    R, C = 3, 5
    coarse = (2 * rng.randn(R, C, 7, 7)).astype(np.float32)
    classes = rng.randint(0, C, R)
    w = rng.randn(C, 2)

    def point_fn(coords):      # any function of the point alone: the point head sees the same inputs either way
        return np.tanh(coords @ w.T * 3) * 4 + PR.sample(coarse[0], coords[0, :, 0], coords[0, :, 1], PR.F64)[None] * 0

    one, amb1 = PR.subdivision_loop(coarse, classes, point_fn, 3, 28 * 28, True, META["subdiv_margin"])
    full, amb2 = PR.subdivision_loop(coarse, classes, point_fn, 3, 28 * 28, False, META["subdiv_margin"])
    assert one.shape == (R, 56, 56)
    keep = ~(amb1 | amb2)
    assert keep.any()
    assert np.abs(one[keep] - full[keep]).max() <= META["up_bar"]
