"""CPU suite: the ROILoopPool restatement (tests/roi_loop_pool_ref.py) against answers derived by hand on small maps
(ROILoopPool_cuda.cu:10-205), and the boxes on which the two readings of `w*1.8f - w` part."""
import numpy as np
import pytest

import roi_loop_pool_ref as ref

H = W = 12


def _map(seed=0):
    """(1, 1, 12, 12): distinct small positive values below 1 (0.001 * (flat index + 1))."""
    return (np.arange(H * W, dtype=np.float32).reshape(1, 1, H, W) + 1) * np.float32(0.001)


def _one(x, roi, P=1, scale=1.0):
    out, arg = ref.forward(x, np.array([roi], np.float32), scale, P, P)
    return out[:, 0], arg[:, 0]      # (3, P, P): box, frame, context


def test_geometry_of_a_plain_box():
    # w = 7: inner 7/1.8 = 3.888..., residual 3.111.../2 = 1.555... -> (3.555, 7.444) -> [4, 7];
    # outer 12.6, residual 5.6/2 = 2.8 -> (-0.8 -> 0, 11.8) -> [0, 12]
    g = ref.geometry(np.array([0, 2, 2, 9, 9], np.float32), 1.0, H, W)
    assert g["box"] == (2, 2, 9, 9)
    assert g["inner"] == (4, 4, 7, 7)
    assert g["outer"] == (0, 0, 12, 12)


def test_frame_excludes_exactly_the_strict_interior_of_the_inner_box():
    x = _map()
    x[0, 0, 5, 5] = 100.0    # strictly inside the inner box [4, 7]: box yes, frame no
    x[0, 0, 6, 6] = 90.0     # strictly inside too
    x[0, 0, 4, 4] = 50.0     # on the inner box's border: belongs to the frame
    out, arg = _one(x, [0, 2, 2, 9, 9])
    assert out[0, 0, 0] == 100.0 and arg[0, 0, 0] == 5 * W + 5
    assert out[1, 0, 0] == 50.0 and arg[1, 0, 0] == 4 * W + 4
    x[0, 0, 4, 4] = 0.001
    x[0, 0, 7, 5] = 40.0     # the inner box's far border (h == 7) is frame too
    out, arg = _one(x, [0, 2, 2, 9, 9])
    assert out[1, 0, 0] == 40.0 and arg[1, 0, 0] == 7 * W + 5


def test_context_excludes_exactly_the_strict_interior_of_the_box():
    x = _map()
    x[0, 0, 5, 5] = 200.0    # strictly inside the box [2, 9]: context no
    x[0, 0, 3, 8] = 150.0    # strictly inside too
    x[0, 0, 2, 6] = 80.0     # the box's own border: context yes
    out, arg = _one(x, [0, 2, 2, 9, 9])
    assert out[2, 0, 0] == 80.0 and arg[2, 0, 0] == 2 * W + 6
    x[0, 0, 11, 0] = 90.0    # outside the box, inside the (clipped) outer box
    out, arg = _one(x, [0, 2, 2, 9, 9])
    assert out[2, 0, 0] == 90.0 and arg[2, 0, 0] == 11 * W + 0


@pytest.mark.parametrize("corner", ["top_left", "bottom_right", "top_right", "bottom_left"])
def test_outer_box_is_clipped_at_each_map_border(corner):
    # w = 3: outer 5.4, residual 2.4/2 = 1.2.  At (0, 0, 3, 3): (-1.2 -> 0, 4.2) -> [0, 4].
    # At (8, 8, 11, 11): (6.8, 12.2 -> 12) -> [7, 12], bins [7, 13) clipped to [7, 12).
    lo, hi = (0, 3), (8, 11)
    ys = lo if corner in ("top_left", "top_right") else hi
    xs = lo if corner in ("top_left", "bottom_left") else hi
    roi = [0, xs[0], ys[0], xs[1], ys[1]]
    g = ref.geometry(np.array(roi, np.float32), 1.0, H, W)
    orect = lambda s: (0, 4) if s == lo else (7, 12)   # noqa: E731
    assert g["outer"] == (orect(xs)[0], orect(ys)[0], orect(xs)[1], orect(ys)[1])
    x = _map()
    # a large value just outside the outer box (never pooled) and a smaller one on its inner edge
    oy = 5 if ys == lo else 6
    ox = 5 if xs == lo else 6
    x[0, 0, oy, ox] = 70.0
    ey = 4 if ys == lo else 7
    ex = 4 if xs == lo else 7
    x[0, 0, ey, ex] = 60.0
    out, arg = _one(x, roi)
    assert out[2, 0, 0] == 60.0 and arg[2, 0, 0] == ey * W + ex


def test_degenerate_box_is_forced_to_one_cell():
    x = _map()
    x[0, 0, 5, 5] = 30.0
    x[0, 0, 4, 4] = 40.0
    # x2 < x1: rectangle [5, 4] -> width max(0, 1) = 1; every bin of a 2 x 2 grid is the cell (5, 5)
    out, arg = _one(x, [0, 5, 5, 4, 4], P=2)
    assert (out[0] == 30.0).all() and (arg[0] == 5 * W + 5).all()


def test_all_zero_and_negative_bins_give_zero_and_minus_one():
    x = np.zeros((1, 1, H, W), np.float32)
    out, arg = _one(x, [0, 2, 2, 9, 9], P=2)
    assert (out == 0).all() and (arg == -1).all()
    x = -1.0 - _map()            # all negative: the reference's maxima start at 0
    out, arg = _one(x, [0, 2, 2, 9, 9], P=2)
    assert (out == 0).all() and (arg == -1).all()


def test_row_order_of_the_3r_output():
    rng = np.random.default_rng(3)
    x = rng.random((2, 3, H, W), dtype=np.float32)
    rois = np.array([[0, 1, 1, 6, 8], [1, 3, 2, 11, 10], [0, 0, 5, 4, 11]], np.float32)
    out, arg = ref.forward(x, rois, 1.0, 2, 2)
    R = len(rois)
    assert out.shape == (3 * R, 3, 2, 2)
    for n in range(R):
        o1, a1 = ref.forward(x, rois[n:n + 1], 1.0, 2, 2)
        for k in range(3):
            np.testing.assert_array_equal(out[k * R + n], o1[k])
            np.testing.assert_array_equal(arg[k * R + n], a1[k])


def test_roundf_is_half_away_from_zero():
    assert [ref.roundf(v) for v in (0.5, 1.5, 2.5, -0.5, -2.5, 0.49999997)] == [1, 2, 3, -1, -3, 0]


# Boxes (x1, y1, x2, y2 as float32, image 0, stride 8 on a 128 x 128 map) on which the two readings of the outer
# residual `w * 1.8f - w` give different integer outer rectangles: unfused (each step rounded, the product first —
# what this project computes) versus one fused multiply-add (what a contracting CUDA build may
# compute).  Found by search; listed so that the choice stays visible.
FUSED_SPLIT_BOXES = [
    # box,                                                         unfused outer,   fused outer
    ((39.31743621826172, 40.0, 139.8049774169922, 200.0), (0, 0, 22, 33), (0, 0, 23, 33)),
    ((177.0312957763672, 40.0, 356.2946472167969, 200.0), (13, 0, 53, 33), (13, 0, 54, 33)),
    ((273.1219482421875, 40.0, 423.7491149902344, 200.0), (27, 0, 61, 33), (27, 0, 60, 33)),
    ((-44.42686462402344, 40.0, 247.3065948486328, 200.0), (0, 0, 46, 33), (0, 0, 45, 33)),
]


@pytest.mark.parametrize("box,unfused,fused", FUSED_SPLIT_BOXES)
def test_fused_and_unfused_readings_differ_on_listed_boxes(box, unfused, fused):
    roi = np.array((0,) + box, np.float32)
    assert ref.geometry(roi, 0.125, 128, 128, fused=False)["outer"] == unfused
    assert ref.geometry(roi, 0.125, 128, 128, fused=True)["outer"] == fused


def test_backward_scatters_every_block_into_one_map():
    x = _map()
    x[0, 0, 5, 5] = 100.0
    x[0, 0, 4, 4] = 50.0
    x[0, 0, 11, 0] = 90.0
    rois = np.array([[0, 2, 2, 9, 9]], np.float32)
    out, arg = ref.forward(x, rois, 1.0, 1, 1)
    g = np.array([1.0, 2.0, 4.0], np.float32).reshape(3, 1, 1, 1)
    gin = ref.backward(g, rois, arg, 1, 1, H, W)
    want = np.zeros((H, W), np.float32)
    want[5, 5], want[4, 4], want[11, 0] = 1.0, 2.0, 4.0
    np.testing.assert_array_equal(gin[0, 0], want)
