"""CPU checks of the rotated-box yardstick itself (tests/rotated_ref.py) against what the reference computes:

a. the restatement reproduces the reference's RNG-free known answers (tests/structures/test_rotated_boxes.py) under
   that file's torch.allclose defaults, and lies within T_ref of the compiled reference's IoU matrices recorded in
   tests/golden/rotated_reference_cases.npz (T_ref is the largest difference the golden maker measured on exactly
   these matrices, so this also pins the restatement against drift);
b. on every golden NMS case the restatement's keep list (`>`, per-class segments, no offsets) equals the compiled
   reference's (`>=`, per class) and the keep list of the reference's offset formula: under the recorded margin
   neither the comparison operator nor the class-segment deviation changes a result."""
import os

import numpy as np
import pytest

import rotated_ref as R

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rotated_reference_cases.npz"))
T_REF, MARGIN = float(GOLDEN["T_ref"]), float(GOLDEN["margin"])
NS = (1, 63, 64, 65, 129, 260, 1000)
THRESHOLDS = (0.3, 0.5, 0.7)


@pytest.mark.parametrize("case", R.known_answer_cases(), ids=lambda c: c[0])
def test_known_answers(case):
    name, b1, b2, want = case
    got = R.iou_matrix(b1, b2)
    assert got.shape == (b1.shape[0], b2.shape[0]) and got.dtype == np.float32
    if want is None:
        assert got.min() >= 0, got
    else:
        assert R.allclose_default(got, want), (got, want)


def test_margin_recorded():
    assert MARGIN == max(1e-5, 4 * T_REF)
    assert T_REF < 1e-5     # near 1e-6 was expected; a much larger distance would want an explanation first


@pytest.mark.parametrize("c", range(12))
def test_within_t_ref_of_the_compiled_reference(c):
    b1, b2, want = GOLDEN["iou_%d_b1" % c], GOLDEN["iou_%d_b2" % c], GOLDEN["iou_%d_ref" % c]
    got = R.iou_matrix(b1, b2)
    assert (want > 0.05).sum() > 20     # the clusters overlap: the comparison is not one of zeros
    assert np.abs(got.astype(np.float64) - want).max() <= T_REF


@pytest.mark.parametrize("classes", [1, 3])
@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("n", NS)
def test_keep_lists(n, thr, classes):
    key = "nms_%d_%d_%d" % (n, round(thr * 10), classes)
    seed, jitter = int(GOLDEN[key + "_seed"]), float(GOLDEN[key + "_jitter"])
    boxes, scores, idxs = R.clustered_boxes(n, seed, jitter, classes=classes)
    inp = "in_%d_%d_%d" % (n, seed, round(jitter * 100))
    assert np.array_equal(boxes, GOLDEN[inp + "_boxes"]) and np.array_equal(scores, GOLDEN[inp + "_scores"])
    compared = []
    keep = R.batched_nms(boxes, scores, idxs, thr, compared)
    if compared:
        assert np.abs(np.concatenate(compared).astype(np.float64) - thr).min() > MARGIN - T_REF
    assert np.array_equal(keep, GOLDEN[key + "_keep"])
    assert np.array_equal(keep, GOLDEN[key + "_keep_offset"])
    if classes == 1:
        assert np.array_equal(keep, R.nms(boxes, scores, thr))
