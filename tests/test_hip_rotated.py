"""GPU suite (pytest -m gpu): pairwise_iou_rotated, nms_rotated and batched_nms_rotated (jtsm_amd/csrc/rotated_boxes.hip)
against the NumPy restatement of the reference's device branch (tests/rotated_ref.py).

IoU: the reference's RNG-free known answers under torch.allclose's defaults; random clustered cases at (N, M) around
the 64-column tile — empty sides, one pair, 63 x 65, 64 x 64, 65 x 130 (three column tiles, a ragged last one) — with
max |kernel - restatement| <= T_ref, the distance between the reference's own two branches that
tests/golden/make_rotated_golden.py measured (it is 0: the check is bit equality; the kernel differs from the
restatement only in the device's fp64 sin / cos, whose cast to float hides a last-bit difference); degenerate rows;
one 1500 x 1500 call on zero boxes (more workgroups than one 64 x 64 tiling of a grid dimension's worth of rows).

NMS: keep lists identical to the restatement's, order included, on the golden inputs (n in 1 .. 1000 around the
64-row block, thresholds 0.3 / 0.5 / 0.7, 1 and 3 classes; the golden maker asserted that no compared IoU lies within
max(1e-5, 4 T_ref) of the threshold); the empty input; the input left unmodified; angle-0 boxes against this repo's
batched_nms on the xyxy boxes; 90 and 180 degree turns.  The generators of the last two assert the same margin on
every variant and may discard at most half of the 4 seeds they try."""
import os

import numpy as np
import pytest
import torch

import rotated_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rotated_reference_cases.npz"))
T_REF, MARGIN = float(GOLDEN["T_ref"]), float(GOLDEN["margin"])
NS = (1, 63, 64, 65, 129, 260, 1000)
THRESHOLDS = (0.3, 0.5, 0.7)


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda", 0)


def _iou(cuda, b1, b2):
    from jtsm_amd.layers import pairwise_iou_rotated
    return pairwise_iou_rotated(torch.from_numpy(b1).to(cuda), torch.from_numpy(b2).to(cuda)).cpu().numpy()


@pytest.mark.parametrize("case", R.known_answer_cases(), ids=lambda c: c[0])
def test_iou_known_answers(cuda, case):
    name, b1, b2, want = case
    got = _iou(cuda, b1, b2)
    assert got.shape == (b1.shape[0], b2.shape[0]) and got.dtype == np.float32
    if want is None:
        assert got.min() >= 0, got
    else:
        assert R.allclose_default(got, want), (got, want)
    ref = R.iou_matrix(b1, b2)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.abs(np.nan_to_num(got).astype(np.float64) - np.nan_to_num(ref)).max(initial=0.0) <= T_REF


@pytest.mark.parametrize("N,M", [(0, 5), (5, 0), (1, 1), (63, 65), (64, 64), (65, 130)])
def test_iou_random_clustered(cuda, N, M):
    both = R.clustered_boxes(N + M, 11)[0]     # one draw, so that the two sets pile on the same 6 rectangles
    b1, b2 = both[:N], both[N:]
    if N == 1 and M == 1:
        b2 = b1 + np.float32([3, 2, 1, 1, 5])          # the one pair overlaps
    got, want = _iou(cuda, b1, b2), R.iou_matrix(b1, b2)
    assert got.shape == (N, M)
    if N and M:
        diff = np.abs(got.astype(np.float64) - want)
        print("N=%d M=%d max|diff|=%.3e bit-equal %.4f%% nonzero %d" % (N, M, diff.max(), 100.0 * np.mean(got == want),
                                                                       int((want > 0).sum())))
        assert (want > 0).any()
        assert diff.max() <= T_REF


def test_iou_degenerate_rows(cuda):
    base = R.clustered_boxes(40, 21)[0]
    zero_w = base.copy()
    zero_w[:, 2] = 0
    turned = base.copy()
    turned[0::2, 4] += 720.0
    turned[1::2, 4] -= 1080.0
    far = base.copy()
    far[:, 0] += 5000.0
    for b1, b2 in ((zero_w, base), (base, zero_w), (base, base), (turned, base), (base, far)):
        got, want = _iou(cuda, b1, b2), R.iou_matrix(b1, b2)
        assert np.abs(got.astype(np.float64) - want).max() <= T_REF
    assert not _iou(cuda, zero_w, base).any() and not _iou(cuda, base, far).any()
    same = np.diag(_iou(cuda, base, base))
    assert np.abs(same.astype(np.float64) - np.diag(R.iou_matrix(base, base))).max() <= T_REF
    assert np.abs(same - 1.0).max() < 1e-5


def test_iou_many_zero_boxes(cuda):
    from jtsm_amd.layers import pairwise_iou_rotated
    z = torch.zeros(1500, 5, device=cuda)
    ious = pairwise_iou_rotated(z, z)
    assert tuple(ious.shape) == (1500, 1500) and not bool(ious.any())


# ---- NMS ----------------------------------------------------------------------------------------------------------
_KEEP = {}


def _golden_case(n, thr, classes):
    key = "nms_%d_%d_%d" % (n, round(thr * 10), classes)
    seed, jitter = int(GOLDEN[key + "_seed"]), float(GOLDEN[key + "_jitter"])
    boxes, scores, idxs = R.clustered_boxes(n, seed, jitter, classes=classes)
    inp = "in_%d_%d_%d" % (n, seed, round(jitter * 100))
    assert np.array_equal(boxes, GOLDEN[inp + "_boxes"]) and np.array_equal(scores, GOLDEN[inp + "_scores"])
    if key not in _KEEP:
        _KEEP[key] = R.batched_nms(boxes, scores, idxs, thr)
    return boxes, scores, idxs, _KEEP[key]


@pytest.mark.parametrize("classes", [1, 3])
@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("n", NS)
def test_nms_matches_restatement(cuda, n, thr, classes):
    from jtsm_amd.layers import batched_nms_rotated, nms_rotated
    boxes, scores, idxs, want = _golden_case(n, thr, classes)
    tb, ts, ti = torch.from_numpy(boxes).to(cuda), torch.from_numpy(scores).to(cuda), torch.from_numpy(idxs).to(cuda)
    before = tb.clone()
    got = batched_nms_rotated(tb, ts, ti, thr)
    assert got.dtype == torch.int64 and got.device == tb.device
    assert torch.equal(tb, before)
    assert np.array_equal(got.cpu().numpy(), want)
    if classes == 1:
        assert np.array_equal(nms_rotated(tb, ts, thr).cpu().numpy(), want)
        assert torch.equal(tb, before)


def test_nms_empty_and_half(cuda):
    from jtsm_amd.layers import batched_nms_rotated, nms_rotated
    e = torch.zeros((0, 5), device=cuda)
    for keep in (nms_rotated(e, e[:, 0], 0.5), batched_nms_rotated(e, e[:, 0], e[:, 0].long(), 0.5)):
        assert keep.dtype == torch.int64 and keep.numel() == 0 and keep.device == e.device
    boxes, scores, idxs, want = _golden_case(65, 0.5, 3)
    tb, ts, ti = torch.from_numpy(boxes).to(cuda), torch.from_numpy(scores).to(cuda), torch.from_numpy(idxs).to(cuda)
    assert np.array_equal(batched_nms_rotated(tb.half(), ts.half(), ti, 0.5).cpu().numpy(),
                          R.batched_nms(tb.half().float().cpu().numpy(), ts.half().float().cpu().numpy(), idxs, 0.5))


def _clear(boxes, scores, idxs, thr):
    compared = []
    keep = R.batched_nms(boxes, scores, idxs, thr, compared)
    near = np.abs(np.concatenate(compared).astype(np.float64) - thr).min() if compared else 1.0
    return keep, near > MARGIN


def _first_clear_seed(variants, n, thr, classes):
    """variants(boxes) -> list of box sets that must all be clear of the threshold; at least 2 of 4 seeds pass"""
    passing = []
    for seed in range(4):
        boxes, scores, idxs = R.clustered_boxes(n, 50 + seed, classes=classes)
        sets = variants(boxes)
        keeps = [_clear(b, scores, idxs, thr) for b in sets]
        if all(ok for _, ok in keeps):
            passing.append((sets, scores, idxs, [k for k, _ in keeps]))
    assert len(passing) >= 2, "the generator discarded %d of 4 seeds" % (4 - len(passing))
    return passing[0]


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_nms_angle_0_equals_axis_aligned(cuda, thr):
    from jtsm_amd.layers import batched_nms, batched_nms_rotated

    def flat(boxes):
        b = boxes.copy()
        b[:, 4] = 0
        return [b]
    (b,), scores, idxs, (want,) = _first_clear_seed(flat, 129, thr, 1)   # one class: batched_nms adds no offsets
    half = np.float32(2.0)
    xyxy = np.stack([b[:, 0] - b[:, 2] / half, b[:, 1] - b[:, 3] / half, b[:, 0] + b[:, 2] / half,
                     b[:, 1] + b[:, 3] / half], 1)
    ts, ti = torch.from_numpy(scores).to(cuda), torch.from_numpy(idxs).to(cuda)
    rot = batched_nms_rotated(torch.from_numpy(b).to(cuda), ts, ti, thr).cpu().numpy()
    axis = batched_nms(torch.from_numpy(xyxy).to(cuda), ts, ti, thr).cpu().numpy()
    assert np.array_equal(rot, want)
    assert np.array_equal(rot, axis)


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_nms_quarter_and_half_turns(cuda, thr):
    from jtsm_amd.layers import nms_rotated

    def turns(boxes):
        flat = boxes.copy()
        flat[:, 4] = 0
        quarter = flat[:, [0, 1, 3, 2, 4]].copy()
        quarter[:, 4] = 90
        half = flat.copy()
        half[:, 4] = 180
        return [flat, quarter, half]
    sets, scores, _, keeps = _first_clear_seed(turns, 129, thr, 1)
    ts = torch.from_numpy(scores).to(cuda)
    got = [nms_rotated(torch.from_numpy(np.ascontiguousarray(b)).to(cuda), ts, thr).cpu().numpy() for b in sets]
    for g, k in zip(got, keeps):
        assert np.array_equal(g, k)
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
