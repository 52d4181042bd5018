"""The NumPy restatement of C-MIL's ROIMerge and ROILabel (tests/cmil_ref.py) on cases worked by hand, and the host
side of the layers: lambda's end points, the threshold guard."""
import numpy as np
import pytest

import cmil_ref as CR


def _disjoint_boxes(n):
    """n boxes that do not touch: every IoU is 0."""
    x = np.arange(n, dtype=np.float32) * 10
    return np.stack([x, np.zeros(n, np.float32), x + 5, np.full(n, 5, np.float32)], 1)


def test_lambda_zero_cuts_the_top_into_windows_of_forty():
    n = 201
    S = np.linspace(1.0, 0.0, n).astype(np.float32)          # row = rank
    bx = _disjoint_boxes(n)
    I, num_id, num_top = CR.merge_ids(S, CR.pairwise_iou(bx, bx), 0.0)
    assert num_top == 5 and num_id == 6                       # 200 ranks in 5 windows, + the 201st row
    assert I[:200].tolist() == [r // 40 for r in range(200)] and I[200] == 5


def test_lambda_one_merges_identical_boxes_only():
    bx = _disjoint_boxes(6)
    bx[4] = bx[1]                                             # rows 1 and 4 coincide
    bx[5, 2] += 1e-3                                          # nearly row 5's own neighbour: no effect
    S = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4], np.float32)
    I, num_id, num_top = CR.merge_ids(S, CR.pairwise_iou(bx, bx), 1.0)
    assert I.tolist() == [0, 1, 2, 3, 1, 4] and num_id == num_top == 5


def test_a_chain_is_not_a_clique():
    # A ~ B and B ~ C but not A ~ C, ranked A, B, C: B joins A's clique, C is tested against both members and stays out
    A, B, C = [0, 0, 10, 10], [3, 0, 13, 10], [6, 0, 16, 10]
    bx = np.array([A, B, C], np.float32)
    J = CR.pairwise_iou(bx, bx)
    assert J[0, 1] > 0.5 and J[1, 2] > 0.5 and J[0, 2] < 0.5
    I, num_id, _ = CR.merge_ids(np.array([0.9, 0.8, 0.7], np.float32), J, 0.5)
    assert I.tolist() == [0, 0, 1] and num_id == 2
    # ranked B first, both neighbours are tested against B alone — then C against A as well
    I, _, _ = CR.merge_ids(np.array([0.8, 0.9, 0.7], np.float32), J, 0.5)
    assert I.tolist() == [0, 0, 1]


def test_ties_go_to_the_lower_row():
    bx = _disjoint_boxes(3)
    I, _, _ = CR.merge_ids(np.array([0.5, 0.5, 0.9], np.float32), CR.pairwise_iou(bx, bx), 0.5)
    assert I.tolist() == [1, 2, 0]


def test_means_of_a_two_member_clique_by_hand():
    C = np.array([[1.0, 3.0], [10.0, 0.5], [0.25, 7.0]], np.float32)
    D = -C
    I = np.array([0, 1, 0], np.int32)
    MC, MD, IC = CR.merge_means(C, D, I, 2)
    assert IC.tolist() == [2, 1]
    assert MC.tolist() == [[0.625, 5.0], [10.0, 0.5]] and MD.tolist() == [[-0.625, -5.0], [-10.0, -0.5]]
    # each quotient is rounded before it is added: thirds of 1 do not sum to 1
    C3 = np.ones((3, 1), np.float32)
    MC3, _, _ = CR.merge_means(C3, C3, np.zeros(3, np.int32), 1)
    third = np.float32(1) / np.float32(3)
    assert MC3[0, 0] == (third + third) + third
    gC, gD = CR.roi_merge_backward(np.array([[2.0, 4.0], [6.0, 8.0]], np.float32), np.zeros((2, 2), np.float32), I, IC)
    assert gC.tolist() == [[1.0, 2.0], [6.0, 8.0], [1.0, 2.0]] and not gD.any()


def test_batch_is_compacted_and_dead_rows_are_zero():
    rows = [3, 2]
    bx = np.concatenate([np.array([[0, 0, 10, 10], [0, 0, 10, 10], [50, 50, 60, 60]], np.float32), _disjoint_boxes(2)])
    S = np.array([0.3, 0.2, 0.1, 0.9, 0.8], np.float32)
    C = np.arange(10, dtype=np.float32).reshape(5, 2)
    out = CR.roi_merge(S, bx, C, C, np.array([0, 3, 5], np.int32), 0.7)
    assert out["merged_offsets"].tolist() == [0, 2, 4] and out["I"].tolist() == [0, 0, 1, 2, 3]
    assert out["IC"].tolist() == [2, 1, 1, 1, 0] and not out["MC"][4:].any()
    assert out["MC"][0].tolist() == [1.0, 2.0]


def test_lambda_runs_from_zero_to_one():
    assert CR.getlambda(0, 1250, 40) == 0.0 and CR.getlambda(50000, 1250, 40) == 1.0
    mid = [CR.getlambda(i, 1250, 40) for i in (1, 100, 1250, 25000)]
    assert all(0 < a < b < 1 for a, b in zip(mid, mid[1:]))
    from jtsm_amd.layers.cmil import ROIMerge, getlambda
    assert all(getlambda(i, 1250, 40) == float(CR.getlambda(i, 1250, 40)) for i in (0, 1, 777, 50000))
    m = ROIMerge(320, 40, 1250)
    assert m.cur_iter == 0 and m.lam == 0.0
    m.cur_iter = 50000
    assert m.lam == 1.0


def _label_inputs():
    # rows 0-2 overlap one another; row 3 is far away.  Class 0 and class 1 both like row 0 best.
    bx = np.array([[0, 0, 10, 10], [0, 0, 10, 9], [0, 0, 10, 4], [50, 50, 60, 60]], np.float32)
    S = np.array([[0.9, 0.8], [0.5, 0.7], [0.1, 0.2], [0.3, 0.1]], np.float32)
    return S, bx


def test_label_seeds_exclude_rows_another_class_took():
    S, bx = _label_inputs()
    rows, cls, p = CR.label_seeds(S, [0, 1])
    assert rows == [0, 1] and cls == [0, 1] and p == [np.float32(0.9), np.float32(0.7)]
    out = CR.roi_label_image(S, bx, [0, 1], np.array([0.25, 0.75], np.float32), [0, 1, 2, 3])
    # row 0: its own seed (IoU 1 against 0.9 with the other: class 0); row 1: its own seed (class 1); row 2: IoU 40/100
    # with seed 0 and 40/90 with seed 1 -> class 1, neither fg (0.6) nor below bg_hi (0.4): weight 0;
    # row 3: IoU 0 with every seed: the FIRST seed's class, below bg_lo: weight 0
    assert out["labels"].tolist() == [0, 1, 1, 0] and out["weights"].tolist() == [0.25, 0.75, 0.0, 0.0]


def test_label_more_classes_than_rows():
    S, bx = _label_inputs()
    rows, cls, _ = CR.label_seeds(S[:1], [0, 1])
    assert rows == [0] and cls == [0]                         # class 1 finds no row left
    out = CR.roi_label_image(S[:1], bx[:1], [0, 1], np.array([0.5, 0.5], np.float32), [0])
    assert out["labels"].tolist() == [0] and out["weights"].tolist() == [0.5]
    none = CR.roi_label_image(S, bx, [], np.array([0.5, 0.5], np.float32), [0, 1, 2, 3])
    assert none["labels"].tolist() == [2] * 4 and not none["weights"].any()


def test_label_caps_are_thirty_three_and_ninety_seven():
    n_fg, n_bg = 40, 110
    fg_box = np.tile(np.array([[0, 0, 10, 10]], np.float32), (n_fg, 1))               # IoU 1 with the seed
    bg_box = np.tile(np.array([[0, 0, 10, 2.5]], np.float32), (n_bg, 1))              # IoU 0.25
    bx = np.concatenate([fg_box, bg_box])
    n = n_fg + n_bg
    S = np.linspace(0.9, 0.1, n).astype(np.float32)[:, None]                           # row 0 is the seed
    perm = list(range(n - 1, -1, -1))                                                  # visited from the back
    out = CR.roi_label_image(S, bx, [0], np.array([0.5], np.float32), perm)
    assert out["eligible"] == (n_fg, n_bg)
    lab, w = out["labels"], out["weights"]
    assert (lab[:n_fg] == 0).all() and int((w[:n_fg] > 0).sum()) == 33                 # num_pos + 1 (`<=`, :141)
    assert (w[n_fg - 33:n_fg] > 0).all()                                               # the LAST 33 rows: visited first
    assert int((lab[n_fg:] == 1).sum()) == 97 and (lab[n - 97:] == 1).all()            # num_neg + 1
    assert (lab[n_fg:n - 97] == 0).all() and not w[n_fg:n - 97].any()                  # overflow: the seed's class, 0


def test_label_refuses_fg_below_bg_hi():
    S, bx = _label_inputs()
    with pytest.raises(ValueError):
        CR.roi_label_image(S, bx, [0], np.array([0.5, 0.5], np.float32), [0, 1, 2, 3], fg=0.3, bg_hi=0.4)
    from jtsm_amd.layers.cmil import ROILabel
    with pytest.raises(ValueError):
        ROILabel(0.3, 0.4, 0.1, 32, 96, 1)
    assert ROILabel(0.4, 0.4, 0.1, 32, 96, 1).num_pos == 32


# ---- against the reference's own compiled host operators (tests/golden/make_cmil_golden.py) ---------------------------
def _golden():
    import os

    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, "cmil_reference_cases.npz"))


def test_restatement_reproduces_the_recorded_roi_merge():
    z = _golden()
    sizes = set()
    for k in range(8):
        g = lambda name: z["merge%d_%s" % (k, name)]  # noqa: E731
        cur_iter, max_epoch, size_epoch = g("iters").tolist()
        n = g("S").shape[0]
        out = CR.roi_merge(g("S"), g("boxes"), g("C"), g("D"), np.array([0, n], np.int32),
                           CR.getlambda(cur_iter, size_epoch, max_epoch))
        live = g("MC").shape[0]
        assert int(out["merged_offsets"][1]) == live, k
        assert np.array_equal(out["I"], g("I")) and np.array_equal(out["IC"], g("IC")), k
        assert np.array_equal(out["MC"][:live], g("MC")) and np.array_equal(out["MD"][:live], g("MD")), k
        gC, gD = CR.roi_merge_backward(g("gM")[0], g("gM")[1], g("I"), g("IC"))
        assert np.array_equal(gC, g("GC")) and np.array_equal(gD, g("GD")), k
        sizes |= set(g("IC")[:live].tolist())
    assert min(sizes) == 1 and max(sizes) == 40, sorted(sizes)


def test_restatement_reproduces_the_recorded_roi_label():
    z = _golden()
    labelled_bg = 0
    for k in range(6):
        g = lambda name: z["label%d_%s" % (k, name)]  # noqa: E731
        n = g("S").shape[0]
        ids = np.nonzero(g("L")[0] == 1)[0]
        for perm in (np.arange(n), np.arange(n)[::-1]):                  # no cap binds: the order does not matter
            out = CR.roi_label_image(g("S"), g("boxes"), ids, g("CW"), perm, num_classes=20)
            assert np.array_equal(out["labels"], g("RL")) and np.array_equal(out["weights"], g("RW")), k
        labelled_bg += int((g("RL") == 20).sum())
    assert labelled_bg > 0
