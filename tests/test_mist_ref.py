"""The MIST restatement (tests/mist_ref.py) on hand-built cases whose answers are worked out here."""
import torch

import mist_ref as MR
from oracle import model as OM

K = 4


def _pile(x, y, n, step=1.0, side=40.0):
    """n boxes of `side`, each shifted by `step` from the one before: neighbours overlap almost fully."""
    return torch.tensor([[x + i * step, y, x + i * step + side, y + side] for i in range(n)])


def test_three_piles_two_classes_one_survivor_per_pile_in_score_order():
    # 20 rows: piles A (rows 0-6), B (7-13), C (14-19), far apart.  t = max(int(20 * 0.15), 1) = 3.
    boxes = torch.cat([_pile(0, 0, 7), _pile(200, 0, 7), _pile(0, 200, 6)])
    scores = torch.full((20, K), 0.001)
    scores[:, 1] += torch.arange(20) * 1e-5                          # (distinct fillers)
    scores[:, 3] += torch.arange(20) * 1e-5 + 5e-6
    scores[[0, 1, 8], 1] = torch.tensor([0.9, 0.8, 0.7])             # class 1: two in A, one in B
    scores[[15, 9, 2], 3] = torch.tensor([0.95, 0.6, 0.5])           # class 3: C, B, A
    ids = torch.tensor([1, 3])
    c = MR.candidates(boxes[:, None, :].expand(20, K, 4), scores, ids)
    assert c["t"] == 3
    # the (t, G) tensors flattened: rank-major, class-minor
    assert c["rows"].tolist() == [0, 15, 1, 9, 8, 2] and c["classes"].tolist() == [1, 3, 1, 3, 1, 3]
    m = MR.mist(boxes[:, None, :].expand(20, K, 4), scores, ids)
    # visiting order 0.95 (C), 0.9 (A), 0.8 (A: dropped), 0.7 (B), 0.6 (B: dropped), 0.5 (A: dropped)
    assert m["rows"].tolist() == [15, 0, 8] and m["classes"].tolist() == [3, 1, 1]
    assert torch.equal(m["scores"], torch.tensor([0.95, 0.9, 0.7])) and torch.equal(m["weights"], m["scores"])
    assert torch.equal(m["boxes"], boxes[[15, 0, 8]])


def test_seven_rows_give_one_candidate_per_class_the_top1_mining():
    g = torch.Generator().manual_seed(1)
    boxes = torch.rand(7, 2, generator=g) * 300
    boxes = torch.cat([boxes, boxes + 20 + torch.rand(7, 2, generator=g) * 50], 1)
    scores = torch.rand(7, K, generator=g)
    ids = torch.tensor([0, 2])
    assert MR.top_t(7, 0.15) == 1 and int(7 * 0.15) == 1
    bpc = boxes[:, None, :].expand(7, K, 4)
    c = MR.candidates(bpc, scores, ids)
    t1 = OM.mine_top1(bpc, scores, ids, torch.zeros(K))
    assert torch.equal(c["rows"], t1["idx"]) and torch.equal(c["boxes"], t1["boxes"])
    assert torch.equal(c["scores"], t1["scores"]) and torch.equal(c["classes"], t1["classes"])


def test_the_flatten_order_is_rank_major():
    # 14 rows, t = 2, two classes, no ties: candidate (j, g) gets list index j * G + g.  A class-major flatten
    # (g * t + j) would list class 0's two rows first.
    n = 14
    boxes = _pile(0, 0, n, step=100.0)                               # all apart: everything survives
    scores = torch.full((n, K), 0.01) + torch.arange(n)[:, None] * 1e-4 + torch.arange(K)[None, :] * 1e-5
    scores[[3, 5], 0] = torch.tensor([0.9, 0.5])
    scores[[7, 11], 2] = torch.tensor([0.8, 0.6])
    ids = torch.tensor([0, 2])
    c = MR.candidates(boxes[:, None, :].expand(n, K, 4), scores, ids)
    assert c["t"] == 2 and c["rows"].tolist() == [3, 7, 5, 11] and c["classes"].tolist() == [0, 2, 0, 2]
    m = MR.mist(boxes[:, None, :].expand(n, K, 4), scores, ids)
    assert m["rows"].tolist() == [3, 7, 11, 5] and m["classes"].tolist() == [0, 2, 2, 0]


def test_equal_scores_are_visited_in_list_order():
    # two classes share their scores: candidates (j, 0) and (j, 1) tie, the lower list index (class slot 0) is visited
    # first and suppresses its twin
    n = 14
    boxes = _pile(0, 0, n, step=100.0)
    scores = torch.full((n, K), 0.01) + torch.arange(n)[:, None] * 1e-4
    scores[[4, 9], 1] = torch.tensor([0.9, 0.5])
    scores[:, 2] = scores[:, 1]
    m = MR.mist(boxes[:, None, :].expand(n, K, 4), scores, torch.tensor([1, 2]))
    assert m["rows"].tolist() == [4, 9] and m["classes"].tolist() == [1, 1]


def test_labelling_against_a_survivor_list_longer_than_the_class_list():
    # one present class, three survivors (three piles): a proposal takes the survivor it overlaps best, background
    # below IoU 0.5; matched indices run over the SURVIVOR list (0..2), not the class list (0..0)
    boxes = torch.cat([_pile(0, 0, 7), _pile(200, 0, 7), _pile(0, 200, 7, step=15.0)])
    scores = torch.full((21, K), 0.001) + torch.arange(21)[:, None] * 1e-5
    scores[[3, 10, 14], 2] = torch.tensor([0.9, 0.8, 0.7])
    m = MR.mist(boxes[:, None, :].expand(21, K, 4), scores, torch.tensor([2]))
    assert m["rows"].tolist() == [3, 10, 14]
    lab = MR.label(boxes, m, K)
    # pile C steps by 15 px on a 40 px side: IoU with row 14 is 1, 25/55, 10/70, then 0 — only row 14 itself reaches
    # 0.5, and a proposal that overlaps nothing is matched to index 0 (the first maximum of all-zero IoUs)
    assert lab["idx"].tolist() == [0] * 7 + [1] * 7 + [2, 2, 2, 0, 0, 0, 0]
    assert lab["classes"].tolist() == [2] * 14 + [2] + [K] * 6
    assert torch.equal(lab["weights"], m["scores"][lab["idx"]])
