"""CPU suite: the restatements the PCL GPU tests compare against.

* tests/pcl_ref.py, fed the top-ranking sets scikit-learn returned, reproduces the arrays the reference's own pcl.py
  wrote into tests/golden/pcl_reference_cases.npz (tests/golden/make_pcl_golden.py): the integer tables exactly, the
  float tables within 1e-6 relative (they are fp32 means / sums of at most a few thousand terms in [0, 1]: pairwise
  rounding is about log2(n) * 6e-8).
* the deterministic Lloyd step against the recorded scikit-learn sets: MEASURED (share of identical sets, mean Jaccard
  index), printed, not gated — only its own rules are asserted.
* the loss restatement and its gradient against an fp64 autograd evaluation of the same formula.
* tests/roi_pool_ref.py against hand-derived answers."""
import numpy as np
import pytest
import torch

import pcl_ref
import roi_pool_ref
from conftest import load_cases

INT_FIELDS = ("labels", "gt_assignment", "pc_labels", "pc_count")
FLOAT_FIELDS = ("cls_loss_weights", "pc_probs", "img_cls_loss_weights")


@pytest.fixture(scope="module")
def cases():
    c = load_cases("pcl_reference_cases.npz")
    assert len(c) >= 24
    return c


def recorded_sets(case):
    return np.split(case["top_flat"], np.cumsum(case["top_len"])[:-1])


def test_restatement_reproduces_the_reference_arrays(cases):
    for name, c in sorted(cases.items()):
        got = pcl_ref.pcl(c["boxes"], c["cls_prob"], c["im_labels"], c["cls_prob_new"], top_sets=recorded_sets(c))
        info = got["info"]
        assert not (info["degree_tie"] or info["score_tie"] or info["duplicate_box"]), name
        assert 200 <= len(c["boxes"]) and 1 <= int(c["im_labels"].sum()) <= 4
        for f in INT_FIELDS:
            want = c[f].reshape(-1)
            assert np.array_equal(got[f].astype(np.float32), want), (name, f)
        for f in FLOAT_FIELDS:
            want = c[f].reshape(-1)
            np.testing.assert_allclose(got[f], want, rtol=1e-6, atol=0, err_msg="%s %s" % (name, f))
        assert np.array_equal(got["im_labels_real"], c["im_labels_real"].reshape(-1))


def test_lloyd_agreement_with_scikit_learn_is_measured(cases, capsys):
    same, jac, total = 0, 0.0, 0
    for name, c in sorted(cases.items()):
        got = pcl_ref.pcl(c["boxes"], c["cls_prob"], c["im_labels"], c["cls_prob_new"])
        # the pools part once one centre differs, so only the first present class is comparable set by set
        mine, theirs = set(got["info"]["sets"][0].tolist()), set(recorded_sets(c)[0].tolist())
        same += mine == theirs
        jac += len(mine & theirs) / len(mine | theirs)
        total += 1
    with capsys.disabled():
        print("\nLloyd vs scikit-learn KMeans on the first present class of %d cases: identical sets %.3f, "
              "mean Jaccard %.3f" % (total, same / total, jac / total))
    assert total >= 24


def test_lloyd_rules():
    f = np.float32
    assert pcl_ref.lloyd_top_set(f([0.3])).tolist() == [0]
    assert pcl_ref.lloyd_top_set(f([0.3, 0.7])).tolist() == [1]
    assert pcl_ref.lloyd_top_set(f([0.5, 0.5, 0.5, 0.5])).tolist() == [0, 1, 2, 3]     # equal centres: the first
    v = f([0.01, 0.02, 0.015, 0.5, 0.52, 0.9, 0.91, 0.93])
    assert pcl_ref.lloyd_top_set(v).tolist() == [5, 6, 7]
    # a value midway between two centres goes to the lower one: centres 0 / 0.5 / 1 after the first pass
    assert pcl_ref.lloyd_top_set(f([0.0, 0.5, 0.75, 1.0])).tolist() == [3]


def _random_case(seed, R=150, K=6):
    rng = np.random.default_rng(seed)
    c = rng.uniform(40, 200, (R, 2))
    wh = rng.uniform(30, 90, (R, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    prev = rng.dirichlet(np.ones(K) * 0.3, R).astype(np.float32)
    labels = np.zeros(K, np.float32)
    labels[rng.choice(K, 2, replace=False)] = 1
    logits = rng.normal(0, 2, (R, K + 1))
    return boxes, prev, labels, logits


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_loss_restatement_against_fp64_autograd(seed):
    boxes, prev, labels, logits = _random_case(seed)
    probs = pcl_ref.softmax(logits)
    t = pcl_ref.pcl(boxes, prev, labels, probs.astype(np.float32))
    assert t["pc_count"].sum() > 0 and (t["labels"] == 0).any()
    z = torch.from_numpy(logits).double().requires_grad_()
    p = torch.softmax(z, dim=1)
    lab = torch.from_numpy(t["labels"].astype(np.int64))
    asg = torch.from_numpy(t["gt_assignment"].astype(np.int64))
    w = torch.from_numpy(t["cls_loss_weights"]).double()
    loss = -(w[lab == 0] * torch.log(p[lab == 0, 0].clamp_min(1e-6))).sum()
    pc = []
    for j in range(len(t["pc_labels"])):
        m = asg == j
        if int(m.sum()):
            pcj = p[m, int(t["pc_labels"][j])].clamp(1e-9, 1 - 1e-9).mean()
            pc.append(float(pcj.detach()))
            loss = loss - float(t["img_cls_loss_weights"][j]) * torch.log(pcj.clamp_min(1e-6))
    loss = loss / len(boxes)
    (loss * 1.7).backward()
    # the tables hold float32 roundings of pc_prob: 6e-8 relative
    np.testing.assert_allclose(t["pc_probs"][t["pc_count"] > 0], pc, rtol=2e-7)
    assert abs(pcl_ref.loss(probs, t) - float(loss.detach())) <= 1e-6 * abs(float(loss.detach()))
    g = pcl_ref.loss_grad_logits(logits, t, upstream=1.7)
    np.testing.assert_allclose(g, z.grad.numpy(), rtol=1e-5, atol=1e-6 * np.abs(z.grad.numpy()).max())


def test_roi_pool_ref_hand_cases():
    x = np.arange(2 * 1 * 6 * 8, dtype=np.float32).reshape(2, 1, 6, 8)
    x[1] = -x[1] - 1
    # the box (8, 8)-(31, 23) at 1/8: rectangle x 1..4, y 1..3 (31/8 = 3.875 -> 4, 23/8 = 2.875 -> 3); 2 x 2 bins:
    # bin_w = 2, bin_h = 1.5: rows [1,3) and [2,4), columns [1,3) and [3,5)
    out, arg = roi_pool_ref.forward(x, np.array([[0, 8, 8, 31, 23]], np.float32), 0.125, 2, 2)
    assert out[0, 0].tolist() == [[18, 20], [26, 28]] and arg[0, 0].tolist() == [[18, 20], [26, 28]]
    # the same box on the negative image: the first cell of each bin wins
    out, arg = roi_pool_ref.forward(x, np.array([[1, 8, 8, 31, 23]], np.float32), 0.125, 2, 2)
    assert arg[0, 0].tolist() == [[9, 11], [17, 19]] and out[0, 0].tolist() == [[-58, -60], [-66, -68]]
    # half away from zero: 12 / 8 = 1.5 -> 2 (round-half-even would give 2 too), 20 / 8 = 2.5 -> 3 (half-even: 2)
    assert roi_pool_ref.rect([0, 12, 20, 12, 20], 0.125) == (2, 3, 2, 3)
    # out of the map and degenerate boxes: empty bins give 0 / -1; a box of negative extent is one cell wide
    out, arg = roi_pool_ref.forward(x, np.array([[0, 100, 100, 120, 120], [0, 24, 16, 8, 8]], np.float32), 0.125, 2, 2)
    assert (out[0] == 0).all() and (arg[0] == -1).all()
    assert arg[1, 0].tolist() == [[19, 19], [19, 19]]
    # backward: the gradients of bins that picked the same cell add up
    g = np.ones((1, 1, 2, 2), np.float32)
    gin = roi_pool_ref.backward(g, np.array([[0, 24, 16, 8, 8]], np.float32), arg[1:2], 2, 1, 6, 8)
    assert gin[0, 0, 2, 3] == 4 and gin.sum() == 4
