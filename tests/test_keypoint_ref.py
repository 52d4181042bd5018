"""CPU suite: the NumPy restatement of the keypoint path (tests/keypoint_ref.py) against the vectors recorded from the
reference (tests/golden/keypoint_reference_cases.npz, tests/golden/make_keypoint_golden.py), the 4x4 transposed
convolution written as a 3x3 convolution + pixel shuffle against F.conv_transpose2d in fp64, and
select_proposals_with_visible_keypoints on a hand-made case."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_cases

sys.path.insert(0, os.path.join(GOLDEN))
import keypoint_ref as KR  # noqa: E402
import make_keypoint_golden as MK  # noqa: E402

CASES = load_cases("keypoint_reference_cases.npz")
META = {k: float(v) for k, v in CASES["meta"].items()}


def test_the_bars_come_from_the_reference_error():
    assert META["margin"] == max(1e-5, 4 * META["T_ref_decode"]) and META["loss_bar"] == max(1e-6, 4 * META["T_ref_loss"])
    assert 0 < META["T_ref_decode"] < 1e-3 and META["T_ref_loss"] < 1e-5
    assert set(MK.DECODE_CASES) | set(MK.TARGET_CASES) | set(MK.LOSS_CASES) | {"meta"} == set(CASES)


@pytest.mark.parametrize("name", sorted(MK.TARGET_CASES))
def test_targets_equal_the_reference(name):
    c = CASES[name]
    kp, rois = MK.target_inputs(int(c["N"]), int(c["K"]), int(c["S"]), int(c["seed"]))
    t, v = KR.keypoints_to_heatmap(kp, rois, int(c["S"]))
    assert np.array_equal(t, c["targets"]) and np.array_equal(v, c["valid"])
    if int(c["N"]) >= 9:    # the special points are in: on x2 / y2, outside, v = 0
        assert 0 < v.sum() < v.size and (kp[..., 0] == rois[:, None, 2]).any() and (kp[..., 2] == 0).any()


def check_decode(got, name, maps, rois):
    """The decode contract, shared with the GPU suite: x / y equal the reference's on every non-ambiguous row and lie
    at a pixel within `margin` of the fp64 maximum on the ambiguous ones; logit within margin; score within
    4 T_ref_decode relative.  The 5 % cap on ambiguous rows was asserted when the golden was recorded."""
    want = CASES[name]["out"]
    mine, amb = KR.heatmaps_to_keypoints(maps, rois, margin=META["margin"])
    assert amb.mean() <= 0.05
    got = np.asarray(got)
    assert got.shape == want.shape
    clear = ~amb
    assert np.array_equal(got[..., :2][clear].astype(np.float32), want[..., :2][clear]), name
    if amb.any():
        xi, yi = KR.pixel_of(got[..., :2], rois)
        assert (KR.value_at(maps, rois, xi, yi)[amb] >= mine[..., 2][amb] - META["margin"]).all()
    assert np.abs(got[..., 2] - want[..., 2].astype(np.float64)).max() <= META["margin"]
    assert (np.abs(got[..., 3] - want[..., 3]) <= 4 * META["T_ref_decode"] * want[..., 3]).all()


def decode_case(name):
    c = CASES[name]
    return MK.decode_inputs(str(c["kind"]), int(c["R"]), int(c["K"]), int(c["S"]), float(c["wmax"]), float(c["wmin"]),
                            int(c["seed"]))


@pytest.mark.parametrize("name", sorted(MK.DECODE_CASES))
def test_decode_restatement_against_the_reference(name):
    maps, rois = decode_case(name)
    check_decode(KR.heatmaps_to_keypoints(maps, rois), name, maps, rois)
    if name == "c4tiny":
        assert (KR.roi_sizes(rois)[2] == 1).all() and (KR.roi_sizes(rois)[3] == 1).all()
    if name == "c3blob":
        _, _, ow, oh, _, _ = KR.roi_sizes(rois)
        assert (ow * oh).max() > 3 * 10 ** 5  # far more output pixels than one pass of a 256-thread workgroup


def test_value_at_is_the_resized_map():
    maps, rois = decode_case("c2plain")
    _, ups = KR.heatmaps_to_keypoints(maps, rois, want_maps=True)
    xi = np.zeros(maps.shape[:2], np.int64)
    yi = np.array([[u.shape[1] - 1] * maps.shape[1] for u in ups])
    got = KR.value_at(maps, rois, xi, yi)
    assert np.allclose(got, np.array([u[:, -1, 0] for u in ups]), rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", sorted(MK.LOSS_CASES))
def test_loss_restatement_and_its_gradient(name):
    c = CASES[name]
    N, K, S = int(c["N"]), int(c["K"]), int(c["S"])
    logits, kp, rois = MK.loss_inputs(N, K, S, int(c["seed"]))
    t, v = KR.keypoints_to_heatmap(kp, rois, S)
    loss, grad = KR.keypoint_loss(logits, t, v, normalizer=1.0)
    assert abs(loss - float(c["sum"])) <= 1e-12 * abs(loss)
    x = torch.from_numpy(logits).double().requires_grad_(True)
    rows = torch.from_numpy(np.nonzero(v.reshape(-1))[0])
    ref = F.cross_entropy(x.view(N * K, S * S)[rows], torch.from_numpy(t.reshape(-1))[rows], reduction="sum")
    ref.backward()
    assert abs(float(ref.detach()) - loss) <= 1e-12 * abs(loss) and np.abs(x.grad.numpy() - grad).max() <= 1e-12
    vis, _ = KR.keypoint_loss(logits, t, v)
    assert abs(vis - loss / v.sum()) <= 1e-12 * abs(vis)
    zero, g0 = KR.keypoint_loss(logits, t, np.zeros_like(v))
    assert zero == 0.0 and not g0.any()


@pytest.mark.parametrize("R,C,K,H", [(1, 4, 1, 2), (2, 8, 17, 7), (2, 6, 3, 5)])
def test_transposed_convolution_identity_in_fp64(R, C, K, H):
    """ConvTranspose2d(C, K, 4, stride 2, padding 1) = the 3x3 / padding-1 convolution to 4K parity-major channels
    (jtsm_amd.layers.keypoint.transposed4x4_as_conv3x3) followed by the pixel shuffle; and the restatement of both
    the transposed convolution and the x2 bilinear equal torch's in fp64, values and gradients."""
    from jtsm_amd.layers.keypoint import transposed4x4_as_conv3x3

    g = torch.Generator().manual_seed(R * 100 + K)
    x = torch.randn(R, C, H, H + 1, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(C, K, 4, 4, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(K, generator=g, dtype=torch.float64, requires_grad=True)
    want = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    w3, b3 = transposed4x4_as_conv3x3(w, b)
    assert w3.shape[0] % 8 == 0 and w3.shape[0] >= 4 * K and not w3[4 * K:].any() and not b3[4 * K:].any()
    z = F.conv2d(x, w3, b3, padding=1)[:, :4 * K]
    W = H + 1
    got = z.reshape(R, 2, 2, K, H, W).permute(0, 3, 4, 1, 5, 2).reshape(R, K, 2 * H, 2 * W)
    assert float((got - want).detach().abs().max()) <= 1e-12
    gw3 = torch.autograd.grad(got.square().sum(), w)[0]      # the rearrangement is differentiable back to the parameter
    assert float((gw3 - torch.autograd.grad(want.square().sum(), w, retain_graph=True)[0]).abs().max()) <= 1e-9
    up = F.interpolate(want, scale_factor=2.0, mode="bilinear", align_corners=False)
    mine = KR.head_tail(x.detach().numpy(), w.detach().numpy(), b.detach().numpy())
    assert np.abs(mine - up.detach().numpy()).max() <= 1e-12
    gout = torch.randn(up.shape, generator=g, dtype=torch.float64)
    gx, gw, gb = torch.autograd.grad((up * gout).sum(), (x, w, b))
    dx, dw, db = KR.head_tail_grads(x.detach().numpy(), w.detach().numpy(), gout.numpy())
    for a, r in ((dx, gx), (dw, gw), (db, gb)):
        assert np.abs(a - r.numpy()).max() <= 1e-11 * max(1.0, float(r.abs().max()))


def test_select_proposals_with_visible_keypoints():
    from jtsm_amd.modeling.roi_heads import select_proposals_with_visible_keypoints
    from jtsm_amd.structures import Boxes, Instances, Keypoints

    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [20, 20, 30, 30], [0, 0, 10, 10], [5, 5, 6, 6]], np.float32)
    kp = np.array([[[5, 5, 2], [50, 50, 2]],        # one visible point inside: kept
                   [[5, 5, 0], [50, 50, 2]],        # the inside point is not labelled, the labelled one is outside
                   [[30, 20, 1], [0, 0, 0]],        # on the box's edge, labelled but not visible: kept
                   [[11, 5, 2], [5, -1, 2]],        # both just outside
                   [[5, 5, 1], [6, 6, 1]]], np.float32)   # corners of a small box: kept
    assert KR.select_proposals_with_visible_keypoints(boxes, kp).tolist() == [0, 2, 4]
    inst = Instances((40, 40), proposal_boxes=Boxes(torch.from_numpy(boxes)), gt_keypoints=Keypoints(kp),
                     tag=torch.arange(5))
    empty = Instances((40, 40), proposal_boxes=Boxes(torch.zeros(0, 4)), gt_keypoints=Keypoints(torch.zeros(0, 2, 3)))
    out = select_proposals_with_visible_keypoints([inst, empty])
    assert out[0].tag.tolist() == [0, 2, 4] and len(out[1]) == 0
    assert torch.equal(out[0].gt_keypoints.tensor, torch.from_numpy(kp[[0, 2, 4]]))


def test_keypoints_container():
    from jtsm_amd.structures import Instances, Keypoints

    k = Keypoints(np.arange(36, dtype=np.float64).reshape(4, 3, 3))
    assert len(k) == 4 and k.tensor.dtype == torch.float32 and k.device.type == "cpu"
    assert len(k[1]) == 1 and torch.equal(k[1].tensor[0], k.tensor[1]) and len(k[1:3]) == 2
    assert torch.equal(k[torch.tensor([3, 0, 3])].tensor, k.tensor[[3, 0, 3]])          # an index tensor, as the sampler passes
    assert torch.equal(k[torch.tensor([True, False, True, False])].tensor, k.tensor[[0, 2]])
    both = Instances.cat([Instances((8, 8), gt_keypoints=k), Instances((8, 8), gt_keypoints=k[:1])])
    assert len(both.gt_keypoints) == 5 and len(Keypoints.cat([k, k]).to(torch.device("cpu"))) == 8
    with pytest.raises(RuntimeError):
        k.to_heatmap(torch.zeros(4, 4), 56)         # no CPU path


def test_keypoint_annotation_transforms():
    from jtsm_amd.data import (HFlipTransform, ResizeTransform, TransformList, create_keypoint_hflip_indices,
                               transform_keypoint_annotations)

    names = ["nose", "left_eye", "right_eye", "left_ear", "right_ear"]
    flip = create_keypoint_hflip_indices(names, [("left_eye", "right_eye"), ("left_ear", "right_ear")])
    assert flip.tolist() == [0, 2, 1, 4, 3] and flip.dtype == np.int32
    kp = [10, 20, 2, 30, 20, 2, 50, 20, 1, 0, 0, 0, 99, 10, 2]
    same = transform_keypoint_annotations(kp, TransformList([ResizeTransform(50, 100, 100, 200)]), (100, 200))
    assert same.tolist() == [[20, 40, 2], [60, 40, 2], [100, 40, 1], [0, 0, 0], [198, 20, 2]]
    flipped = transform_keypoint_annotations(kp, TransformList([HFlipTransform(100)]), (50, 100), flip)
    assert flipped.tolist() == [[90, 20, 2], [50, 20, 1], [70, 20, 2], [1, 10, 2], [0, 0, 0]]
    out = transform_keypoint_annotations([10, 20, 2, 60, 20, 2], TransformList([ResizeTransform(50, 100, 100, 200)]), (100, 100))
    assert out.tolist() == [[20, 40, 2], [0, 0, 0]]          # left the image: unlabelled, x = y = 0
    with pytest.raises(AssertionError):
        transform_keypoint_annotations(kp, TransformList([HFlipTransform(100)]), (50, 100))
