"""CPU: tests/panoptic_deeplab_ref.py (the restatement the GPU tests compare the kernels with) and the package's target
generator equal, bit for bit, what the reference's own post_processing.py and target_generator.py gave for the same
inputs (tests/golden/panoptic_deeplab.npz, written by tools/make_panoptic_deeplab_golden.py)."""
import os

import numpy as np
import pytest
import torch

import panoptic_deeplab_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "panoptic_deeplab.npz")
TARGET_KEYS = ("sem_seg", "center", "offset", "sem_seg_weights", "center_weights", "offset_weights", "center_points")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_scene_inputs_are_the_recorded_ones(golden):
    logits, heat, offsets = R.synthetic_scene()
    for name, t in (("scene_logits", logits), ("scene_heat", heat), ("scene_offsets", offsets)):
        assert np.array_equal(golden[name], t.numpy()), name
    pan, _ = R.target_scene()
    assert np.array_equal(golden["target_panoptic"], pan)


def test_panoptic_map_and_centres(golden):
    S = R.SCENE
    sem = torch.from_numpy(golden["scene_logits"]).argmax(dim=0, keepdim=True)
    pan, centers, rows = R.get_panoptic_segmentation(
        sem, torch.from_numpy(golden["scene_heat"]), torch.from_numpy(golden["scene_offsets"]), set(S["thing_ids"]),
        S["label_divisor"], S["stuff_area"], S["void_label"], S["threshold"], S["nms_kernel"], S["top_k"])
    assert pan.dtype == torch.int64 and np.array_equal(pan.numpy(), golden["scene_panoptic"])
    assert np.array_equal(centers.numpy(), golden["scene_centers"])
    # the scene is what the GPU tests need it to be: a voided stripe and corner, two instances of one class, and a
    # table that lists exactly the ids of the map
    ids = set(np.unique(golden["scene_panoptic"]).tolist())
    assert S["void_label"] in ids and 2 * S["label_divisor"] not in ids and 3 * S["label_divisor"] not in ids
    assert {4 * S["label_divisor"] + 1, 4 * S["label_divisor"] + 2} <= ids
    assert {r[0] for r in rows} == ids - {S["void_label"]}
    assert all(int((golden["scene_panoptic"] == r[0]).sum()) == r[4] for r in rows)


@pytest.mark.parametrize("name,kernel,top_k", [("k3", 3, 20), ("cut", 7, 3)])
def test_centres_alone(golden, name, kernel, top_k):
    c = R.find_instance_center(torch.from_numpy(golden["scene_heat"]), R.SCENE["threshold"], kernel, top_k)
    assert np.array_equal(c.numpy(), golden["centers_" + name])
    assert c.shape[0] <= top_k - 1


def test_plateau_yields_no_centre():
    assert R.find_instance_center(torch.full((1, 9, 11), 0.5), 0.1, 3, 5).shape[0] == 0


def test_target_restatement(golden):
    pan, segments = R.target_scene()
    got = R.generate_targets(pan, segments, **R.TARGETS)
    for k in TARGET_KEYS:
        want = golden["target_" + k]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        assert np.array_equal(got[k], want), k
    assert len(got["center_points"]) == 4 and got["sem_seg_weights"].max() == 3 and got["center"].max() == 1


def test_target_generator_class(golden):
    from jtsm_amd.data import PanopticDeepLabTargetGenerator
    T = dict(R.TARGETS)
    gen = PanopticDeepLabTargetGenerator(T.pop("ignore_label"), T.pop("thing_ids"), **T)
    pan, segments = R.target_scene()
    got = gen(pan, segments)
    for k in TARGET_KEYS:
        want = golden["target_" + k]
        have = np.asarray(got[k], np.float64).reshape(-1, 2) if k == "center_points" else got[k].numpy()
        assert have.dtype == want.dtype and np.array_equal(have, want), k
