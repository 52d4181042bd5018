"""Keypoints — surface of detectron2/structures/keypoints.py: the (N, K, 3) = x, y, visibility annotation container
and `heatmaps_to_keypoints`.  `to_heatmap` and the decode are library calls (jtsm_amd/csrc/keypoint.hip); neither
reads anything back to the host."""
from typing import Any, List

import numpy as np
import torch


class Keypoints:
    """v = 0: not labelled (x = y = 0); v = 1: labelled, not visible; v = 2: labelled and visible."""

    def __init__(self, keypoints):
        device = keypoints.device if isinstance(keypoints, torch.Tensor) else torch.device("cpu")
        if isinstance(keypoints, (list, tuple)) and keypoints and isinstance(keypoints[0], torch.Tensor):
            keypoints = torch.stack(list(keypoints))
            device = keypoints.device
        elif isinstance(keypoints, np.ndarray):
            keypoints = torch.from_numpy(np.ascontiguousarray(keypoints))
        keypoints = torch.as_tensor(keypoints, dtype=torch.float32, device=device)
        assert keypoints.dim() == 3 and keypoints.shape[2] == 3, keypoints.shape
        self.tensor = keypoints

    def __len__(self) -> int:
        return self.tensor.size(0)

    def to(self, *args: Any, **kwargs: Any) -> "Keypoints":
        return type(self)(self.tensor.to(*args, **kwargs))

    @property
    def device(self) -> torch.device:
        return self.tensor.device

    def to_heatmap(self, boxes: torch.Tensor, heatmap_size: int):
        """(targets, valid), both (N, K): the flat cell `y * heatmap_size + x` of each keypoint inside its box (0 where
        not valid) as int32, and valid = inside the box and v > 0 as uint8 — the reference's integers in the dtypes
        the loss kernel reads."""
        from ..layers.keypoint import keypoint_targets
        return keypoint_targets(self.tensor, boxes, heatmap_size)

    def __getitem__(self, item) -> "Keypoints":
        """An int keeps one instance; a slice, a mask or an index tensor select as they do on a tensor."""
        if isinstance(item, int):
            return Keypoints(self.tensor[item][None])
        return Keypoints(self.tensor[item])

    @staticmethod
    def cat(keypoints_list: List["Keypoints"]) -> "Keypoints":
        assert len(keypoints_list) > 0 and all(isinstance(k, Keypoints) for k in keypoints_list)
        return Keypoints(torch.cat([k.tensor for k in keypoints_list], dim=0))

    def __repr__(self) -> str:
        return self.__class__.__name__ + "(num_instances={})".format(len(self.tensor))


def heatmaps_to_keypoints(maps: torch.Tensor, rois: torch.Tensor) -> torch.Tensor:
    """maps (R, K, S, S) logits, rois (R, 4) -> (R, K, 4) = x, y, logit, score.  The reference's per-roi loop (a
    bicubic F.interpolate to the box's pixel size, two reductions and an assert that reads back, per roi) as one
    launch with one workgroup per (roi, keypoint)."""
    from ..layers.keypoint import keypoint_decode
    return keypoint_decode(maps, rois)
