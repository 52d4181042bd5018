"""Writes tests/golden/panoptic_deeplab.npz: the inputs of tests/panoptic_deeplab_ref.py (synthetic_scene, target_scene)
and what the reference's own post_processing.py and target_generator.py give for them.  Both files are imported
stand-alone by path from a checkout of the reference (they need torch and NumPy only); nothing of them is copied.

    python tools/make_panoptic_deeplab_golden.py /path/to/reference
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import panoptic_deeplab_ref as R  # noqa: E402


def _load(reference, name):
    path = os.path.join(reference, "projects", "Panoptic-DeepLab", "panoptic_deeplab", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def main(reference):
    post, target = _load(reference, "post_processing"), _load(reference, "target_generator")
    out = {}
    logits, heat, offsets = R.synthetic_scene()
    sem = logits.argmax(dim=0, keepdim=True)
    S = R.SCENE
    pan, centers = post.get_panoptic_segmentation(sem, heat.clone(), offsets, thing_ids=set(S["thing_ids"]),
                                                  label_divisor=S["label_divisor"], stuff_area=S["stuff_area"],
                                                  void_label=S["void_label"], threshold=S["threshold"],
                                                  nms_kernel=S["nms_kernel"], top_k=S["top_k"])
    out.update(scene_logits=logits.numpy(), scene_heat=heat.numpy(), scene_offsets=offsets.numpy(),
               scene_panoptic=pan.numpy().astype(np.int32), scene_centers=centers.numpy().astype(np.int32))
    # the centres alone, at the other NMS size and with the cut at work (top_k = 3 keeps two)
    for name, kernel, top_k in (("k3", 3, 20), ("cut", 7, 3)):
        c = post.find_instance_center(heat.clone(), threshold=S["threshold"], nms_kernel=kernel, top_k=top_k)
        out["centers_" + name] = c.numpy().astype(np.int32)
    panoptic, segments = R.target_scene()
    T = R.TARGETS
    gen = target.PanopticDeepLabTargetGenerator(T["ignore_label"], T["thing_ids"], sigma=T["sigma"],
                                                ignore_stuff_in_offset=T["ignore_stuff_in_offset"],
                                                small_instance_area=T["small_instance_area"],
                                                small_instance_weight=T["small_instance_weight"],
                                                ignore_crowd_in_semantic=T["ignore_crowd_in_semantic"])
    got = gen(panoptic, segments)
    out["target_panoptic"] = panoptic
    for k, v in got.items():
        out["target_" + k] = np.asarray(v, np.float64).reshape(-1, 2) if k == "center_points" else v.numpy()
    path = os.path.join(ROOT, "tests", "golden", "panoptic_deeplab.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})
    print("centres:", centers.tolist(), "ids:", torch.unique(pan).tolist())


if __name__ == "__main__":
    main(sys.argv[1])
