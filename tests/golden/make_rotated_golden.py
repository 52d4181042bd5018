"""Record tests/golden/rotated_reference_cases.npz — for the build container only (it needs the reference checkout).

    python tests/golden/make_rotated_golden.py /path/to/reference

Compiles the reference's detectron2/layers/csrc/box_iou_rotated/box_iou_rotated_cpu.cpp and
nms_rotated/nms_rotated_cpu.cpp where they lie into a temporary directory (nothing of them is copied; the only file
written there is a three-line binding) and records:

  iou_<c>_b1, iou_<c>_b2, iou_<c>_ref   a dozen clustered cases (tests/rotated_ref.clustered_boxes) and the
                                        reference's IoU matrices (its HOST branch: std::sort, the compiler's FMAs)
  T_ref                                 the largest |restatement - reference| over those matrices: the distance between
                                        the reference's own device and host branches (sort order, FMA).  Measured
                                        here: 0.0 (an x86-64 build contracts nothing and the two sorts agree on
                                        these inputs); no code under test involved.
  margin                                max(1e-5, 4 * T_ref)
  nms_<n>_<thr*10>_<classes>_...        per NMS case: seed, jitter, the compiled nms_rotated keep list per class
                                        segment merged by score (`keep`), and the keep list of the reference's
                                        offset batched_nms_rotated formula (`keep_offset`)
  in_<n>_<seed>_<jitter*100>_...        boxes, scores of the NMS inputs (idxs: rotated_ref.clustered_boxes again)

A case is kept only if no IoU that the greedy pass compares lies within `margin` of the threshold (checked on the
reference's IoUs of the plain and of the offset boxes); of the 4 seeds tried per case at least 2 must pass, and the
first that passes is recorded."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rotated_ref as R  # noqa: E402

NS = (1, 63, 64, 65, 129, 260, 1000)
THRESHOLDS = (0.3, 0.5, 0.7)
CLASSES = (1, 3)

BINDING = """
#include <torch/extension.h>
namespace detectron2 {
at::Tensor box_iou_rotated_cpu(const at::Tensor& boxes1, const at::Tensor& boxes2);
at::Tensor nms_rotated_cpu(const at::Tensor& dets, const at::Tensor& scores, const float iou_threshold);
}
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("box_iou_rotated", &detectron2::box_iou_rotated_cpu);
  m.def("nms_rotated", &detectron2::nms_rotated_cpu);
}
"""


def compile_reference(root, tmp):
    from torch.utils.cpp_extension import load
    csrc = os.path.join(root, "detectron2", "layers", "csrc")
    bind = os.path.join(tmp, "binding.cpp")
    with open(bind, "w") as f:
        f.write(BINDING)
    return load(name="rotated_reference", build_directory=tmp, extra_cflags=["-O2"],
                sources=[bind, os.path.join(csrc, "box_iou_rotated", "box_iou_rotated_cpu.cpp"),
                         os.path.join(csrc, "nms_rotated", "nms_rotated_cpu.cpp")])


def offset_boxes(boxes, idxs):
    """detectron2/layers/nms.py batched_nms_rotated: centres + idxs * (max - min + 1), in fp32 torch arithmetic"""
    b = torch.from_numpy(boxes)
    max_coordinate = (torch.max(b[:, 0], b[:, 1]) + torch.max(b[:, 2], b[:, 3]) / 2).max()
    min_coordinate = (torch.min(b[:, 0], b[:, 1]) - torch.max(b[:, 2], b[:, 3]) / 2).min()
    offsets = torch.from_numpy(idxs).to(b) * (max_coordinate - min_coordinate + 1)
    out = b.clone()
    out[:, :2] += offsets[:, None]
    return out


def clear_of_threshold(ref, boxes, scores, idxs, thr, margin):
    """no IoU the greedy per-class pass compares (on `boxes`, with the reference's IoU) is within margin of thr"""
    iou = ref.box_iou_rotated(boxes, boxes).numpy()
    for c in np.unique(idxs):
        sel = np.nonzero(idxs == c)[0]
        compared = []
        R.greedy_nms(sel[R.score_order(scores[sel])], lambda i, js: iou[i, js], thr, False, compared)
        if compared and np.abs(np.concatenate(compared).astype(np.float64) - thr).min() <= margin:
            return False
    return True


def main(root):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        ref = compile_reference(root, tmp)
        half = torch.tensor([[0.5, 0.5, 1.0, 1.0, 0.0]]), torch.tensor([[0.25, 0.5, 0.5, 1.0, 0.0]])
        assert abs(float(ref.box_iou_rotated(*half)) - 0.5) < 1e-6

        t_ref = 0.0
        for c in range(12):
            both = R.clustered_boxes(64, 100 + c)[0]           # one draw: both sets pile on the same 6 rectangles
            b1, b2 = both[:24], both[24:]
            if c % 2:
                b2 = np.concatenate([b1[:10], b2[10:]])       # some identical pairs
            want = ref.box_iou_rotated(torch.from_numpy(b1), torch.from_numpy(b2)).numpy()
            t_ref = max(t_ref, float(np.abs(R.iou_matrix(b1, b2).astype(np.float64) - want).max()))
            out["iou_%d_b1" % c], out["iou_%d_b2" % c], out["iou_%d_ref" % c] = b1, b2, want
        margin = max(1e-5, 4 * t_ref)
        out["T_ref"], out["margin"] = np.float64(t_ref), np.float64(margin)
        print("T_ref = %.3e  margin = %.3e" % (t_ref, margin))

        for n in NS:
            for thr in THRESHOLDS:
                for classes in CLASSES:
                    jitter = 1.0
                    while True:
                        passing = []
                        for seed in range(4):
                            boxes, scores, idxs = R.clustered_boxes(n, seed, jitter, classes=classes)
                            tb = torch.from_numpy(boxes)
                            if clear_of_threshold(ref, tb, scores, idxs, thr, margin) and \
                                    clear_of_threshold(ref, offset_boxes(boxes, idxs), scores, idxs, thr, margin):
                                passing.append(seed)
                        if len(passing) >= 2:
                            break
                        assert n == 1000 and thr == 0.7 and jitter == 1.0, (n, thr, classes, passing)
                        jitter = 0.5                          # the one case the issue allows to tighten its clusters
                    seed = passing[0]
                    boxes, scores, idxs = R.clustered_boxes(n, seed, jitter, classes=classes)
                    tb, ts = torch.from_numpy(boxes), torch.from_numpy(scores)
                    keep = []
                    for c in np.unique(idxs):
                        sel = np.nonzero(idxs == c)[0]
                        keep.append(sel[ref.nms_rotated(tb[sel].contiguous(), ts[sel].contiguous(), thr).numpy()])
                    keep = np.concatenate(keep)
                    keep = keep[np.argsort(-scores[keep].astype(np.float64), kind="stable")]
                    keep_offset = ref.nms_rotated(offset_boxes(boxes, idxs), ts, thr).numpy()
                    key = "nms_%d_%d_%d" % (n, round(thr * 10), classes)
                    out[key + "_seed"], out[key + "_jitter"] = np.int32(seed), np.float64(jitter)
                    out[key + "_keep"], out[key + "_keep_offset"] = keep.astype(np.int32), keep_offset.astype(np.int32)
                    inp = "in_%d_%d_%d" % (n, seed, round(jitter * 100))
                    out[inp + "_boxes"], out[inp + "_scores"] = boxes, scores
                    print(key, "seeds passing", passing, "jitter", jitter, "kept", keep.size)
    np.savez_compressed(os.path.join(HERE, "rotated_reference_cases.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
