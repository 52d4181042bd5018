"""Records tests/golden/cmil_reference_cases.npz — build container only (it compiles the reference's own
projects/WSL/wsl/layers/csrc/ROIMerge/ROIMerge_cpu.cpp and ROILabel/ROILabel_cpu.cpp where they lie, into a temporary
directory; nothing of them is copied).

    python tests/golden/make_cmil_golden.py

The two sources include TH/TH.h, which the installed torch no longer ships: an EMPTY header of that name in the
temporary directory stands in (they use nothing of it).  Per ROIMerge case the file holds the inputs (S, boxes, C, D,
cur_iter, max_epoch, size_epoch) and the reference's MC, MD, I, IC and backward (GC, GD for a recorded upstream); per
ROILabel case the inputs (S, boxes, L, CW) and RL, RW.  J and U, which the reference is handed, are this repository's
pairwise_iou of the boxes.  Only cases are kept whose result does not hang on what the reference leaves open: no equal
scores (std::sort), no IoU within 1e-6 of lambda or of a threshold, and — ROILabel — neither cap binding, so that the
visiting order it draws from srand(time(0)) does not matter."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
CSRC = "/root/reference/projects/WSL/wsl/layers/csrc"
OUT = os.path.join(HERE, "cmil_reference_cases.npz")
MERGE_CASES, LABEL_CASES, K = 8, 6, 20

BINDING = """
#include <torch/extension.h>
#include "ROIMerge/ROIMerge.h"
#include "ROILabel/ROILabel.h"
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("roi_merge_forward", &wsl::ROIMerge_forward_cpu);
  m.def("roi_merge_backward", &wsl::ROIMerge_backward_cpu);
  m.def("roi_label_forward", &wsl::ROILabel_forward_cpu);
}
"""


def reference_module(build_dir):
    from torch.utils.cpp_extension import load

    os.makedirs(os.path.join(build_dir, "stub", "TH"), exist_ok=True)
    open(os.path.join(build_dir, "stub", "TH", "TH.h"), "w").close()          # the empty stand-in
    binding = os.path.join(build_dir, "binding.cpp")
    with open(binding, "w") as f:
        f.write(BINDING)
    return load(name="cmil_reference", build_directory=build_dir, verbose=False,
                sources=[binding, os.path.join(CSRC, "ROIMerge", "ROIMerge_cpu.cpp"),
                         os.path.join(CSRC, "ROILabel", "ROILabel_cpu.cpp")],
                extra_include_paths=[os.path.join(build_dir, "stub"), CSRC], extra_cflags=["-O1", "-w"])


def main():
    import cmil_ref as CR

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        ref = reference_module(tmp)
        kept, seed = 0, 0
        while kept < MERGE_CASES:
            seed += 1
            rng = np.random.default_rng(seed)
            n = int(rng.choice([1, 39, 41, 150, 199, 201, 260, 333]))
            cur_iter, size_epoch, max_epoch = int(rng.choice([0, 40, 700, 2500, 9000, 50000])), 1250, 40
            lam = CR.getlambda(cur_iter, size_epoch, max_epoch)
            case = CR.merge_case(seed, [n], int(rng.choice([3, 20])), lam)
            if case is None:
                continue
            J = CR.pairwise_iou(case["boxes"], case["boxes"])
            P = torch.tensor([0, 1000, cur_iter, max_epoch, size_epoch, 0, 0, 0], dtype=torch.int32)
            t = torch.from_numpy
            MC, MD, I, IC, _ = ref.roi_merge_forward(t(case["S"])[:, None], t(J), t(case["C"]), t(case["D"]), P)
            g = np.random.default_rng(seed + 1000).normal(0, 1, (2,) + tuple(MC.shape)).astype(np.float32)
            GC, GD = ref.roi_merge_backward(t(case["C"]), t(case["D"]), t(g[0]), t(g[1]), I, IC)
            pre = "merge%d_" % kept
            for name, v in (("S", case["S"]), ("boxes", case["boxes"]), ("C", case["C"]), ("D", case["D"]),
                            ("iters", np.array([cur_iter, max_epoch, size_epoch], np.int32)), ("MC", MC.numpy()),
                            ("MD", MD.numpy()), ("I", I.numpy()), ("IC", IC.numpy()), ("gM", g), ("GC", GC.numpy()),
                            ("GD", GD.numpy())):
                out[pre + name] = v
            kept += 1
        kept, seed = 0, 100
        while kept < LABEL_CASES:
            seed += 1
            rng = np.random.default_rng(seed)
            n = int(rng.choice([1, 12, 40, 64, 90]))
            case = CR.label_case(seed, [n], int(rng.integers(1, 5)), K=K, mode="raw")
            if case is None:
                continue
            ids = case["classes"][0, :case["counts"][0]]
            mine = CR.roi_label_image(case["S"], case["boxes"], ids, case["CW"][0], case["perm"], num_classes=K)
            sb = case["boxes"][mine["seed_rows"]]
            if mine["eligible"][0] > 32 or mine["eligible"][1] > 96 or len(mine["seed_rows"]) < len(ids):
                continue                                                          # a cap binds, or the rows ran out
            if not CR.far_from(CR.pairwise_iou(case["boxes"], sb), case["boxes"], sb, [0.6, 0.4, 0.1]):
                continue
            L = np.zeros((1, K), np.float32)
            L[0, ids] = 1
            P = torch.tensor([0.6, 0.4, 0.1, 32, 96, 1, 0, 0, 1000, 0, 0, 0, 0, 0], dtype=torch.float32)
            t = torch.from_numpy
            U = CR.pairwise_iou(case["boxes"], case["boxes"])
            RL, RW, _ = ref.roi_label_forward(t(case["S"]), t(U), t(L), t(case["CW"][0].copy()), P)
            pre = "label%d_" % kept
            for name, v in (("S", case["S"]), ("boxes", case["boxes"]), ("L", L), ("CW", case["CW"][0]),
                            ("RL", RL.numpy()), ("RW", RW.numpy())):
                out[pre + name] = v
            kept += 1
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d ROIMerge and %d ROILabel cases, %d bytes" % (OUT, MERGE_CASES, LABEL_CASES, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
