"""Records tests/golden/pointrend_reference_cases.npz — in the build container only, where the reference tree exists.

    python tests/golden/make_pointrend_golden.py [/root/reference]

The reference's projects/PointRend/point_rend/point_features.py, point_head.py and mask_head.py are loaded BY FILE
PATH as submodules of an empty package of this file's own, behind stub modules (detectron2.layers / .structures /
.modeling / .utils.events / .utils.registry, fvcore.nn.weight_init) that hold a `cat`, a Boxes and a BitMasks with the
two attributes the functions touch, and an event storage that keeps what is put into it.  They run on the CPU in fp32 on
inputs that tests/pointrend_ref.py regenerates from a seed; nothing of the reference is copied.  Stored — seeds, shapes
and results only:

  gather cases   seed, the reference's rows (R * P, C) and image-space coordinates
  select cases   seed, the reference's point coordinates and the candidate indices it chose (as a sorted set)
  loss cases     seed, the reference's loss, gradient, soft targets and accuracy count
  subdiv cases   seed, the reference's up-sampled map (every `stride`-th pixel) and chosen cells (as a sorted set)
  meta           for each float quantity T = max |reference fp32 - fp64 restatement| over the cases at their FIRST seed
                 (gradients relative to the case's largest |gradient|) and bar = max(1e-6, 4 T) — the factor 4 is the
                 head-room the keypoint and rotated goldens give a kernel that sums in another order than the host;
                 select_margin / subdiv_margin = 2 bars of the ranked value: two candidates closer than that may swap.

Discrete results: a roi is ambiguous when the fp64 values of its last chosen and first rejected candidate lie within the
margin.  Up to 4 seeds are tried per case; the first is kept for which at most 5 % of the rois are ambiguous and the
reference's set equals the restatement's on all others (and, for the loss, the reference's accuracy count equals the
restatement's float32 one)."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pointrend_ref as PR  # noqa: E402

BASE_SEEDS = {"gather": 100, "select": 200, "loss": 300, "subdiv": 400}
TRIES = 4
CAP = 0.05


class _Storage(object):
    def __init__(self):
        self.scalars = {}

    def put_scalar(self, name, value):
        self.scalars[name] = value


STORAGE = _Storage()


def load_reference(root):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class Boxes(object):
        def __init__(self, tensor):
            self.tensor = tensor

        @staticmethod
        def cat(boxes):
            return Boxes(torch.cat([b.tensor for b in boxes]))

    class BitMasks(object):
        def __init__(self, tensor):
            self.tensor = tensor
            self.image_size = tuple(tensor.shape[1:])

    class Registry(object):
        def __init__(self, name):
            self.name = name

        def register(self):
            return lambda cls: cls

    def cat(tensors, dim=0):
        return tensors[0] if len(tensors) == 1 else torch.cat(tensors, dim)

    stub("fvcore")
    stub("fvcore.nn")
    stub("fvcore.nn.weight_init")
    sys.modules["fvcore.nn"].weight_init = sys.modules["fvcore.nn.weight_init"]
    stub("detectron2")
    stub("detectron2.layers", cat=cat, ShapeSpec=object, Conv2d=torch.nn.Conv2d,
         interpolate=torch.nn.functional.interpolate)
    stub("detectron2.structures", Boxes=Boxes, BitMasks=BitMasks)
    stub("detectron2.utils")
    stub("detectron2.utils.events", get_event_storage=lambda: STORAGE)
    stub("detectron2.utils.registry", Registry=Registry)
    stub("detectron2.modeling", ROI_MASK_HEAD_REGISTRY=Registry("m"), BaseMaskRCNNHead=torch.nn.Module)
    stub("detectron2.modeling.roi_heads")
    stub("detectron2.modeling.roi_heads.mask_head", mask_rcnn_inference=None, mask_rcnn_loss=None)
    pkg = types.ModuleType("ref_point_rend")
    pkg.__path__ = [os.path.join(root, "projects", "PointRend", "point_rend")]
    sys.modules["ref_point_rend"] = pkg
    out = {n: importlib.import_module("ref_point_rend." + n) for n in ("point_features", "point_head", "mask_head")}
    out["Boxes"], out["BitMasks"] = Boxes, BitMasks
    return out


class _Inst(object):
    def __init__(self, n, **fields):
        self.n = n
        self.__dict__.update(fields)

    def __len__(self):
        return self.n


def ref_gather(ref, name, seed, grads=False):
    fine, scales, coarse, boxes, roi_image, points = PR.gather_inputs(name, seed)
    pf = ref["point_features"]
    counts = np.bincount(roi_image, minlength=fine[0].shape[0])
    split = np.split(boxes, np.cumsum(counts)[:-1])
    ft = [torch.from_numpy(f).requires_grad_(grads) for f in fine]
    ct = torch.from_numpy(coarse).requires_grad_(grads) if coarse is not None else None
    feats, coords = pf.point_sample_fine_grained_features(ft, scales, [ref["Boxes"](torch.from_numpy(b)) for b in split],
                                                          torch.from_numpy(points))
    parts = [feats]
    if ct is not None:
        parts.append(pf.point_sample(ct, torch.from_numpy(points), align_corners=False))
    rows = torch.cat(parts, 1).permute(0, 2, 1).reshape(points.shape[0] * points.shape[1], -1)
    if not grads:
        return rows.detach().numpy(), coords.numpy()
    g = np.random.RandomState(seed + 7).randn(*rows.shape).astype(np.float32)
    rows.backward(torch.from_numpy(g))
    return g, [f.grad.numpy() for f in ft], (ct.grad.numpy() if ct is not None else None)


def ref_select(ref, name, seed):
    coarse, classes, cand, rand, P, U = PR.select_inputs(name, seed)
    R, C, S, P, k, beta = PR.SELECT_CASES[name]
    mh, pf = ref["mask_head"], ref["point_features"]
    torch.manual_seed(seed)
    coords = pf.get_uncertain_point_coords_with_randomness(
        torch.from_numpy(coarse), lambda logits: mh.calculate_uncertainty(logits, torch.from_numpy(classes)), P, k,
        beta).numpy()
    chosen = np.zeros((R, U), np.int64)
    for r in range(R):
        for j in range(U):
            hit = np.nonzero((cand[r] == coords[r, j]).all(1))[0]
            assert len(hit) >= 1, (name, r, j)
            chosen[r, j] = hit[0]
    u32 = mh.calculate_uncertainty(pf.point_sample(torch.from_numpy(coarse), torch.from_numpy(cand), align_corners=False),
                                   torch.from_numpy(classes))[:, 0].numpy()
    return coords, np.sort(chosen, 1), u32


def ref_loss(ref, name, seed):
    logits, classes, masks, roi_image, matched, coords, P = PR.loss_inputs(name, seed)
    R, C = roi_image.shape[0], logits.shape[1]
    x = torch.from_numpy(logits).view(R, P, C).permute(0, 2, 1).contiguous().requires_grad_(True)
    inst, targets = [], []
    for n, m in enumerate(masks):
        rows = np.nonzero(roi_image == n)[0]
        if m is None or len(rows) == 0:
            inst.append(_Inst(0))
            continue
        bits = torch.from_numpy(m[matched[rows]]).to(torch.bool)
        inst.append(_Inst(len(rows), gt_masks=ref["BitMasks"](bits), gt_classes=torch.from_numpy(classes[rows])))
        h, w = m.shape[1:]
        targets.append(ref["point_features"].point_sample(
            bits.to(torch.float32).unsqueeze(1), torch.from_numpy(coords[rows]) / torch.tensor([w, h], dtype=torch.float),
            align_corners=False).squeeze(1))
    loss = ref["point_head"].roi_mask_point_loss(x, inst, torch.from_numpy(coords))
    loss.backward()
    acc = STORAGE.scalars["point_rend/accuracy"]
    grad = x.grad.permute(0, 2, 1).reshape(R * P, C).numpy()
    return float(loss.detach()), grad, torch.cat(targets).reshape(-1).numpy(), int(round(acc * R * P))


def step_points(H, W, N, last=False):
    """The reference's skip rule for the step H x W -> 2H x 2W: 0 = only up-sample."""
    return 0 if (N >= 4 * (2 * H) * (2 * W) and not last) else N


def ref_subdiv(ref, name, seed):
    m, N = PR.subdiv_inputs(name, seed)
    up = torch.nn.functional.interpolate(torch.from_numpy(m)[:, None], scale_factor=2, mode="bilinear",
                                         align_corners=False)
    n = step_points(m.shape[1], m.shape[2], N)
    if n == 0:
        return up[:, 0].numpy(), None
    u = ref["mask_head"].calculate_uncertainty(up, None)
    idx, _ = ref["point_features"].get_uncertain_point_coords_on_grid(u, n)
    return up[:, 0].numpy(), np.sort(idx.numpy(), 1)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    ref = load_reference(root)
    torch.set_num_threads(8)
    out, T = {}, {k: 0.0 for k in ("gather", "coords", "target", "loss", "grad", "loss_grad", "up", "select_u")}

    # ---- pass 1: the float bars, every case at its first seed
    for i, name in enumerate(PR.GATHER_CASES):
        seed = BASE_SEEDS["gather"] + 10 * i
        fine, scales, coarse, boxes, roi_image, points = PR.gather_inputs(name, seed)
        rows, coords = ref_gather(ref, name, seed)
        mine, mine_c = PR.gather(fine, scales, coarse, boxes, roi_image, points)
        T["gather"] = max(T["gather"], float(np.abs(rows - mine).max()))
        T["coords"] = max(T["coords"], float(np.abs(coords - mine_c).max()))
        out["gather_%s_seed" % name] = np.int64(seed)
        out["gather_%s_rows" % name] = rows
        out["gather_%s_coords" % name] = coords
        if name in ("one", "two"):
            g, gf, gc = ref_gather(ref, name, seed, grads=True)
            mf, mc = PR.gather_adjoint(g.astype(np.float64), [f.shape for f in fine], scales,
                                       None if coarse is None else coarse.shape, boxes, roi_image, points)
            for a, b in list(zip(gf, mf)) + ([(gc, mc)] if gc is not None else []):
                T["grad"] = max(T["grad"], float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)))
        print("gather %s seed %d: rows %s" % (name, seed, rows.shape))
    for i, name in enumerate(PR.SELECT_CASES):
        seed = BASE_SEEDS["select"] + 10 * i
        coarse, classes, cand, rand, P, U = PR.select_inputs(name, seed)
        _, _, u32 = ref_select(ref, name, seed)
        T["select_u"] = max(T["select_u"], float(np.abs(u32 - PR.uncertainties(coarse, classes, cand)).max()))
    for i, name in enumerate(PR.LOSS_CASES):
        seed = BASE_SEEDS["loss"] + 10 * i
        args = PR.loss_inputs(name, seed)
        loss, grad, targets, _ = ref_loss(ref, name, seed)
        ml, mg, mt, _ = PR.point_loss(*args)
        T["loss"] = max(T["loss"], abs(loss - ml))
        T["loss_grad"] = max(T["loss_grad"], float(np.abs(grad - mg).max() / np.abs(mg).max()))
        T["target"] = max(T["target"], float(np.abs(targets - mt).max()))
    for i, name in enumerate(PR.SUBDIV_CASES):
        seed = BASE_SEEDS["subdiv"] + 10 * i
        m, N = PR.subdiv_inputs(name, seed)
        up, _ = ref_subdiv(ref, name, seed)
        T["up"] = max(T["up"], float(np.abs(up - PR.upsample2(m)).max()))
    bars = {k: max(1e-6, 4 * v) for k, v in T.items()}
    margins = {"select": 2 * bars["select_u"], "subdiv": 2 * bars["up"]}

    # ---- pass 2: the discrete cases, the first seed of up to four that the reference alone settles
    for i, name in enumerate(PR.SELECT_CASES):
        for t in range(TRIES):
            seed = BASE_SEEDS["select"] + 10 * i + t
            coarse, classes, cand, rand, P, U = PR.select_inputs(name, seed)
            coords, chosen, _ = ref_select(ref, name, seed)
            _, mine, u = PR.select(coarse, classes, cand, rand, U)
            amb = PR.ambiguous(u, U, margins["select"])
            same = all(np.array_equal(np.sort(mine[r]), chosen[r]) for r in range(len(u)) if not amb[r])
            if amb.mean() <= CAP and same:
                break
        else:
            raise SystemExit("select %s: no seed within the cap" % name)
        out["select_%s_seed" % name] = np.int64(seed)
        out["select_%s_coords" % name] = coords
        out["select_%s_chosen" % name] = chosen
        print("select %s seed %d: %d ambiguous of %d" % (name, seed, int(amb.sum()), len(amb)))
    for i, name in enumerate(PR.LOSS_CASES):
        for t in range(TRIES):
            seed = BASE_SEEDS["loss"] + 10 * i + t
            loss, grad, targets, acc = ref_loss(ref, name, seed)
            if PR.point_loss(*PR.loss_inputs(name, seed))[3] == acc:
                break
        else:
            raise SystemExit("loss %s: no seed on which the accuracy counts agree" % name)
        one = int((targets >= 1.0).sum())
        near = int(((targets < 1.0) & (targets > 1.0 - 1e-6)).sum())
        out["loss_%s_seed" % name] = np.int64(seed)
        out["loss_%s_loss" % name] = np.float64(loss)
        out["loss_%s_grad" % name] = grad
        out["loss_%s_targets" % name] = targets
        out["loss_%s_accurate" % name] = np.int64(acc)
        print("loss %s seed %d: loss %.6f, %d of %d accurate, %d targets of 1.0, %d just below" % (
            name, seed, loss, acc, len(targets), one, near))
    for i, name in enumerate(PR.SUBDIV_CASES):
        for t in range(TRIES):
            seed = BASE_SEEDS["subdiv"] + 10 * i + t
            m, N = PR.subdiv_inputs(name, seed)
            up, chosen = ref_subdiv(ref, name, seed)
            n = step_points(m.shape[1], m.shape[2], N)
            if n == 0:
                amb = np.zeros(len(m), bool)
                break
            _, mine, _ = PR.subdivide(m, n)
            amb = PR.ambiguous(-np.abs(PR.upsample2(m)).reshape(len(m), -1), mine.shape[1], margins["subdiv"])
            same = all(np.array_equal(np.sort(mine[r]), chosen[r]) for r in range(len(m)) if not amb[r])
            if amb.mean() <= CAP and same:
                break
        else:
            raise SystemExit("subdiv %s: no seed within the cap" % name)
        stride = 4 if up.shape[-1] > 64 else 1
        out["subdiv_%s_seed" % name] = np.int64(seed)
        out["subdiv_%s_up" % name] = up[:, ::stride, ::stride]
        out["subdiv_%s_stride" % name] = np.int64(stride)
        if chosen is not None:
            out["subdiv_%s_chosen" % name] = chosen.astype(np.int32)
        print("subdiv %s seed %d: %d ambiguous of %d, %s cells" % (
            name, seed, int(amb.sum()), len(amb), "no" if chosen is None else chosen.shape[1]))

    meta = {"T_" + k: v for k, v in T.items()}
    meta.update({k + "_bar": v for k, v in bars.items()})
    meta.update({k + "_margin": v for k, v in margins.items()})
    meta["ambiguous_cap"] = CAP
    out["meta_keys"] = np.array(sorted(meta))
    out["meta_values"] = np.array([meta[k] for k in sorted(meta)], np.float64)
    for k in sorted(meta):
        print("%-16s %.3e" % (k, meta[k]))
    path = os.path.join(HERE, "pointrend_reference_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
