"""One OICR + MIST training step of the shipped `reg_all_mist` configuration (tests/golden/configs/
oicr_mist_WSR_18_DC5_1x.yaml): B=2 synthetic 3x1024x1024 images, 2000 clustered proposals each, 20 classes, four
regressing refinement branches.  Prints one JSON line: ms/step, img/s, and from one more step under the library's
per-call hipEvents the time inside the mining launches (jtsm_mine_top_p_f32, with the row log-sum-exp in front of it)
and the labelling launches (jtsm_match_label_f32), summed over the four branches.  --torch-mining also times the same
mining written in torch device ops (tests/mist_ref.py on GPU tensors) on the last step's inputs and counts its host
synchronisations per step.

    python tools/bench_oicr.py [--steps N] [--warmup W] [--torch-mining]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_mining(aux, boxes, counts, class_ids, repeats=5):
    """get_pgt_mist of the four branches in torch device ops, per image as the reference runs it; the NMS is the
    library's batched_nms, whose keep count comes to the host as torchvision's keep list does.  -> (ms per step, host syncs)."""
    from jtsm_amd.layers.postprocess import batched_nms_device

    def one_pass():
        syncs = 0
        lo = 0
        for i, n in enumerate(counts):
            ids = class_ids[i]
            for k in range(4):
                if k == 0:
                    sc, bpc = aux["mil_scores"][lo:lo + n], boxes[lo:lo + n][:, None, :].expand(n, 20, 4)
                else:
                    from jtsm_amd.modeling.box_regression import Box2BoxTransform
                    sc = torch.softmax(aux["logits_r%d" % (k - 1)][lo:lo + n], dim=-1)
                    bpc = Box2BoxTransform(weights=(10.0, 10.0, 5.0, 5.0)).apply_deltas(
                        aux["deltas_r%d" % (k - 1)][lo:lo + n], boxes[lo:lo + n]).view(n, 20, 4)
                t = max(int(n * 0.15), 1)
                top, idx = torch.topk(torch.index_select(sc, 1, ids), t, dim=0)
                bx = torch.gather(torch.index_select(bpc, 1, ids), 0, idx[:, :, None].expand(t, ids.numel(), 4))
                m = t * ids.numel()
                keep, num, _ = batched_nms_device(bx.reshape(-1, 4), top.reshape(-1),
                                                  torch.zeros(m, dtype=torch.int64, device=sc.device), 0.2, 1, m, 0)
                keep = keep[:int(num)]                       # the keep list's length comes to the host
                syncs += 1
                _ = bx.reshape(-1, 4)[keep], top.reshape(-1)[keep]
            lo += n
        return syncs

    one_pass()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        syncs = one_pass()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeats, syncs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-mining", action="store_true")
    a = ap.parse_args()
    from jtsm_amd import _lib as L
    from jtsm_amd.config import add_wsl_config, get_cfg
    from jtsm_amd.modeling import build_model
    from model_util import to_batched_inputs
    from oracle import model as OM

    B, R = 2, 2000
    cfg = get_cfg()
    add_wsl_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "tests", "golden", "configs", "oicr_mist_WSR_18_DC5_1x.yaml"))
    cfg.MODEL.DEVICE = "cuda"
    model = build_model(cfg)
    with torch.no_grad():
        model.backbone.stem.conv1.weight.mul_(1.0 / 64)
    model.train()
    batch = OM.synthetic_batch(1234, B=B, size=1024, R=R, sp_block=32, n_stuff=1, nt=20, ns=2, cluster=1.0, objects=40)
    inputs = to_batched_inputs(batch)
    for x in inputs:
        x["image"] = x["image"].to(torch.uint8).cuda()
        x["proposals"] = x["proposals"].to("cuda")
        x["instances"] = x["instances"].to("cuda")
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1e-7, momentum=0.9)

    def step():
        opt.zero_grad(set_to_none=True)
        losses = model(inputs)
        sum(losses.values()).backward()
        opt.step()
        return losses

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        losses = step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    L.TIMING = []
    try:
        step()
        torch.cuda.synchronize()
        spans = [(n, span.ms()) for n, span, _ in L.TIMING]
    finally:
        L.TIMING = None
    total = lambda *names: round(sum(t for n, t in spans if n in names), 4)  # noqa: E731
    aux = model.roi_heads.aux
    out = {"workload": "OICR + MIST WSR-18 DC5, %d x 3x1024x1024, %d proposals each, 20 classes, 4 branches" % (B, R),
           "ms_per_step": round(ms, 3), "img_per_s": round(1000.0 * B / ms, 2),
           "mining_ms": total("jtsm_mine_top_p_f32", "jtsm_row_lse_f32"), "labelling_ms": total("jtsm_match_label_f32"),
           "mining_host_syncs_per_step": 0,
           "survivors_per_branch": [int(aux["pgt_num_r%d" % k].sum()) for k in range(4)],
           "losses": {k: round(float(v), 6) for k, v in losses.items()}}
    if a.torch_mining:
        boxes = torch.cat([x["proposals"].proposal_boxes.tensor for x in inputs])
        ids = [torch.nonzero(r)[:, 0] for r in model.roi_heads.gt_classes_img_oh]
        t_ms, syncs = torch_mining(aux, boxes, [R] * B, ids)
        out["torch_mining_ms"], out["torch_mining_host_syncs_per_step"] = round(t_ms, 4), syncs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
