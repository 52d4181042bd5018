"""MIST pseudo-ground-truth mining (jtsm_amd/csrc/mist.hip): get_pgt_mist of
projects/WSL/wsl/modeling/roi_heads/roi_heads_oicr.py:550-591 — per image and present class the top fraction of the
proposals by class score, one class-agnostic NMS at IoU 0.2 over all of them — for every image of the step in one
library call that reads nothing back.  The survivor list is padded; `match_label` takes it as it is."""
import torch

from .. import _lib as L


def top_p_counts(rows_per_image, top_pro, device):
    """-> (top_t (B,) int32 on `device`, t_max): max(int(rows * top_pro), 1) per image, the reference's expression
    (roi_heads_oicr.py:727) evaluated in Python floats as it is there."""
    top_ts = [max(int(num_pred * top_pro), 1) for num_pred in rows_per_image]
    return torch.tensor(top_ts, dtype=torch.int32).to(device, non_blocking=True), max(top_ts)


@torch.no_grad()
def mine_top_p(scores, proposals, bag_offsets, classes, counts, top_t, t_max, lse=None, deltas=None, decode=None,
               iou_thresh=0.2):
    """scores (R, ld) with optional lse (R,) (score = exp(scores - lse)) and deltas (R, 4K), proposals (R, 4),
    bag_offsets (B+1,), classes (B, G), counts (B,), top_t (B,) int32 device tensors; t_max: host int >= max(top_t)
    (top_p_counts gives both).  decode: the candidate's box is the proposal decoded with zero deltas rather than the
    proposal row when there are no deltas — the default whenever lse is given, i.e. for a refinement branch without
    regression, as the reference computes it.
    -> dict(boxes (B,P,4), classes (B,P) int32, scores (B,P), weights (B,P) = scores, rows (B,P) int32, num (B,) int32),
    P = t_max * G, survivors in NMS visiting order, zeros behind them."""
    L.require_gpu(scores, proposals, lse, deltas)
    assert scores.stride(1) == 1 and (deltas is None or deltas.stride(1) == 1)
    assert classes.dtype == counts.dtype == top_t.dtype == bag_offsets.dtype == torch.int32
    B, G = classes.shape
    P = int(t_max) * G
    dev = scores.device
    if decode is None:
        decode = lse is not None
    words = torch.empty(8 * B * P + B, dtype=torch.int32, device=dev)       # one allocation carved into the outputs
    n = B * P
    out = dict(boxes=words[:4 * n].view(torch.float32).view(B, P, 4), classes=words[4 * n:5 * n].view(B, P),
               scores=words[5 * n:6 * n].view(torch.float32).view(B, P),
               weights=words[6 * n:7 * n].view(torch.float32).view(B, P), rows=words[7 * n:8 * n].view(B, P),
               num=words[8 * n:])
    lib = L.lib()
    ws = torch.empty(lib.jtsm_mine_top_p_workspace_bytes(B, G, int(t_max)), dtype=torch.uint8, device=dev)
    proposals = proposals.contiguous()
    L.check(lib.jtsm_mine_top_p_f32(
        L.ptr(scores), scores.stride(0), L.ptr(lse), L.ptr(proposals), L.ptr(deltas),
        deltas.stride(0) if deltas is not None else 0, int(bool(decode)), L.ptr(bag_offsets), L.ptr(classes),
        L.ptr(counts), L.ptr(top_t), B, G, int(t_max), iou_thresh, L.ptr(out["boxes"]), L.ptr(out["classes"]),
        L.ptr(out["scores"]), L.ptr(out["weights"]), L.ptr(out["rows"]), L.ptr(out["num"]), L.ptr(ws), L.stream()),
        "mine_top_p")
    return out
