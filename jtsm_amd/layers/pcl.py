"""PCL on the device (jtsm_amd/csrc/pcl.hip): proposal clustering and the PCL loss of one refinement branch.

pcl_cluster  <- PCL(boxes, cls_prob, im_labels, cls_prob_new)
                (projects/WSL/wsl/modeling/roi_heads/third_party/pcl.py:24-200), for every image of the batch
pcl_loss     <- PCLOutputs.pcl_loss (projects/WSL/wsl/modeling/roi_heads/fast_rcnn_oicr.py:917-936): soft-max,
                clustering from the previous branch's probabilities, wsl.layers.pcl_loss (pcl_loss.py:9-93)

Nothing is read back to the host: launch sizes come from the number of images and the largest number of proposals
of one image, both host integers the caller already has.  For B images the loss is the mean of the per-image losses
(the reference asserts one image per process, pcl.py:90).  The backward multiplies by the incoming gradient (the
reference ignores it, pcl_loss.py:55-90; identical when it is 1)."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .wsl_losses import _rowmajor

MAX_PC = 5           # clusters per present class (cfg_TRAIN_MAX_PC_NUM)
MAX_ROWS = 8192      # proposals of one image the centre search holds


def pcl_softmax(logits):
    """(R, K+1) soft-max of the rows of `logits` (any leading dimension), dense."""
    L.require_gpu(logits)
    z, ld = _rowmajor(logits)
    R, ncls = z.shape
    probs = torch.empty((R, ncls), dtype=torch.float32, device=z.device)
    L.check(L.lib().jtsm_pcl_softmax_f32(L.ptr(z), ld, ncls, R, L.ptr(probs), L.stream()), "pcl_softmax")
    return probs


def pcl_cluster(boxes, offsets, max_rows, prev_probs, labels, probs):
    """The cluster tables of every image.

    boxes (R, 4) float32; offsets (B+1,) int32 device tensor; max_rows: host int, at least the rows of any image;
    prev_probs (R, K) or (R, K+1) with the background first (that column is dropped, pcl.py:29-30); labels (B, K) 0/1;
    probs (R, K+1) this branch's probabilities, background first.
    -> dict: row_label (R) int32 in [0, K], row_assign (R) int32 (-1 = background), row_weight (R) float32,
       pc_int (B, 5K, 3) int32 = (label, count, centre row), pc_flt (B, 5K, 3) float32 = (centre score, summed weight,
       pc_prob), pc_num (B) int32."""
    L.require_gpu(boxes, offsets, prev_probs, labels, probs)
    B, K = labels.shape
    R = boxes.shape[0]
    if probs.shape[1] != K + 1 or prev_probs.shape[1] not in (K, K + 1):
        raise RuntimeError("pcl_cluster: %d classes, probabilities %s, previous probabilities %s" % (
            K, tuple(probs.shape), tuple(prev_probs.shape)))
    if offsets.numel() != B + 1 or offsets.dtype != torch.int32:
        raise RuntimeError("pcl_cluster: offsets must be int32 (images + 1,)")
    if max_rows > MAX_ROWS:
        raise RuntimeError("pcl_cluster: at most %d proposals per image, got %d" % (MAX_ROWS, max_rows))
    boxes = boxes.to(torch.float32).contiguous()
    prev, ld_prev = _rowmajor(prev_probs)
    p, ld_p = _rowmajor(probs)
    labels = labels.to(torch.float32).contiguous()
    dev = boxes.device
    out = {"row_label": torch.empty(R, dtype=torch.int32, device=dev),
           "row_assign": torch.empty(R, dtype=torch.int32, device=dev),
           "row_weight": torch.empty(R, dtype=torch.float32, device=dev),
           "pc_int": torch.empty((B, MAX_PC * K, 3), dtype=torch.int32, device=dev),
           "pc_flt": torch.empty((B, MAX_PC * K, 3), dtype=torch.float32, device=dev),
           "pc_num": torch.empty(B, dtype=torch.int32, device=dev)}
    lib = L.lib()
    ws = torch.empty(max(lib.jtsm_pcl_cluster_workspace_bytes(B, max_rows), 16), dtype=torch.uint8, device=dev)
    L.check(lib.jtsm_pcl_cluster_f32(
        L.ptr(boxes), L.ptr(offsets), B, max_rows, R, L.ptr(prev), ld_prev, prev.shape[1] - K, L.ptr(labels), K,
        L.ptr(p), ld_p, L.ptr(out["row_label"]), L.ptr(out["row_assign"]), L.ptr(out["row_weight"]),
        L.ptr(out["pc_int"]), L.ptr(out["pc_flt"]), L.ptr(out["pc_num"]), L.ptr(ws), L.stream()), "pcl_cluster")
    return out


class _PCLLoss(Function):
    @staticmethod
    def forward(ctx, logits, probs, offsets, labels, row_label, row_assign, row_weight, pc_int, pc_flt, pc_num):
        L.require_gpu(logits, probs, offsets)
        z, ld = _rowmajor(logits)
        B, K = labels.shape
        lib = L.lib()
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        ws = torch.empty(lib.jtsm_pcl_loss_workspace_bytes(B), dtype=torch.uint8, device=z.device)
        L.check(lib.jtsm_pcl_loss_forward_f32(
            L.ptr(probs), K + 1, L.ptr(offsets), B, K, L.ptr(row_label), L.ptr(row_weight), L.ptr(pc_int),
            L.ptr(pc_flt), L.ptr(pc_num), L.ptr(loss), L.ptr(ws), L.stream()), "pcl_loss_forward")
        ctx.save_for_backward(z, offsets, row_label, row_assign, row_weight, pc_int, pc_flt)
        ctx.cfg = (ld, K, B)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss):
        z, offsets, row_label, row_assign, row_weight, pc_int, pc_flt = ctx.saved_tensors
        ld, K, B = ctx.cfg
        R = z.shape[0]
        dz = torch.empty((R, K + 1), dtype=torch.float32, device=z.device)
        g = g_loss.to(torch.float32).contiguous()
        L.check(L.lib().jtsm_pcl_loss_backward_f32(
            L.ptr(z), ld, K, L.ptr(offsets), B, R, L.ptr(row_label), L.ptr(row_assign), L.ptr(row_weight),
            L.ptr(pc_int), L.ptr(pc_flt), L.ptr(g), L.ptr(dz), K + 1, L.stream()), "pcl_loss_backward")
        return (dz,) + (None,) * 9


def pcl_loss(logits, boxes, offsets, max_rows, prev_probs, labels, tables=None):
    """(loss, probs, tables) of one refinement branch: logits (R, K+1) with the background in column 0; the other
    arguments as pcl_cluster's.  `probs` (the branch's soft-max, no gradient) is what the next branch clusters from;
    `tables` are the cluster tables the loss used (given ones are used as they are: tests)."""
    with torch.no_grad():
        probs = pcl_softmax(logits)
        t = tables if tables is not None else pcl_cluster(boxes, offsets, int(max_rows), prev_probs, labels, probs)
    loss = _PCLLoss.apply(logits, probs, offsets, labels, t["row_label"], t["row_assign"], t["row_weight"], t["pc_int"],
                          t["pc_flt"], t["pc_num"])
    return loss, probs, t
