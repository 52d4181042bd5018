"""Panoptic-DeepLab's losses and bottom-up post-processing on the device (csrc/panoptic_deeplab.hip).

Surface of projects/Panoptic-DeepLab/panoptic_deeplab/post_processing.py (find_instance_center, group_pixels,
get_instance_segmentation, merge_semantic_and_instance, get_panoptic_segmentation: the reference's signatures and return
values) and of PanopticDeepLabInsEmbedHead.center_losses / offset_losses (panoptic_seg.py:536-561) fused with the
up-sampling that precedes them.  `panoptic_deeplab_postprocess` is the form the model calls: every launch of an image
is queued without a read-back, and the row counts come to the host once at the end."""
import torch

from .. import _lib as L

MAX_CENTERS = 1024      # PD_MAX_CENTERS of panoptic_deeplab.hip
MAX_CLASSES = 64        # PD_MAX_CLASSES
_LUTS = {}


# ---- losses ------------------------------------------------------------------------------------------------------------
def _rows(pred):
    """(pred as pitched channels-last rows, the pitch): a [:, :c] slice of a wider channels-last map is read in place."""
    n, c, hs, ws = pred.shape
    ld = pred.stride(3)
    if (c == 1 or pred.stride(1) == 1) and ld >= c and pred.stride(2) == ws * ld and pred.stride(0) == hs * ws * ld:
        return pred, ld
    rows = pred.permute(0, 2, 3, 1).contiguous()
    return rows.permute(0, 3, 1, 2), c


class _RegressionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weights, scale, kind):
        L.require_gpu(pred, target, weights)
        if pred.dtype != torch.float32:
            raise RuntimeError("panoptic_deeplab loss: float32 predictions, got %s" % pred.dtype)
        n, c, hs, ws = pred.shape
        if tuple(target.shape) != (n, c, hs * scale, ws * scale):
            raise RuntimeError("panoptic_deeplab loss: target %s is not %dx the prediction %s"
                               % (tuple(target.shape), scale, tuple(pred.shape)))
        if weights.numel() != n * hs * scale * ws * scale:
            raise RuntimeError("panoptic_deeplab loss: weights %s, one per pixel of %s expected"
                               % (tuple(weights.shape), tuple(target.shape)))
        pred, ld = _rows(pred)
        target = target.to(torch.float32).contiguous()
        weights = weights.to(torch.float32).contiguous()
        lib = L.lib()
        out = torch.empty(2, dtype=torch.float32, device=pred.device)
        wsb = torch.empty(lib.jtsm_pdl_loss_workspace_bytes(), dtype=torch.uint8, device=pred.device)
        L.note_bytes(4.0 * n * hs * ws * c + 4.0 * (target.numel() + weights.numel()))
        L.check(lib.jtsm_pdl_loss_forward_f32(L.ptr(pred), ld, c, L.ptr(target), L.ptr(weights), kind, L.ptr(out),
                                              L.ptr(wsb), n, hs, ws, scale, L.stream()), "pdl_loss_forward")
        ctx.save_for_backward(pred, target, weights, out)
        ctx.cfg = (ld, scale, kind)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        pred, target, weights, out = ctx.saved_tensors
        ld, scale, kind = ctx.cfg
        n, c, hs, ws = pred.shape
        dfull = torch.empty((n, hs, ws, ld), dtype=torch.float32, device=pred.device)
        g = g.to(torch.float32).contiguous()
        L.note_bytes(4.0 * n * hs * ws * c + 4.0 * (target.numel() + weights.numel()) + 4.0 * dfull.numel())
        L.check(L.lib().jtsm_pdl_loss_backward_f32(L.ptr(pred), ld, c, L.ptr(target), L.ptr(weights), kind, L.ptr(out),
                                                   L.ptr(g), L.ptr(dfull), n, hs, ws, scale, L.stream()),
                "pdl_loss_backward")
        if ld != c:
            from .conv import ZERO_PADDED
            setattr(dfull, ZERO_PADDED, True)   # (the kernel wrote zeros into channels c .. ld - 1)
        return dfull.permute(0, 3, 1, 2)[:, :c], None, None, None, None


def _scale_of(scale):
    if int(scale) != scale or scale < 1:
        raise ValueError("panoptic_deeplab loss: integer scale >= 1, got %r" % (scale,))
    return int(scale)


def center_loss(center, target, weights, scale):
    """sum((up(center) - target)^2 * weights) / sum(weights), 0 (and a zero gradient) where the weights sum to 0;
    up = F.interpolate(scale_factor=scale, mode="bilinear", align_corners=False), never materialised.
    center (N,1,h,w), target and weights (N,1,H,W)."""
    return _RegressionLoss.apply(center, target, weights, _scale_of(scale), 0)


def offset_loss(offset, target, weights, scale):
    """sum(|scale * up(offset) - target| * weights) / sum(weights): offset (N,2,h,w), target (N,2,H,W), weights
    (N,1,H,W) counted once per pixel."""
    return _RegressionLoss.apply(offset, target, weights, _scale_of(scale), 1)


# ---- post-processing ---------------------------------------------------------------------------------------------------
def thing_lut(thing_ids, num_classes, device):
    """(num_classes,) uint8 on the device, 1 at the thing classes; uploaded once per (ids, classes, device)."""
    ids = tuple(sorted(int(i) for i in thing_ids))
    key = (ids, int(num_classes), str(device))
    lut = _LUTS.get(key)
    if lut is None:
        host = torch.zeros(int(num_classes), dtype=torch.uint8)
        for i in ids:
            if 0 <= i < num_classes:
                host[i] = 1
        lut = _LUTS[key] = host.to(device)
    return lut


def _map2d(t, what, channels=1):
    if t.dim() != 3 or t.shape[0] != channels:
        raise ValueError("%s: a (%d,H,W) tensor is expected, got %s" % (what, channels, tuple(t.shape)))
    L.require_gpu(t)
    return t


def _find_centers(heat, threshold, nms_kernel, top_k):
    """heat (H,W) float32 -> centers (top_k,2) int32 (y, x; unused rows -1), count (1,) int32; nothing read back."""
    h, w = heat.shape
    if top_k is None:
        raise NotImplementedError("find_instance_center: top_k=None (every centre above the threshold) is not built")
    top_k, nms_kernel = int(top_k), int(nms_kernel)
    if not 1 <= top_k <= h * w:
        raise RuntimeError("find_instance_center: selected index k out of range (top_k=%d, %d pixels)" % (top_k, h * w))
    if top_k > MAX_CENTERS:
        raise ValueError("find_instance_center: top_k <= %d (got %d)" % (MAX_CENTERS, top_k))
    if nms_kernel < 1 or nms_kernel % 2 == 0 or nms_kernel > 31:
        raise ValueError("find_instance_center: nms_kernel must be odd and <= 31 (got %d)" % nms_kernel)
    lib = L.lib()
    centers = torch.empty((top_k, 2), dtype=torch.int32, device=heat.device)
    count = torch.empty(1, dtype=torch.int32, device=heat.device)
    wsb = torch.empty(lib.jtsm_pdl_centers_workspace_bytes(h, w), dtype=torch.uint8, device=heat.device)
    L.note_bytes(4.0 * h * w * 8)
    L.check(lib.jtsm_pdl_find_centers_f32(L.ptr(heat), h, w, float(threshold), nms_kernel, top_k, L.ptr(centers),
                                          L.ptr(count), L.ptr(wsb), L.stream()), "pdl_find_centers")
    return centers, count


@torch.no_grad()
def find_instance_center(center_heatmap, threshold=0.1, nms_kernel=3, top_k=None):
    """-> (K,2) int64 (y, x) in row-major order, K <= top_k - 1: the pixels above the threshold that equal their
    nms_kernel x nms_kernel maximum and lie strictly above max(the top_k-th largest such value, 0)."""
    heat = _map2d(center_heatmap, "center_heatmap").to(torch.float32)[0].contiguous()
    centers, count = _find_centers(heat, threshold, nms_kernel, top_k)
    return centers[:int(count.item())].to(torch.int64)


def _group(centers, count, offsets, sem=None, lut=None):
    _, h, w = offsets.shape
    ins = torch.empty((h, w), dtype=torch.int32, device=offsets.device)
    L.note_bytes(4.0 * h * w * (3 + (sem is not None)))
    L.check(L.lib().jtsm_pdl_group_pixels_f32(L.ptr(centers), L.ptr(count), centers.shape[0], L.ptr(offsets), L.ptr(sem),
                                              L.ptr(lut), 0 if lut is None else lut.numel(), L.ptr(ins), h, w,
                                              L.stream()), "pdl_group_pixels")
    return ins


def _center_table(center_points, device):
    pts = center_points.reshape(-1, 2)
    if pts.shape[0] > MAX_CENTERS:
        raise ValueError("group_pixels: at most %d centres (got %d)" % (MAX_CENTERS, pts.shape[0]))
    centers = pts.to(device=device, dtype=torch.int32).contiguous()
    count = torch.full((1,), pts.shape[0], dtype=torch.int32, device=device)
    return centers, count


@torch.no_grad()
def group_pixels(center_points, offsets):
    """-> (1,H,W) int64 in [1, K]: the centre nearest to (y + offset_y, x + offset_x), the lowest index on equal
    distances."""
    offsets = _map2d(offsets, "offsets", 2).to(torch.float32).contiguous()
    if center_points.shape[0] == 0:
        raise ValueError("group_pixels: no centre")
    centers, count = _center_table(center_points, offsets.device)
    return _group(centers, count, offsets).to(torch.int64).unsqueeze(0)


@torch.no_grad()
def get_instance_segmentation(sem_seg, center_heatmap, offsets, thing_seg, thing_ids, threshold=0.1, nms_kernel=3,
                              top_k=None):
    """-> ((1,H,W) instance ids, 0 outside `thing_seg`; (1,K,2) centres).  Without a centre every id is 0."""
    heat = _map2d(center_heatmap, "center_heatmap").to(torch.float32)[0].contiguous()
    offsets = _map2d(offsets, "offsets", 2).to(torch.float32).contiguous()
    centers, count = _find_centers(heat, threshold, nms_kernel, top_k)
    ids = _group(centers, count, offsets).unsqueeze(0)         # (all 0 when count is 0)
    found = centers[:int(count.item())].to(torch.int64).unsqueeze(0)
    return (thing_seg * ids).to(sem_seg.dtype), found


def _merge(sem, ins, thing_seg, lut, max_instances, label_divisor, stuff_area, void_label, id_offset, logits=None,
           heat=None):
    """sem, ins (H,W) int32 -> pan (H,W) int32, table (max_instances + C + 1, 5) int32 whose LAST row starts with num =
    {rows, thing rows} (one buffer, so that one copy brings rows and counts to the host), num (a view of that row),
    inst (max_instances, 8) float32 or None; nothing read back."""
    h, w = sem.shape
    c, dev, lib = lut.numel(), sem.device, L.lib()
    if id_offset not in (0, 1):
        raise ValueError("merge_semantic_and_instance: id_offset is 0 or 1")
    nbytes = lib.jtsm_pdl_merge_workspace_bytes(max_instances, c)
    if nbytes == 0:
        raise ValueError("merge_semantic_and_instance: 1 <= instances <= %d and 1 <= classes <= %d (got %d, %d)"
                         % (MAX_CENTERS, MAX_CLASSES, max_instances, c))
    pan = torch.empty((h, w), dtype=torch.int32, device=dev)
    table = torch.zeros((max_instances + c + 1, 5), dtype=torch.int32, device=dev)
    num = table[-1]
    inst = None if logits is None else torch.zeros((max_instances, 8), dtype=torch.float32, device=dev)
    wsb = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.note_bytes(4.0 * h * w * (5 + (0 if logits is None else 2 * c)))
    L.check(lib.jtsm_pdl_merge_f32(L.ptr(sem), L.ptr(ins), L.ptr(thing_seg), L.ptr(lut), L.ptr(logits), L.ptr(heat),
                                   max_instances, c, h, w, int(label_divisor), int(stuff_area), int(void_label),
                                   int(id_offset), L.ptr(pan), L.ptr(table), L.ptr(num), L.ptr(inst), L.ptr(wsb),
                                   L.stream()), "pdl_merge")
    return pan, table, num, inst


@torch.no_grad()
def merge_semantic_and_instance(sem_seg, ins_seg, semantic_thing_seg, label_divisor, thing_ids, stuff_area, void_label,
                                id_offset=0, num_classes=None, max_instances=None, return_table=False):
    """-> (1,H,W) panoptic map in sem_seg's dtype (class * label_divisor + per-class instance id; stuff classes with at
    least `stuff_area` pixels outside instances: class * label_divisor; void_label elsewhere; id_offset added to all).
    return_table: also the (n,5) int32 device rows {id, isthing, category_id, instance_id, area}.  num_classes /
    max_instances: bounds of the labels; read from the maps (one read-back each) where not given."""
    sem = _map2d(sem_seg, "sem_seg")
    ins = _map2d(ins_seg, "ins_seg")
    if num_classes is None:
        num_classes = int(sem.max().item()) + 1
    if max_instances is None:
        max_instances = max(int(ins.max().item()), 1)
    lut = thing_lut(thing_ids, num_classes, sem.device)
    thing = None
    if semantic_thing_seg is not None:
        thing = (semantic_thing_seg.reshape(sem.shape[1:]) > 0).to(torch.uint8).contiguous()
    pan, table, num, _ = _merge(sem[0].to(torch.int32).contiguous(), ins[0].to(torch.int32).contiguous(), thing, lut,
                                int(max_instances), label_divisor, stuff_area, void_label, id_offset)
    pan = pan.to(sem_seg.dtype).unsqueeze(0)
    if return_table:
        return pan, table[:int(num[0].item())]
    return pan


@torch.no_grad()
def get_panoptic_segmentation(sem_seg, center_heatmap, offsets, thing_ids, label_divisor, stuff_area, void_label,
                              threshold=0.1, nms_kernel=7, top_k=200, foreground_mask=None, num_classes=MAX_CLASSES):
    """-> (panoptic (1,H,W) int64, centers (1,K,2)); K is the one value read back.  sem_seg (1,H,W) labels below
    `num_classes`.  As in the reference, a class that receives `label_divisor` or more instances runs into the next
    class's ids: nothing checks it."""
    sem = _map2d(sem_seg, "sem_seg")[0].to(torch.int32).contiguous()
    heat = _map2d(center_heatmap, "center_heatmap").to(torch.float32)[0].contiguous()
    offsets = _map2d(offsets, "offsets", 2).to(torch.float32).contiguous()
    lut = thing_lut(thing_ids, num_classes, sem.device)
    thing = None
    if foreground_mask is not None:
        thing = (_map2d(foreground_mask, "foreground_mask")[0] > 0).to(torch.uint8).contiguous()
    centers, count = _find_centers(heat, threshold, nms_kernel, top_k)
    if thing is None:
        ins = _group(centers, count, offsets, sem, lut)
    else:
        ins = _group(centers, count, offsets) * thing.to(torch.int32)
    pan, _, _, _ = _merge(sem, ins, thing, lut, centers.shape[0], label_divisor, stuff_area, void_label, 0)
    k = int(count.item())
    return pan.to(torch.int64).unsqueeze(0), centers[:k].to(torch.int64).unsqueeze(0)


@torch.no_grad()
def panoptic_deeplab_postprocess(sem_logits, center, offset, thing_ids, label_divisor, stuff_area, threshold=0.1,
                                 nms_kernel=7, top_k=200, void_label=-1, id_offset=1):
    """The whole bottom-up post-processing of one image.  sem_logits (C,H,W), center (1,H,W), offset (2,H,W) float32.
    -> dict: "panoptic" (H,W) int32 (every id + id_offset: void is 0 with the defaults), "table" (n,5) int32 device rows
    {id, isthing, category_id, instance_id, area} (things in ascending instance order, then stuff by class), "rows" the
    same as host lists,
    "instances" (n_things,8) float32 device rows {x0, y0, x1, y1, semantic score, centre score, centre y, centre x},
    "sem_seg" (H,W) int32 arg-max, "centers" (top_k,2) int32 with "num_centers" (1,) on the device.  Every launch is
    queued first; the segment table (with its two row counts) is the only thing copied to the host, once, at the end."""
    L.require_gpu(sem_logits, center, offset)
    c, h, w = sem_logits.shape
    if c > MAX_CLASSES:
        raise ValueError("panoptic_deeplab_postprocess: at most %d classes (got %d)" % (MAX_CLASSES, c))
    logits = sem_logits.to(torch.float32).contiguous()
    heat = _map2d(center, "center_heatmap").to(torch.float32)[0].contiguous()
    offset = _map2d(offset, "offsets", 2).to(torch.float32).contiguous()
    if heat.shape != (h, w) or offset.shape[1:] != (h, w):
        raise ValueError("panoptic_deeplab_postprocess: maps of different sizes")
    lut = thing_lut(thing_ids, c, logits.device)
    sem = torch.empty((h, w), dtype=torch.int32, device=logits.device)
    L.note_bytes(4.0 * h * w * (c + 1))
    L.check(L.lib().jtsm_pdl_argmax_f32(L.ptr(logits), c, h, w, L.ptr(sem), L.stream()), "pdl_argmax")
    centers, count = _find_centers(heat, threshold, nms_kernel, top_k)
    ins = _group(centers, count, offset, sem, lut)
    pan, table, num, inst = _merge(sem, ins, None, lut, centers.shape[0], label_divisor, stuff_area, void_label,
                                   id_offset, logits, heat)
    host = table.cpu()                              # the one read-back: rows and counts together
    n, n_things = int(host[-1, 0]), int(host[-1, 1])
    return {"panoptic": pan, "table": table[:n], "rows": host[:n].tolist(), "instances": inst[:n_things],
            "sem_seg": sem, "centers": centers, "num_centers": count}
