"""RetinaNet operators (jtsm_amd/csrc/retinanet.hip) behind ctypes, and the loss as an autograd function.

retinanet_label_anchors  <- RetinaNet.label_anchors + Matcher          (detectron2/modeling/meta_arch/retinanet.py:353-397,
                                                                       modeling/matcher.py:61-126)
retinanet_loss           <- RetinaNet.losses                           (retinanet.py:287-351)
retinanet_candidates     <- the per-level part of inference_single_image (retinanet.py:453-481)

The head's per-level outputs are read where the convolutions wrote them: a level is either the head's own
(N, A * K, H, W) channels-last map — a channel slice of a padded map included, as conv2d_padded returns for bbox_pred —
or the reference's (N, H * W * A, K) view of it.  Either is described to the kernels by a cell count, a cell stride and
an image stride; only a tensor that is neither (not unit-stride along K) is copied."""
import ctypes as C
import math

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib as L

SCALE_CLAMP = math.log(1000.0 / 16)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _cells(t, K):
    """One level -> (tensor kept alive, A, cells, image stride, cell stride), strides in floats."""
    if t.dtype != torch.float32 or t.dim() not in (3, 4):
        raise RuntimeError("retinanet: a level must be float32 (N, A*K, H, W) or (N, HWA, K), got %s %s"
                           % (tuple(t.shape), t.dtype))
    if t.dim() == 3:
        if t.shape[2] != K:
            raise RuntimeError("retinanet: level %s for K = %d" % (tuple(t.shape), K))
        v = t.unsqueeze(1)                          # (N, 1, HWA, K): cells of one row
    else:
        if t.shape[1] % K:
            raise RuntimeError("retinanet: level %s for K = %d" % (tuple(t.shape), K))
        v = t.permute(0, 2, 3, 1)                   # (N, H, W, A*K)
    n, h, w, c = v.shape
    cs = v.stride(2) if w > 1 else (v.stride(1) if h > 1 else c)
    ok = (c == 1 or v.stride(3) == 1) and cs >= c and (h == 1 or w == 1 or v.stride(1) == w * cs)
    img = v.stride(0) if n > 1 else h * w * cs
    ok = ok and img >= (h * w - 1) * cs + c
    if not ok:
        t = t.contiguous() if t.dim() == 3 else t.contiguous(memory_format=torch.channels_last)
        cs, img = c, h * w * c
    return t, c // K, h * w, img, cs


class _Table(object):
    """The kernels' level table for two lists of per-level tensors."""

    def __init__(self, logits, deltas, K):
        if len(logits) != len(deltas) or not 1 <= len(logits) <= 8:
            raise RuntimeError("retinanet: %d logit levels, %d delta levels (1..8, equal)" % (len(logits), len(deltas)))
        L.require_gpu(*logits)
        L.require_gpu(*deltas)
        self.K, self.N = int(K), int(logits[0].shape[0])
        x = [_cells(t, self.K) for t in logits]
        d = [_cells(t, 4) for t in deltas]
        self.A = x[0][1]
        rows, geom = 0, []
        for (_, ax, cx, ix, sx), (_, ad, cd, idd, sd), t in zip(x, d, logits):
            if ax != self.A or ad != self.A or cx != cd or t.shape[0] != self.N:
                raise RuntimeError("retinanet: levels disagree on N, A or H x W")
            geom += [cx, rows, ix, sx, idd, sd]
            rows += cx * self.A
        self.R, self.levels = rows, len(x)
        self.logits, self.deltas = [e[0] for e in x], [e[0] for e in d]
        self.geom_list = geom
        self.geom = (C.c_int64 * len(geom))(*geom)

    @staticmethod
    def pointers(tensors):
        return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def gradient_maps(self):
        """Per level: zero-free buffers of the inputs' cell strides, and their views in the inputs' shapes."""
        bufs, views, geom = ([], []), ([], []), []
        for l in range(self.levels):
            cells, off, _, sx, _, sd = self.geom_list[6 * l:6 * l + 6]
            geom += [cells, off, cells * sx, sx, cells * sd, sd]
            for which, (src, stride, k) in enumerate(((self.logits[l], sx, self.K), (self.deltas[l], sd, 4))):
                buf = torch.empty((self.N, cells, stride), dtype=torch.float32, device=src.device)
                bufs[which].append(buf)
                if src.dim() == 3:
                    views[which].append(buf[:, :, :k])
                else:
                    h, w = src.shape[2], src.shape[3]
                    views[which].append(buf.view(self.N, h, w, stride)[..., :self.A * k].permute(0, 3, 1, 2))
        return bufs, views, (C.c_int64 * len(geom))(*geom)


def _weights(w):
    if len(w) != 4:
        raise RuntimeError("retinanet: four Box2BoxTransform weights, got %r" % (w,))
    return (C.c_float * 4)(*[float(v) for v in w])


@torch.no_grad()
def retinanet_label_anchors(anchors, gt_boxes, gt_classes, gt_counts, num_classes, thresholds=(0.4, 0.5),
                            labels=(0, -1, 1)):
    """anchors (R, 4); gt_boxes (G, 4) / gt_classes (G) concatenated over the N images, gt_counts their N lengths
    (host ints).  -> labels (N, R) int32 in {-1 ignore, 0 .. K - 1, K background}, matched (N, R) int32 (gt row within
    the image), gt_offsets (N + 1) int32 and num_pos (1,) int32, all on the device; nothing is read back."""
    L.require_gpu(anchors, gt_boxes, gt_classes)
    counts = [int(c) for c in gt_counts]
    n, r, g = len(counts), int(anchors.shape[0]), int(gt_boxes.shape[0])
    if tuple(anchors.shape) != (r, 4) or tuple(gt_boxes.shape) != (g, 4) or gt_classes.numel() != g or sum(counts) != g:
        raise RuntimeError("retinanet_label_anchors: anchors %s / gt_boxes %s / gt_classes %s / counts %r" % (
            tuple(anchors.shape), tuple(gt_boxes.shape), tuple(gt_classes.shape), counts))
    if len(labels) != len(thresholds) + 1:
        raise RuntimeError("retinanet_label_anchors: %d thresholds need %d labels" % (len(thresholds), len(thresholds) + 1))
    dev = anchors.device
    anchors, gt_boxes = anchors.to(torch.float32).contiguous(), gt_boxes.to(torch.float32).contiguous()
    gt_classes = gt_classes.to(torch.int64).contiguous()
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    offsets = torch.tensor(offs, dtype=torch.int32).to(dev)
    out = torch.empty((n, r), dtype=torch.int32, device=dev)
    matched = torch.empty((n, r), dtype=torch.int32, device=dev)
    num_pos = torch.empty(1, dtype=torch.int32, device=dev)
    lib = L.lib()
    ws = _ws(lib.jtsm_retinanet_label_workspace_bytes(g), dev)
    thr = (C.c_float * max(len(thresholds), 1))(*[float(t) for t in thresholds])
    lab = (C.c_int32 * len(labels))(*[int(v) for v in labels])
    L.check(lib.jtsm_retinanet_label_anchors_f32(L.ptr(anchors), r, L.ptr(gt_boxes), L.ptr(offsets), L.ptr(gt_classes),
                                                 n, g, thr, lab, len(thresholds), int(num_classes), L.ptr(out),
                                                 L.ptr(matched), L.ptr(num_pos), L.ptr(ws), L.stream()),
            "retinanet_label_anchors")
    return out, matched, offsets, num_pos


class _RetinaNetLoss(Function):
    @staticmethod
    def forward(ctx, levels, K, labels, matched, anchors, gt_boxes, gt_offsets, num_pos, normalizer, cfg, *tensors):
        logits, deltas = tensors[:levels], tensors[levels:]
        T = _Table(logits, deltas, K)
        alpha, gamma, beta, weights, momentum, training = cfg
        L.require_gpu(labels, matched, anchors, gt_boxes, gt_offsets, num_pos, normalizer)
        if tuple(labels.shape) != (T.N, T.R) or tuple(matched.shape) != (T.N, T.R) or tuple(anchors.shape) != (T.R, 4) \
                or labels.dtype != torch.int32 or matched.dtype != torch.int32 or gt_offsets.dtype != torch.int32 \
                or gt_offsets.numel() != T.N + 1 or normalizer.dtype != torch.float64 or normalizer.numel() != 1:
            raise RuntimeError("retinanet_loss: labels %s %s / matched %s / anchors %s / normalizer %s for N = %d, R = %d"
                               % (tuple(labels.shape), labels.dtype, tuple(matched.shape), tuple(anchors.shape),
                                  normalizer.dtype, T.N, T.R))
        labels, matched = labels.contiguous(), matched.contiguous()
        anchors, gt_boxes = anchors.to(torch.float32).contiguous(), gt_boxes.to(torch.float32).contiguous()
        dev = labels.device
        lib = L.lib()
        out = torch.empty(2, dtype=torch.float32, device=dev)
        ws = _ws(lib.jtsm_retinanet_loss_workspace_bytes(), dev)
        w = _weights(weights)
        L.check(lib.jtsm_retinanet_loss_forward_f32(
            T.pointers(T.logits), T.pointers(T.deltas), T.geom, T.levels, T.N, T.A, T.K, T.R, L.ptr(labels),
            L.ptr(matched), L.ptr(anchors), L.ptr(gt_boxes), L.ptr(gt_offsets), float(alpha), float(gamma), float(beta),
            w, L.ptr(num_pos), L.ptr(normalizer), float(momentum), int(bool(training)), out.data_ptr(),
            out.data_ptr() + 4, L.ptr(ws), L.stream()), "retinanet_loss_forward")
        ctx.table, ctx.cfg = T, (float(alpha), float(gamma), float(beta), w)
        ctx.save_for_backward(labels, matched, anchors, gt_boxes, gt_offsets, ws)
        return out[0], out[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_box):
        labels, matched, anchors, gt_boxes, gt_offsets, ws = ctx.saved_tensors
        T = ctx.table
        alpha, gamma, beta, w = ctx.cfg
        g = torch.stack([g_cls.to(torch.float32).reshape(()), g_box.to(torch.float32).reshape(())])
        bufs, views, geom = T.gradient_maps()
        L.check(L.lib().jtsm_retinanet_loss_backward_f32(
            T.pointers(T.logits), T.pointers(T.deltas), T.geom, T.levels, T.N, T.A, T.K, T.R, L.ptr(labels),
            L.ptr(matched), L.ptr(anchors), L.ptr(gt_boxes), L.ptr(gt_offsets), alpha, gamma, beta, w, g.data_ptr(),
            g.data_ptr() + 4, L.ptr(ws), T.pointers(bufs[0]), T.pointers(bufs[1]), geom, L.stream()),
            "retinanet_loss_backward")
        return (None,) * 10 + tuple(views[0]) + tuple(views[1])


def retinanet_loss(pred_logits, pred_anchor_deltas, labels, matched, anchors, gt_boxes, gt_offsets, num_pos,
                   normalizer, num_classes, alpha=0.25, gamma=2.0, beta=0.1, weights=(1.0, 1.0, 1.0, 1.0), momentum=0.9,
                   training=True):
    """The two sums of RetinaNet.losses over per-level logits and deltas, divided by the EMA normaliser ->
    (loss_cls, loss_box_reg).  labels / matched / gt_offsets / num_pos are retinanet_label_anchors' outputs;
    `normalizer` is a float64 device tensor of one element that a training call updates in place
    (<- momentum * normalizer + (1 - momentum) * max(num_pos, 1)) before dividing by its fp32 value."""
    pred_logits, pred_anchor_deltas = list(pred_logits), list(pred_anchor_deltas)
    cfg = (alpha, gamma, beta, tuple(weights), momentum, training)
    return _RetinaNetLoss.apply(len(pred_logits), int(num_classes), labels, matched, anchors, gt_boxes, gt_offsets,
                                num_pos, normalizer, cfg, *(pred_logits + pred_anchor_deltas))


def retinanet_candidates_workspace_bytes(n, levels, topk):
    return int(L.lib().jtsm_retinanet_candidates_workspace_bytes(int(n), int(levels), int(topk)))


@torch.no_grad()
def retinanet_candidates(pred_logits, pred_anchor_deltas, anchors, num_classes, score_thresh, topk,
                         weights=(1.0, 1.0, 1.0, 1.0), scale_clamp=SCALE_CLAMP, return_rows=False):
    """Per (image, level): the `topk` best of sigmoid(logit) > score_thresh, equal fp32 scores by lower flat index
    anchor * K + class first, decoded by apply_deltas.  -> boxes (N, L * topk, 4), scores (N, L * topk), classes
    (N, L * topk) int64 with -1 in unused slots, counts (N, L) int32 (and with return_rows the anchor's row within
    its level, (N, L * topk) int32); level-major within an image, one launch
    sequence for the batch and nothing read back."""
    T = _Table([t.detach() for t in pred_logits], [t.detach() for t in pred_anchor_deltas], num_classes)
    L.require_gpu(anchors)
    if tuple(anchors.shape) != (T.R, 4):
        raise RuntimeError("retinanet_candidates: anchors %s for R = %d" % (tuple(anchors.shape), T.R))
    anchors = anchors.to(torch.float32).contiguous()
    dev, topk = anchors.device, int(topk)
    slots = T.levels * topk
    boxes = torch.empty((T.N, slots, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((T.N, slots), dtype=torch.float32, device=dev)
    classes = torch.empty((T.N, slots), dtype=torch.int64, device=dev)
    rows = torch.empty((T.N, slots), dtype=torch.int32, device=dev) if return_rows else None
    counts = torch.empty((T.N, T.levels), dtype=torch.int32, device=dev)
    lib = L.lib()
    ws = _ws(lib.jtsm_retinanet_candidates_workspace_bytes(T.N, T.levels, topk), dev)
    L.check(lib.jtsm_retinanet_candidates_f32(
        T.pointers(T.logits), T.pointers(T.deltas), T.geom, T.levels, T.N, T.A, T.K, T.R, L.ptr(anchors),
        _weights(weights), float(scale_clamp), float(score_thresh), topk, L.ptr(boxes), L.ptr(scores), L.ptr(classes),
        L.ptr(rows), L.ptr(counts), L.ptr(ws), ws.numel(), L.stream()), "retinanet_candidates")
    return (boxes, scores, classes, counts, rows) if return_rows else (boxes, scores, classes, counts)
