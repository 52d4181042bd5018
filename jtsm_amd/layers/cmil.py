"""C-MIL's two operators (jtsm_amd/csrc/cmil.hip): ROIMerge and ROILabel of projects/WSL/wsl/layers/roi_merge.py and
roi_label.py, whose kernels the reference has as host code only (csrc/ROIMerge/ROIMerge_cpu.cpp,
csrc/ROILabel/ROILabel_cpu.cpp).  Both take every image of the step in one library call, form the IoUs they need from
the boxes (no R x R matrix) and read nothing back: the number of cliques an image keeps stays on the device as
`merged_offsets`, which `mil_loss` takes as its bag offsets."""
import math

import numpy as np
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .wsl_losses import _rowmajor


def getlambda(cur_iter, size_epoch, max_epoch):
    """ROIMerge_cpu.cpp:11-17 at iter = cur_iter / size_epoch: evaluated in double, rounded once to float32.  0 at
    iteration 0, 1 at iteration max_epoch * size_epoch."""
    low = 0.01
    it = float(cur_iter) / float(size_epoch)
    lam = (math.log(it + low) - math.log(low)) / (math.log(float(max_epoch) + low) - math.log(low))
    return float(np.float32(lam))


class _ROIMerge(Function):
    @staticmethod
    def forward(ctx, S, boxes, C, D, bag_offsets, lam, max_bag_rows):
        L.require_gpu(S, boxes, C, D, bag_offsets)
        assert bag_offsets.dtype == torch.int32
        c, ldc = _rowmajor(C)
        d, ldd = _rowmajor(D)
        R, K = c.shape
        B = bag_offsets.numel() - 1
        S = S.to(torch.float32).reshape(-1).contiguous()
        boxes = boxes.to(torch.float32).contiguous()
        assert S.numel() == R and tuple(boxes.shape) == (R, 4) and tuple(d.shape) == (R, K)
        dev = c.device
        MC = torch.empty((R, K), dtype=torch.float32, device=dev)
        MD = torch.empty((R, K), dtype=torch.float32, device=dev)
        words = torch.empty(2 * R + B + 1, dtype=torch.int32, device=dev)       # one allocation: I, IC, merged_offsets
        I, IC, merged_offsets = words[:R], words[R:2 * R], words[2 * R:]
        lib = L.lib()
        ws = torch.empty(lib.jtsm_roi_merge_workspace_bytes(B, R), dtype=torch.uint8, device=dev)
        L.check(lib.jtsm_roi_merge_forward_f32(L.ptr(S), L.ptr(boxes), L.ptr(c), ldc, L.ptr(d), ldd, K,
                                               L.ptr(bag_offsets), B, R, int(max_bag_rows), float(lam), L.ptr(MC),
                                               L.ptr(MD), L.ptr(I), L.ptr(IC), L.ptr(merged_offsets), L.ptr(ws),
                                               L.stream()), "roi_merge_forward")
        ctx.save_for_backward(I, IC)
        ctx.mark_non_differentiable(I, IC, merged_offsets)
        return MC, MD, I, IC, merged_offsets

    @staticmethod
    @once_differentiable
    def backward(ctx, gMC, gMD, _gi, _gic, _go):
        I, IC = ctx.saved_tensors
        R = I.numel()
        if gMC is None and gMD is None:
            return None, None, None, None, None, None, None
        ref = gMC if gMC is not None else gMD
        gMC = torch.zeros_like(ref) if gMC is None else gMC
        gMD = torch.zeros_like(ref) if gMD is None else gMD
        gc, ldc = _rowmajor(gMC)
        gd, ldd = _rowmajor(gMD)
        if ldc != ldd:
            gc, gd = gc.contiguous(), gd.contiguous()
            ldc = gc.shape[1]
        K = gc.shape[1]
        dC = torch.empty((R, K), dtype=torch.float32, device=gc.device)
        dD = torch.empty_like(dC)
        L.check(L.lib().jtsm_roi_merge_backward_f32(L.ptr(gc), L.ptr(gd), ldc, K, L.ptr(I), L.ptr(IC), R, L.ptr(dC),
                                                    L.ptr(dD), K, L.stream()), "roi_merge_backward")
        return None, None, dC, dD, None, None, None


def roi_merge(S, boxes, C, D, bag_offsets, lam, max_bag_rows=None):
    """S (R,) the rows' summed MIL scores, boxes (R, 4), C / D (R, K), bag_offsets (B+1,) int32 device tensors; lam: the
    host float of `getlambda`; max_bag_rows: host int upper bound of an image's rows.
    -> (MC (R, K), MD (R, K), I (R,) int32, IC (R,) int32, merged_offsets (B+1,) int32): the clique means, compacted
    over the batch — image b's cliques are rows [merged_offsets[b], merged_offsets[b+1]), rows at and behind
    merged_offsets[B] are zero —, every row's merged row and every merged row's member count.  Gradient flows from MC /
    MD to C / D only."""
    if max_bag_rows is None:
        max_bag_rows = int(C.shape[0])
    return _ROIMerge.apply(S, boxes, C, D, bag_offsets, float(lam), int(max_bag_rows))


def draw_perm(rows_per_image, device, generator=None):
    """The visiting order ROILabel draws (the reference: std::random_shuffle under srand(time(0))): per image a
    torch.randperm of its rows, on the device, concatenated; int32."""
    perms = [torch.randperm(int(n), device=device, generator=generator, dtype=torch.int32) for n in rows_per_image]
    return torch.cat(perms) if perms else torch.zeros(0, dtype=torch.int32, device=device)


@torch.no_grad()
def roi_label(S, boxes, bag_offsets, classes, counts, img_probs, rows_per_image=None, perm=None, generator=None, lse=None,
              fg=0.6, bg_hi=0.4, bg_lo=0.1, num_pos=32, num_neg=96, top_k=1, num_classes=None):
    """S (R, ld) class scores — raw scores, or logits with lse (R,) (score = exp(S - lse), as mine_top1 takes them) —,
    boxes (R, 4), bag_offsets (B+1,), classes (B, G), counts (B,) int32 device tensors, img_probs (B, K) the weights CW
    (None: a seed's score).  perm (R,) int32: for every image a permutation of range(rows) at its rows' positions;
    drawn with `draw_perm(rows_per_image, device, generator)` when not given.
    -> dict(labels (R,) int32, weights (R,), seed_rows (B, G * top_k) int32, seed_num (B,) int32, perm)."""
    if not fg >= bg_hi:
        raise ValueError("roi_label: fg_thresh %r is below bg_thresh_hi %r: a proposal could be both" % (fg, bg_hi))
    L.require_gpu(S, boxes, lse, img_probs)
    assert S.dim() == 2 and S.stride(1) == 1 and S.dtype == torch.float32
    assert classes.dtype == counts.dtype == bag_offsets.dtype == torch.int32
    B, G = classes.shape
    R, dev = S.shape[0], S.device
    if num_classes is None:
        num_classes = img_probs.shape[1]
    if perm is None:
        perm = draw_perm(rows_per_image, dev, generator)
    assert perm.dtype == torch.int32 and perm.numel() == R
    perm = perm.contiguous()
    boxes = boxes.to(torch.float32).contiguous()
    if img_probs is not None:
        img_probs = img_probs.to(torch.float32).contiguous()
    P = G * int(top_k)
    words = torch.empty(2 * R + B * P + B, dtype=torch.int32, device=dev)       # one allocation carved into the outputs
    out = dict(labels=words[:R], weights=words[R:2 * R].view(torch.float32),
               seed_rows=words[2 * R:2 * R + B * P].view(B, P), seed_num=words[2 * R + B * P:], perm=perm)
    L.check(L.lib().jtsm_roi_label_f32(
        L.ptr(S), S.stride(0), L.ptr(lse), L.ptr(boxes), L.ptr(bag_offsets), L.ptr(classes), L.ptr(counts), B, G,
        L.ptr(img_probs), img_probs.shape[1] if img_probs is not None else 0, L.ptr(perm), float(fg), float(bg_hi),
        float(bg_lo), int(num_pos), int(num_neg), int(top_k), int(num_classes), L.ptr(out["labels"]),
        L.ptr(out["weights"]), L.ptr(out["seed_rows"]), L.ptr(out["seed_num"]), L.stream()), "roi_label")
    return out


class ROIMerge(nn.Module):
    """wsl.layers.ROIMerge(debug_info, display, max_epoch, size_epoch) without its int Parameter P: the iteration count
    is the plain host int `cur_iter`, advanced by every training forward and settable on resume; the running clique
    statistics it prints every `display` iterations are not kept."""

    def __init__(self, display, max_epoch, size_epoch):
        super().__init__()
        self.display, self.max_epoch, self.size_epoch = int(display), int(max_epoch), int(size_epoch)
        self.cur_iter = 0

    @property
    def lam(self):
        return getlambda(self.cur_iter, self.size_epoch, self.max_epoch)

    def forward(self, S, boxes, C, D, bag_offsets, max_bag_rows=None):
        out = roi_merge(S, boxes, C, D, bag_offsets, self.lam, max_bag_rows)
        if self.training:
            self.cur_iter += 1
        return out

    def extra_repr(self):
        return "display=%d, max_epoch=%d, size_epoch=%d" % (self.display, self.max_epoch, self.size_epoch)


class ROILabel(nn.Module):
    """wsl.layers.ROILabel(fg_thresh, bg_thresh_hi, bg_thresh_lo, num_pos, num_neg, top_k, ...) without its statistics."""

    def __init__(self, fg, bg_hi, bg_lo, num_pos, num_neg, top_k):
        super().__init__()
        if not fg >= bg_hi:
            raise ValueError("ROILabel: fg_thresh %r is below bg_thresh_hi %r: a proposal could be both" % (fg, bg_hi))
        self.fg, self.bg_hi, self.bg_lo = float(fg), float(bg_hi), float(bg_lo)
        self.num_pos, self.num_neg, self.top_k = int(num_pos), int(num_neg), int(top_k)

    def forward(self, S, boxes, bag_offsets, classes, counts, img_probs, rows_per_image=None, perm=None, generator=None,
                lse=None, num_classes=None):
        return roi_label(S, boxes, bag_offsets, classes, counts, img_probs, rows_per_image, perm, generator, lse,
                         self.fg, self.bg_hi, self.bg_lo, self.num_pos, self.num_neg, self.top_k, num_classes)

    def extra_repr(self):
        return "fg=%g, bg_hi=%g, bg_lo=%g, num_pos=%d, num_neg=%d, top_k=%d" % (
            self.fg, self.bg_hi, self.bg_lo, self.num_pos, self.num_neg, self.top_k)
