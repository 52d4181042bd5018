"""Keypoint R-CNN operators (jtsm_amd/csrc/keypoint.hip) behind ctypes, and the two autograd functions.

keypoint_targets     <- _keypoints_to_heatmap      (detectron2/structures/keypoints.py:84-140)
keypoint_loss        <- keypoint_rcnn_loss         (detectron2/modeling/roi_heads/keypoint_head.py:40-96)
keypoint_decode      <- heatmaps_to_keypoints      (detectron2/structures/keypoints.py:143-217)
keypoint_upsample    <- the pixel shuffle of score_lowres written as a 3x3 convolution + the x2 bilinear
                        (keypoint_head.py:247-272); transposed4x4_as_conv3x3 builds that convolution's weight

Logits are plain contiguous (R, K, S, S) — one (roi, keypoint) map is one row — unlike the channels-last maps of the
rest of the package."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib as L


def _f32(t):
    return t.to(torch.float32).contiguous()


def keypoint_targets(keypoints, rois, heatmap_size):
    """keypoints (N, K, 3), rois (N, 4) -> int32 targets (N, K), uint8 valid (N, K); nothing read back."""
    L.require_gpu(keypoints, rois)
    n, k = int(keypoints.shape[0]), int(keypoints.shape[1])
    if tuple(keypoints.shape) != (n, k, 3) or tuple(rois.shape) != (n, 4):
        raise RuntimeError("keypoint_targets: keypoints %s / rois %s" % (tuple(keypoints.shape), tuple(rois.shape)))
    keypoints, rois = _f32(keypoints), _f32(rois)
    targets = torch.empty((n, k), dtype=torch.int32, device=rois.device)
    valid = torch.empty((n, k), dtype=torch.uint8, device=rois.device)
    L.check(L.lib().jtsm_keypoint_targets_f32(L.ptr(keypoints), L.ptr(rois), n, k, int(heatmap_size), L.ptr(targets),
                                              L.ptr(valid), L.stream()), "keypoint_targets")
    return targets, valid


class _KeypointLoss(Function):
    @staticmethod
    def forward(ctx, logits, targets, valid, normalizer):
        L.require_gpu(logits, targets, valid)
        n, k, s, s2 = logits.shape
        if s != s2 or logits.dtype != torch.float32 or targets.numel() != n * k or valid.numel() != n * k:
            raise RuntimeError("keypoint_loss: logits %s %s / targets %s / valid %s" % (
                tuple(logits.shape), logits.dtype, tuple(targets.shape), tuple(valid.shape)))
        logits = logits.contiguous()
        targets, valid = targets.to(torch.int32).contiguous(), valid.to(torch.uint8).contiguous()
        lib = L.lib()
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        ws = torch.empty(lib.jtsm_keypoint_loss_workspace_bytes(n, k), dtype=torch.uint8, device=logits.device)
        L.check(lib.jtsm_keypoint_loss_forward_f32(L.ptr(logits), L.ptr(targets), L.ptr(valid), n, k, s,
                                                   float(normalizer), L.ptr(loss), L.ptr(ws), L.stream()),
                "keypoint_loss_forward")
        ctx.save_for_backward(logits, targets, valid, ws)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logits, targets, valid, ws = ctx.saved_tensors
        n, k, s, _ = logits.shape
        d = torch.empty_like(logits)
        g = _f32(g)
        L.check(L.lib().jtsm_keypoint_loss_backward_f32(L.ptr(logits), L.ptr(targets), L.ptr(valid), n, k, s, L.ptr(g),
                                                        L.ptr(ws), L.ptr(d), L.stream()), "keypoint_loss_backward")
        return d, None, None, None


def keypoint_loss(logits, targets, valid, normalizer=None):
    """sum over valid rows of cross_entropy(logits.view(N * K, S * S)[row], targets[row]) / normalizer; None (or <= 0)
    divides by the number of valid rows; no valid row gives 0 with a zero gradient.  One launch pair each way."""
    return _KeypointLoss.apply(logits, targets, valid, 0.0 if normalizer is None else float(normalizer))


def keypoint_decode(maps, rois):
    """maps (R, K, S, S), rois (R, 4) -> (R, K, 4) = x, y, logit, score: one launch, no host read-back."""
    L.require_gpu(maps, rois)
    r, k, s, s2 = maps.shape
    if s != s2 or tuple(rois.shape) != (r, 4):
        raise RuntimeError("keypoint_decode: maps %s / rois %s" % (tuple(maps.shape), tuple(rois.shape)))
    maps, rois = _f32(maps.detach()), _f32(rois.detach())
    out = torch.empty((r, k, 4), dtype=torch.float32, device=maps.device)
    L.check(L.lib().jtsm_keypoint_decode_f32(L.ptr(maps), L.ptr(rois), r, k, s, L.ptr(out), L.stream()),
            "keypoint_decode")
    return out


class _KeypointUpsample(Function):
    @staticmethod
    def forward(ctx, z, k):
        L.require_gpu(z)
        r, cp, h, w = z.shape
        if z.dtype != torch.float32 or cp < 4 * k:
            raise RuntimeError("keypoint_upsample: z %s %s for %d keypoints" % (tuple(z.shape), z.dtype, k))
        zl = z.permute(0, 2, 3, 1).contiguous()                     # (R, H, W, Cp): a view of a channels-last map
        out = torch.empty((r, k, 4 * h, 4 * w), dtype=torch.float32, device=z.device)
        L.check(L.lib().jtsm_keypoint_upsample_forward_f32(L.ptr(zl), r, k, h, w, cp, L.ptr(out), L.stream()),
                "keypoint_upsample_forward")
        ctx.cfg = (r, k, h, w, cp)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        r, k, h, w, cp = ctx.cfg
        g = _f32(g)
        dz = torch.empty((r, h, w, cp), dtype=torch.float32, device=g.device)
        L.check(L.lib().jtsm_keypoint_upsample_backward_f32(L.ptr(g), r, k, h, w, cp, L.ptr(dz), L.stream()),
                "keypoint_upsample_backward")
        return dz.permute(0, 3, 1, 2), None


def keypoint_upsample(z, num_keypoints):
    """z (R, Cp, H, W) channels-last, parity-major channels (py * 2 + px) * K + k -> contiguous (R, K, 4H, 4W) logits:
    pixel shuffle to 2H x 2W and F.interpolate(scale_factor=2, "bilinear", align_corners=False) in one pass."""
    return _KeypointUpsample.apply(z, int(num_keypoints))


# tap of the 4-wide transposed kernel read by slot d = -1, 0, +1 of the 3x3 kernel, per output parity (4 = no tap):
# row 2i = tap 1 of input i + tap 3 of input i - 1; row 2i + 1 = tap 0 of input i + 1 + tap 2 of input i
_TAPS = ((3, 1, 4), (4, 2, 0))


def transposed4x4_as_conv3x3(weight, bias, multiple=8):
    """The (in, K, 4, 4) weight and (K,) bias of ConvTranspose2d(in, K, 4, stride 2, padding 1) as the (4K padded, in,
    3, 3) weight and bias of the 3x3 / padding-1 convolution whose parity-major channels are the transposed
    convolution's four output phases.  Differentiable torch ops on 4 x K x in x 9 floats; rows zero-padded to a
    multiple of `multiple` so that the weight gradient stays on the plane kernels (layers/wrappers.py)."""
    k = weight.shape[1]
    wp = torch.nn.functional.pad(weight.permute(1, 0, 2, 3), (0, 1, 0, 1))            # (K, in, 5, 5), tap 4 = 0

    def pick(t, dim, taps):       # (slices and a stack: no index tensor to copy to the device)
        return torch.stack([t.select(dim, i) for i in taps], dim)

    w3 = torch.cat([pick(pick(wp, 2, _TAPS[py]), 3, _TAPS[px]) for py in (0, 1) for px in (0, 1)])
    b3 = bias.repeat(4)
    extra = -(4 * k) % multiple
    if extra:
        w3 = torch.cat([w3, w3.new_zeros((extra,) + tuple(w3.shape[1:]))])
        b3 = torch.cat([b3, b3.new_zeros(extra)])
    return w3.contiguous(memory_format=torch.channels_last), b3
