"""FrozenBatchNorm2d / get_norm — the API of detectron2/layers/batch_norm.py:14-153 (class name, buffer names and
state-dict versioning are fixed by the checkpoints; everything else is this repo's).

On the MI355X path a frozen norm behind a convolution never runs as its own pass: `Conv2d` asks for `scale_bias()`
— the affine map y = x * scale + bias with scale = weight / sqrt(running_var + eps), bias = bias - running_mean * scale
— and the contraction's epilogue applies it.  The pair is memoised on the buffers' version counters, so a frozen layer
costs no launch per step.  `forward` exists for stand-alone use and applies the same map with tensor ops.
"""
import torch
from torch import nn

_STATS = ("weight", "bias", "running_mean", "running_var")


class FrozenBatchNorm2d(nn.Module):
    _version = 3          # state-dict layout version, as the reference writes it into checkpoints' metadata

    def __init__(self, num_features, eps=1e-5):
        super().__init__()
        self.num_features, self.eps = num_features, eps
        start = {"weight": 1.0, "bias": 0.0, "running_mean": 0.0, "running_var": 1.0 - eps}
        for name in _STATS:
            self.register_buffer(name, torch.full((num_features,), start[name]))
        self._memo = None

    # ---- the affine map -------------------------------------------------------------------------------------------
    def _stamp(self):
        return tuple(getattr(self, n)._version for n in _STATS) + (self.weight.data_ptr(), str(self.weight.device))

    def scale_bias(self):
        """(scale, bias), each (C,), recomputed only after one of the four buffers has been written or moved."""
        stamp = self._stamp()
        if self._memo is None or self._memo[0] != stamp:
            with torch.no_grad():
                scale = self.weight * torch.rsqrt(self.running_var + self.eps)
                self._memo = (stamp, scale, self.bias - self.running_mean * scale)
        return self._memo[1], self._memo[2]

    def forward(self, x):
        scale, bias = (t.to(x.dtype).view(1, -1, 1, 1) for t in self.scale_bias())
        return x * scale + bias

    def extra_repr(self):
        return "num_features=%d, eps=%s" % (self.num_features, self.eps)

    # ---- checkpoints of older layouts (batch_norm.py:77-93) ---------------------------------------------------------
    def _load_from_state_dict(self, state_dict, prefix, local_metadata, *rest):
        stored = local_metadata.get("version")
        if stored is None or stored < 2:        # no running statistics in the file: identity statistics
            state_dict.setdefault(prefix + "running_mean", torch.zeros_like(self.running_mean))
            state_dict.setdefault(prefix + "running_var", torch.ones_like(self.running_var))
        if stored is not None and stored < 3:   # the variance was stored WITH eps
            key = prefix + "running_var"
            state_dict[key] = state_dict[key] - self.eps
        super()._load_from_state_dict(state_dict, prefix, local_metadata, *rest)

    # ---- freezing a trained BatchNorm ---------------------------------------------------------------------------------
    @classmethod
    def from_batchnorm(cls, bn):
        frozen = cls(bn.num_features, bn.eps)
        with torch.no_grad():
            if bn.affine:
                frozen.weight.copy_(bn.weight)
                frozen.bias.copy_(bn.bias)
            frozen.running_mean.copy_(bn.running_mean)
            frozen.running_var.copy_(bn.running_var)
        return frozen.to(bn.running_mean.device)

    @classmethod
    def convert_frozen_batchnorm(cls, module):
        """`module` with every BatchNorm2d / SyncBatchNorm in it (or `module` itself) replaced by its frozen form."""
        live = (nn.BatchNorm2d, nn.SyncBatchNorm)
        if isinstance(module, live):
            return cls.from_batchnorm(module)
        for parent in list(module.modules()):
            for name, child in list(parent.named_children()):
                if isinstance(child, live):
                    setattr(parent, name, cls.from_batchnorm(child))
        return module


# ---- batch norm that trains (csrc/batch_norm.hip) ------------------------------------------------------------------
def _world_size(group=None):
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    return dist.get_world_size(group)


def combine_statistics(count, mean, m2, group=None):
    """Per-rank (count, mean, M2 = sum (x - mean)^2) of a (C,) channel vector -> those of the concatenated batch, on
    every rank: ONE all-reduce of a (2C+1) tensor.  The sums travel in fp64 (count * mean, M2 + count * mean^2, count),
    which keeps the variance of a map whose mean is large against its spread.  Host-side, any device and backend;
    returns (total count as a float, mean, m2) with mean / m2 in the dtype they came in."""
    import torch.distributed as dist
    c = mean.numel()
    mu, n = mean.double(), float(count)
    packed = torch.cat([mu * n, m2.double() + n * mu * mu, mu.new_full((1,), n)])
    dist.all_reduce(packed, group=group)
    total = packed[2 * c]
    mean_all = packed[:c] / total
    m2_all = (packed[c:2 * c] - total * mean_all * mean_all).clamp_min(0)
    return float(total), mean_all.to(mean.dtype), m2_all.to(m2.dtype)


def combine_gradient_sums(sums, group=None):
    """Per-rank (2, C) [sum dy, sum dy * xhat] -> the concatenated batch's, on every rank (one all-reduce)."""
    import torch.distributed as dist
    total = sums.double()
    dist.all_reduce(total, group=group)
    return total.to(sums.dtype)


def _row_pitch(x):
    """Leading dimension of a (N,C,H,W) tensor read as N*H*W rows of C floats, or None if it is not stored that way."""
    n, c, h, w = x.shape
    if c > 1 and x.stride(1) != 1:
        return None
    ld = None
    for size, stride, rows in ((w, x.stride(3), 1), (h, x.stride(2), w), (n, x.stride(0), h * w)):
        if size > 1:
            if stride % rows or (ld is not None and ld != stride // rows):
                return None
            ld = stride // rows
    ld = c if ld is None else ld
    return ld if ld >= c else None


class _BatchNormTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, mod, relu):
        from .. import _lib as L
        L.require_gpu(x, gamma, beta, residual)
        n, c, h, w = x.shape
        ld = _row_pitch(x)
        if ld is None:
            x = x.contiguous(memory_format=torch.channels_last)
            ld = c
        rows, dev, lib = n * h * w, x.device, L.lib()
        world = _world_size(mod.process_group) if mod.sync else 1
        if rows * world <= 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
        if residual is not None:
            residual = residual.contiguous(memory_format=torch.channels_last)
        stats = torch.empty((3, c), dtype=torch.float32, device=dev)
        mean, m2, invstd = stats[0], stats[1], stats[2]
        ws = torch.empty(lib.jtsm_batch_norm_workspace_bytes(rows, c), dtype=torch.uint8, device=dev)
        y = torch.empty((n, c, h, w), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        with torch.no_grad():
            mod.num_batches_tracked.add_(1)
        rm, rv, count = mod.running_mean, mod.running_var, float(rows)
        L.note_bytes(4.0 * x.numel())
        if world == 1:
            L.check(lib.jtsm_batch_norm_stats_f32(L.ptr(x), ld, rows, c, L.ptr(mean), L.ptr(m2), mod.eps, mod.momentum,
                                                  L.ptr(invstd), L.ptr(rm), L.ptr(rv), L.ptr(ws), L.stream()),
                    "batch_norm_stats")
        else:
            L.check(lib.jtsm_batch_norm_stats_f32(L.ptr(x), ld, rows, c, L.ptr(mean), L.ptr(m2), mod.eps, mod.momentum,
                                                  None, None, None, L.ptr(ws), L.stream()), "batch_norm_stats")
            count, mean_all, m2_all = combine_statistics(rows, mean, m2, mod.process_group)
            mean.copy_(mean_all)
            m2.copy_(m2_all)
            L.check(lib.jtsm_batch_norm_finalize_f32(L.ptr(mean), L.ptr(m2), count, c, mod.eps, mod.momentum,
                                                     L.ptr(invstd), L.ptr(rm), L.ptr(rv), L.stream()),
                    "batch_norm_finalize")
        mod._memo = None          # the kernels wrote the running statistics behind the version counters
        L.note_bytes(4.0 * (x.numel() + y.numel() + (y.numel() if residual is not None else 0)))
        L.check(lib.jtsm_batch_norm_apply_f32(L.ptr(x), ld, L.ptr(residual), L.ptr(mean), L.ptr(invstd), L.ptr(gamma),
                                              L.ptr(beta), L.ptr(y), rows, c, int(relu), L.stream()), "batch_norm_apply")
        ctx.save_for_backward(x, y if relu else None, gamma, stats)
        ctx.cfg = (ld, bool(relu), residual is not None, count, world, mod.process_group)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .. import _lib as L
        x, y, gamma, stats = ctx.saved_tensors
        ld, relu, has_res, count, world, group = ctx.cfg
        n, c, h, w = x.shape
        rows, dev, lib = n * h * w, x.device, L.lib()
        mean, invstd = stats[0], stats[2]
        dy = dy.contiguous(memory_format=torch.channels_last)
        sums = torch.empty((2, c), dtype=torch.float32, device=dev)
        ws = torch.empty(lib.jtsm_batch_norm_workspace_bytes(rows, c), dtype=torch.uint8, device=dev)
        L.note_bytes(4.0 * x.numel() * (3 if relu else 2))
        L.check(lib.jtsm_batch_norm_backward_reduce_f32(L.ptr(x), ld, L.ptr(dy), L.ptr(y), L.ptr(mean), L.ptr(invstd),
                                                        L.ptr(sums[0]), L.ptr(sums[1]), L.ptr(ws), rows, c, int(relu),
                                                        L.stream()), "batch_norm_backward_reduce")
        # dgamma / dbeta are this rank's sums (the data-parallel wrapper averages parameter gradients); dx needs the
        # whole batch's
        total = combine_gradient_sums(sums, group) if world > 1 else sums
        dx = torch.empty((n, c, h, w), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        dres = torch.empty_like(dx) if has_res and ctx.needs_input_grad[3] else None
        L.note_bytes(4.0 * x.numel() * ((4 if relu else 3) + (1 if dres is not None else 0)))
        L.check(lib.jtsm_batch_norm_backward_apply_f32(L.ptr(x), ld, L.ptr(dy), L.ptr(y), L.ptr(mean), L.ptr(invstd),
                                                       L.ptr(gamma), L.ptr(total[0]), L.ptr(total[1]), count, L.ptr(dx),
                                                       L.ptr(dres), rows, c, int(relu), L.stream()),
                "batch_norm_backward_apply")
        return dx, sums[1], sums[0], dres, None, None


class _ImageMean(torch.autograd.Function):
    """Per-(image, channel) mean of a channels-last map, (N, C, 1, 1): the statistics reduction above, one image at a
    time (adaptive_avg_pool2d(x, 1) — ASPP's image pooling at the training crop)."""

    @staticmethod
    def forward(ctx, x):
        from .. import _lib as L
        L.require_gpu(x)
        n, c, h, w = x.shape
        if _row_pitch(x) is None:
            x = x.contiguous(memory_format=torch.channels_last)
        ld, rows, lib = _row_pitch(x), h * w, L.lib()
        out = torch.empty((n, 2, c), dtype=torch.float32, device=x.device)      # [mean, M2] per image
        ws = torch.empty(lib.jtsm_batch_norm_workspace_bytes(rows, c), dtype=torch.uint8, device=x.device)
        for i in range(n):
            L.note_bytes(4.0 * rows * c)
            L.check(lib.jtsm_batch_norm_stats_f32(L.ptr(x[i]), ld, rows, c, L.ptr(out[i, 0]), L.ptr(out[i, 1]), 0.0, 0.0,
                                                  None, None, None, L.ptr(ws), L.stream()), "batch_norm_stats")
        ctx.shape = (n, c, h, w)
        return out[:, 0].reshape(n, c, 1, 1).contiguous(memory_format=torch.channels_last)

    @staticmethod
    def backward(ctx, g):
        n, c, h, w = ctx.shape
        return (g.reshape(n, c, 1, 1) / float(h * w)).expand(n, c, h, w)


def image_mean(x):
    """F.adaptive_avg_pool2d(x, 1) of a float32 channels-last device map."""
    return _ImageMean.apply(x)


class BatchNorm2d(nn.BatchNorm2d):
    """torch.nn.BatchNorm2d (same parameters, buffers and state-dict keys) whose training pass runs on
    csrc/batch_norm.hip: statistics, then ONE pass y = relu?(xhat * weight + bias (+ residual)).  `Conv2d` calls
    `fused()` behind a plain contraction in training mode and folds `scale_bias()` into the contraction's epilogue in
    evaluation mode, exactly as for FrozenBatchNorm2d — evaluation launches no norm kernel.

    sync=True ("SyncBN", "nnSyncBN", "naiveSyncBN"): with more than one process the per-rank (count, mean, M2) and the
    backward's (sum dy, sum dy * xhat) are all-reduced over torch.distributed, so the result is batch norm over the
    concatenated batch; with one process it is plain BN."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, sync=False, process_group=None):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=True, track_running_stats=True)
        if momentum is None:
            raise NotImplementedError("jtsm_amd BatchNorm2d: a fixed momentum only (no cumulative average)")
        self.sync, self.process_group = bool(sync), process_group
        self._memo = None

    _stamp = FrozenBatchNorm2d._stamp
    scale_bias = FrozenBatchNorm2d.scale_bias

    def fused(self, x, relu=False, residual=None):
        """Training-mode relu?(bn(x) + residual) on a float32 device map; updates the running statistics."""
        return _BatchNormTrain.apply(x, self.weight, self.bias, residual, self, relu)

    def forward(self, x):
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
            return super().forward(x)         # host tensors (construction-time checks, the gloo tests)
        if self.training:
            return self.fused(x)
        return FrozenBatchNorm2d.forward(self, x)


_NORMS = {"FrozenBN": FrozenBatchNorm2d, "GN": lambda channels: nn.GroupNorm(32, channels), "BN": BatchNorm2d,
          # one process: plain BN; several: statistics over all of them, whichever of the reference's three the name asks for
          "SyncBN": lambda channels: BatchNorm2d(channels, sync=True),
          "nnSyncBN": lambda channels: BatchNorm2d(channels, sync=True),
          "naiveSyncBN": lambda channels: BatchNorm2d(channels, sync=True)}


def get_norm(norm, out_channels):
    """None / "" -> no norm; "FrozenBN" | "GN" (what the BASELINE configs use), the trainable "BN" | "SyncBN" |
    "nnSyncBN" | "naiveSyncBN" of batch_norm.py:128-153 (what the DeepLab configs use), or any callable(channels)
    -> module."""
    if not norm:
        return None
    if callable(norm):
        return norm(out_channels)
    if norm not in _NORMS:
        raise KeyError("jtsm_amd supports norm in %s on the JTSM path, got '%s'" % (sorted(_NORMS), norm))
    return _NORMS[norm](out_channels)
