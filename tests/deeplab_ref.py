"""fp64 restatements for the DeepLab tests, written from the reference's behaviour with stock torch CPU ops
(F.batch_norm, F.interpolate, F.cross_entropy, torch.topk).  Nothing here touches the HIP library."""
import torch
import torch.nn.functional as F


def max_rel(got, want):
    """Max-norm relative error: max |got - want| / max(|want|, tiny)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    if want.numel() == 0:
        return 0.0
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def batch_norm_train(x, gamma, beta, dy, residual=None, relu=False, eps=1e-5, momentum=0.1, running_mean=None,
                     running_var=None):
    """relu?(F.batch_norm(x, training=True) + residual) in fp64 and its gradients for the upstream `dy`.
    Returns a dict: y, dx, dgamma, dbeta, dres (None without a residual), running_mean, running_var, mean, var."""
    c = x.shape[1]
    x64 = x.detach().double().cpu().contiguous().requires_grad_(True)
    g64 = gamma.detach().double().cpu().requires_grad_(True)
    b64 = beta.detach().double().cpu().requires_grad_(True)
    r64 = residual.detach().double().cpu().contiguous().requires_grad_(True) if residual is not None else None
    rm = torch.zeros(c, dtype=torch.float64) if running_mean is None else running_mean.detach().double().cpu().clone()
    rv = torch.ones(c, dtype=torch.float64) if running_var is None else running_var.detach().double().cpu().clone()
    y = F.batch_norm(x64, rm, rv, g64, b64, True, momentum, eps)
    if r64 is not None:
        y = y + r64
    if relu:
        y = F.relu(y)
    y.backward(dy.detach().double().cpu())
    return {"y": y.detach(), "dx": x64.grad, "dgamma": g64.grad, "dbeta": b64.grad,
            "dres": r64.grad if r64 is not None else None, "running_mean": rm, "running_var": rv,
            "mean": x64.detach().mean(dim=(0, 2, 3)), "var": x64.detach().var(dim=(0, 2, 3), unbiased=False)}


def pixel_losses(logits, target, scale, ignore_index, weights=None):
    """The per-pixel cross-entropies DeepLabCE ranks, fp64, shape (N, H, W); `logits` must require grad to backpropagate."""
    up = F.interpolate(logits, scale_factor=scale, mode="bilinear", align_corners=False)
    losses = F.cross_entropy(up, target, ignore_index=ignore_index, reduction="none")
    return losses if weights is None else losses * weights


def deeplab_ce(logits, target, scale, ignore_index, top_k_percent_pixels, weights=None, selected=None):
    """DeepLabCE on the up-sampled logits in fp64: (loss, dlogits, per-pixel losses, k).  `selected`: a flat boolean mask
    that replaces torch.topk's choice (for the tie rule, where topk's is open)."""
    z = logits.detach().double().cpu().contiguous().requires_grad_(True)
    t = target.detach().cpu().long()
    w = weights.detach().double().cpu() if weights is not None else None
    pl = pixel_losses(z, t, scale, ignore_index, w).contiguous().view(-1)
    if top_k_percent_pixels == 1.0:
        k = pl.numel()
        loss = pl.mean()
    else:
        k = int(top_k_percent_pixels * pl.numel())
        if selected is not None:
            assert int(selected.sum()) == k
            loss = pl[selected.view(-1)].sum() / k
        else:
            loss = torch.topk(pl, k)[0].mean()
    loss.backward()
    return loss.detach(), z.grad, pl.detach(), k


def kth_gap(pl, k):
    """Gap between the k-th and the (k+1)-th largest per-pixel loss (inf when k is everything)."""
    if k >= pl.numel():
        return float("inf")
    top = torch.topk(pl.view(-1), k + 1)[0]
    return float(top[k - 1] - top[k])


# ---- the heads, with stock torch modules under the reference's module names (so a state dict loads) -------------------
class RefConv(torch.nn.Conv2d):
    """nn.Conv2d with the wrappers' `norm` child (nn.BatchNorm2d) and optional ReLU."""

    def __init__(self, cin, cout, k, padding=0, dilation=1, norm=True, relu=True):
        super().__init__(cin, cout, k, padding=padding, dilation=dilation, bias=not norm)
        self.norm = torch.nn.BatchNorm2d(cout) if norm else None
        self.relu = relu

    def forward(self, x):
        y = super().forward(x)
        if self.norm is not None:
            y = self.norm(y)
        return F.relu(y) if self.relu else y


class RefASPP(torch.nn.Module):
    def __init__(self, cin, cout, dilations):
        super().__init__()
        self.convs = torch.nn.ModuleList([RefConv(cin, cout, 1)])
        for d in dilations:
            self.convs.append(RefConv(cin, cout, 3, padding=d, dilation=d))
        self.convs.append(torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(1), RefConv(cin, cout, 1, norm=False)))
        self.project = RefConv(5 * cout, cout, 1)

    def forward(self, x):
        res = [conv(x) for conv in self.convs]
        res[-1] = F.interpolate(res[-1], size=x.shape[-2:], mode="bilinear", align_corners=False)
        return self.project(torch.cat(res, dim=1))


class RefV3PlusHead(torch.nn.Module):
    """DeepLabV3PlusHead with in_features [res2, res5], batch norm everywhere, no dropout, plain cross-entropy."""

    def __init__(self, c2, c5, project, dim, aspp, dilations, classes, stride, ignore):
        super().__init__()
        self.stride, self.ignore = stride, ignore
        self.decoder = torch.nn.ModuleDict()
        self.decoder["res2"] = torch.nn.ModuleDict({
            "project_conv": RefConv(c2, project, 1),
            "fuse_conv": torch.nn.Sequential(RefConv(project + aspp, dim, 3, padding=1), RefConv(dim, dim, 3, padding=1))})
        self.decoder["res5"] = torch.nn.ModuleDict({"project_conv": RefASPP(c5, aspp, dilations)})
        self.predictor = RefConv(dim, classes, 1, norm=False, relu=False)

    def forward(self, features, targets):
        y = self.decoder["res5"]["project_conv"](features["res5"])
        proj = self.decoder["res2"]["project_conv"](features["res2"])
        y = F.interpolate(y, size=proj.shape[2:], mode="bilinear", align_corners=False)
        y = self.predictor(self.decoder["res2"]["fuse_conv"](torch.cat([proj, y], dim=1)))
        y = F.interpolate(y, scale_factor=self.stride, mode="bilinear", align_corners=False)
        return F.cross_entropy(y, targets, reduction="mean", ignore_index=self.ignore)


class RefV3Head(torch.nn.Module):
    def __init__(self, c5, aspp, dilations, classes, stride, ignore):
        super().__init__()
        self.stride, self.ignore = stride, ignore
        self.aspp = RefASPP(c5, aspp, dilations)
        self.predictor = RefConv(aspp, classes, 1, norm=False, relu=False)

    def forward(self, features, targets):
        y = self.predictor(self.aspp(features["res5"]))
        y = F.interpolate(y, scale_factor=self.stride, mode="bilinear", align_corners=False)
        return F.cross_entropy(y, targets, reduction="mean", ignore_index=self.ignore)


def load_double(ref, state_dict):
    """`ref` in fp64 with the (device, fp32) state dict of the module under test; the unused None child is no key."""
    ref.double()
    ref.load_state_dict({k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu())
                         for k, v in state_dict.items()}, strict=True)
    return ref.train()
