"""GPU suite (pytest -m gpu): deformable ResNet stages (DeformBottleneckBlock) in the R-50 backbone and in the Faster
R-CNN R50-FPN of tests/test_deform_config.deform_cfg.

* At initialisation conv2_offset is zero, so every offset is zero: the v1 deformable backbone with the plain backbone's
  weights computes the plain backbone's res2..res5; the v2 backbone (mask = sigmoid(0) = 0.5) does so with every
  deformable conv2 weight doubled.  Criterion: tests/test_hip_conv.py's for a contraction — per tensor
  max|a - b| / max|b| <= 1e-4 and an element-wise allclose with rtol 1e-4, atol 1e-4 max|b|.
* One training step: finite losses, finite conv2_offset gradients that are non-zero in res5, and a second run from the
  same seed with bit-identical losses and gradients.

The weight gradient of a layer whose output-channel count is no multiple of 8 takes the fp32 kernel, which adds its K
slices with atomicAdd; in this model those were the offset convolutions, the RPN head's two predictors (3 and 12
channels) and cls_score (81), whose gradients differed by 6e-8 to 1.2e-7 of their largest entry between two runs.  They
run zero-padded to a multiple of 8 now (layers/wrappers.py: conv2d_padded, linear_padded)."""
import pytest
import torch

from test_deform_config import deform_cfg

pytestmark = pytest.mark.gpu

REL = 1e-4
FEATURES = ["res2", "res3", "res4", "res5"]


def _backbone(cuda, stages, modulated):
    from jtsm_amd.layers.shape_spec import ShapeSpec
    from jtsm_amd.modeling.backbone.resnet import build_resnet_backbone

    cfg = deform_cfg("cuda", modulated=modulated, stages=stages)
    cfg.MODEL.RESNETS.OUT_FEATURES = FEATURES
    torch.manual_seed(0)
    return build_resnet_backbone(cfg, ShapeSpec(channels=3)).to(cuda).eval()


@pytest.fixture(scope="module")
def plain(cuda):
    torch.manual_seed(5)
    x = torch.randn(2, 3, 128, 160, device=cuda)
    net = _backbone(cuda, (False, False, False, False), False)
    with torch.no_grad():
        return net, x, {k: v.clone() for k, v in net(x).items()}


@pytest.mark.parametrize("modulated", [False, True], ids=["v1", "v2"])
def test_deformable_backbone_at_initialisation_is_the_plain_backbone(cuda, plain, modulated):
    from jtsm_amd.modeling.backbone.resnet import DeformBottleneckBlock

    net0, x, want = plain
    net = _backbone(cuda, (False, True, True, True), modulated)
    missing, unexpected = net.load_state_dict(net0.state_dict(), strict=False)
    assert not unexpected and missing and all(".conv2_offset." in k for k in missing)
    blocks = [m for m in net.modules() if isinstance(m, DeformBottleneckBlock)]
    assert len(blocks) == 13
    with torch.no_grad():
        for b in blocks:
            assert float(b.conv2_offset.weight.abs().max()) == 0.0 and float(b.conv2_offset.bias.abs().max()) == 0.0
            if modulated:
                b.conv2.weight.mul_(2.0)
        got = net(x)
    assert sorted(got) == FEATURES
    for k in FEATURES:
        a, b = got[k].double().cpu(), want[k].double().cpu()
        ref = b.abs().max().item()
        err = (a - b).abs().max().item()
        print("%s: max err %.3e vs max ref %.3e (rel %.2e)" % (k, err, ref, err / ref))
        assert a.shape == b.shape and ref > 0
        assert err <= REL * ref, (k, err, ref)
        assert torch.allclose(a, b, rtol=REL, atol=REL * ref), k


def _batch(cuda):
    from jtsm_amd.structures import Boxes, Instances

    g = torch.Generator().manual_seed(99)
    gt = [[[20.0, 30.0, 90.0, 100.0], [60.0, 10.0, 150.0, 70.0], [5.0, 60.0, 60.0, 120.0]],
          [[30.0, 20.0, 120.0, 110.0], [100.0, 50.0, 155.0, 125.0]]]
    classes = [[0, 2, 1], [1, 0]]
    return [{"image": (torch.rand(3, 128, 160, generator=g) * 255).to(cuda),
             "instances": Instances((128, 160), gt_boxes=Boxes(torch.tensor(b).to(cuda)),
                                    gt_classes=torch.tensor(c).to(cuda))} for b, c in zip(gt, classes)]


@pytest.fixture(scope="module", params=[False, True], ids=["v1", "v2"])
def two_steps(request, cuda):
    """One training step of the deformable Faster R-CNN, run twice from the same seeds: ((losses, grads), (losses, grads))."""
    from jtsm_amd.modeling import build_model

    modulated = request.param

    def step():
        torch.manual_seed(0)
        model = build_model(deform_cfg("cuda", modulated=modulated, groups=2 if modulated else 1))
        with torch.no_grad():
            model.backbone.bottom_up.stem.conv1.weight.mul_(1.0 / 64)
            model.roi_heads.box_head.fc1.weight.mul_(0.02)
        model.train()
        torch.manual_seed(1)
        losses = model(_batch(cuda))
        sum(losses.values()).backward()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        return {k: v.detach().clone() for k, v in losses.items()}, grads

    return step(), step()


def _differing(a, b):
    assert sorted(a) == sorted(b)
    return {n: float((a[n] - b[n]).abs().max() / a[n].abs().max()) for n in a if not torch.equal(a[n], b[n])}


def test_deformable_faster_rcnn_training_step(two_steps):
    (losses, grads), (losses2, grads2) = two_steps
    assert set(losses) == {"loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg"}
    assert all(bool(torch.isfinite(v)) for v in losses.values()), losses
    offsets = [n for n in grads if ".conv2_offset.weight" in n]
    assert len(offsets) == 13
    for n in offsets:
        assert bool(torch.isfinite(grads[n]).all()), n
    res5 = [n for n in offsets if ".res5." in n]
    assert len(res5) == 3 and all(float(grads[n].abs().sum()) > 0 for n in res5)
    for n in grads:
        if ".conv2.weight" in n and ".res5." in n:
            assert float(grads[n].abs().sum()) > 0, n
    # the second run: the same losses, and the same bits in every gradient of the backbone — the deformable stages, the
    # offset convolutions and everything their input gradients reach
    assert not _differing(losses, losses2)
    backbone = {n for n in grads if n.startswith("backbone.")}
    assert len(backbone) == 84       # 13 blocks x (conv1, conv2_offset weight and bias, conv2, conv3), 3 shortcuts, 16 of the FPN
    differ = _differing({n: grads[n] for n in backbone}, {n: grads2[n] for n in backbone})
    assert not differ, differ


def test_deformable_faster_rcnn_training_step_repeats_every_gradient(two_steps):
    """The whole model: bit-identical losses and gradients in a second run from the same seed."""
    (losses, grads), (losses2, grads2) = two_steps
    assert not _differing(losses, losses2)
    differ = _differing(grads, grads2)
    print("gradients that differ between two runs (relative to their largest entry):", differ)
    assert not differ, differ
