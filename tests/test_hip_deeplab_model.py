"""GPU suite: DeepLab v3 / v3+ end to end — the heads against stock-torch restatements in fp64 (tests/deeplab_ref.py),
a training step, its reproducibility, the optimizer and inference, on the flattened v3+ config shrunk to DEPTH 50,
5 classes, ASPP_CHANNELS = CONVS_DIM = 32, PROJECT_CHANNELS [16] and a (64, 128) crop."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deeplab_ref as R

pytestmark = pytest.mark.gpu

from jtsm_amd.config import get_cfg  # noqa: E402
from jtsm_amd.layers.shape_spec import ShapeSpec  # noqa: E402
from jtsm_amd.modeling import build_model  # noqa: E402

REL = 1e-4
FLAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "configs")
V3PLUS, V3 = "deeplab_v3_plus_R_103_os16_mg124_poly_90k_bs16", "deeplab_v3_R_103_os16_mg124_poly_90k_bs16"
SHRINK = ["MODEL.RESNETS.DEPTH", 50, "MODEL.SEM_SEG_HEAD.NUM_CLASSES", 5, "MODEL.SEM_SEG_HEAD.ASPP_CHANNELS", 32,
          "MODEL.SEM_SEG_HEAD.CONVS_DIM", 32, "MODEL.SEM_SEG_HEAD.PROJECT_CHANNELS", [16], "INPUT.CROP.SIZE", [64, 128]]


def _cfg(name=V3PLUS, *overrides):
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(FLAT, name + ".yaml"))
    cfg.merge_from_list(SHRINK + list(overrides))
    return cfg


def _batch(seed=0, h=64, w=128, labels=True):
    """Two images with block-wise random labels and a band of 255."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(2):
        item = {"image": torch.randint(0, 256, (3, h, w), generator=g).float(), "image_id": i, "height": h, "width": w}
        if labels:
            blocks = torch.randint(0, 5, (h // 8, w // 8), generator=g)
            sem = blocks.repeat_interleave(8, 0).repeat_interleave(8, 1)
            sem[:, 40:48] = 255
            item["sem_seg"] = sem
        out.append(item)
    return out


@pytest.fixture
def f32_math():
    from jtsm_amd.layers import conv as K
    before = K.MATH
    K.set_math("f32")
    yield
    K.set_math(before)


@pytest.fixture(scope="module")
def model(cuda):
    torch.manual_seed(1)
    return build_model(_cfg())


def _head_inputs(cuda, with_res2):
    g = torch.Generator().manual_seed(4)
    feats = {"res5": torch.randn(2, 64, 4, 8, generator=g)}
    if with_res2:
        feats["res2"] = torch.randn(2, 32, 16, 32, generator=g)
    target = torch.randint(0, 5, (2, 64, 128), generator=g)
    target[:, :, 40:48] = 255
    shapes = {"res2": ShapeSpec(channels=32, stride=4), "res5": ShapeSpec(channels=64, stride=16)}
    return feats, target, shapes


def _check_head(head, ref, feats, target, cuda):
    from jtsm_amd.layers.conv import planes_clear
    with torch.no_grad():                       # norm parameters off their defaults, so that their role shows
        for m in head.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
        head.predictor.weight.normal_(0, 0.5)
    R.load_double(ref, head.state_dict())
    head.train()
    planes_clear()
    dev = {k: v.to(cuda).contiguous(memory_format=torch.channels_last).requires_grad_(True) for k, v in feats.items()}
    _, losses = head(dev, target.to(cuda))
    losses["loss_sem_seg"].backward()
    f64 = {k: v.double().requires_grad_(True) for k, v in feats.items()}
    want = ref(f64, target)
    want.backward()
    torch.cuda.synchronize()
    assert R.max_rel(losses["loss_sem_seg"], want) <= REL
    got_params, want_params = dict(head.named_parameters()), dict(ref.named_parameters())
    assert sorted(got_params) == sorted(want_params)
    for name, p in got_params.items():
        err = R.max_rel(p.grad, want_params[name].grad)
        print(name, err)
        assert err <= REL, (name, err)
    for k in feats:
        assert R.max_rel(dev[k].grad, f64[k].grad) <= REL, k
    for (name, b), (_, rb) in zip(head.named_buffers(), ref.named_buffers()):
        assert R.max_rel(b.double(), rb.double()) <= REL, name        # the running statistics moved alike


def test_v3plus_head_matches_the_stock_torch_restatement(cuda, f32_math):
    from jtsm_amd.modeling.meta_arch.deeplab import DeepLabV3PlusHead
    feats, target, shapes = _head_inputs(cuda, True)
    torch.manual_seed(2)
    head = DeepLabV3PlusHead(shapes, in_features=["res2", "res5"], project_channels=[16], aspp_dilations=[6, 12, 18],
                             aspp_dropout=0.0, decoder_channels=[32, 32], common_stride=4, norm="BN",
                             train_size=(64, 128), loss_weight=1.0, loss_type="cross_entropy", ignore_value=255,
                             num_classes=5).to(cuda)
    _check_head(head, R.RefV3PlusHead(32, 64, 16, 32, 32, [6, 12, 18], 5, 4, 255), feats, target, cuda)
    decoder = DeepLabV3PlusHead(shapes, in_features=["res2", "res5"], project_channels=[16], aspp_dilations=[6, 12, 18],
                                aspp_dropout=0.0, decoder_channels=[32, 32], common_stride=4, norm="BN",
                                train_size=None).to(cuda)
    assert decoder.decoder_only and not hasattr(decoder, "predictor")          # what Panoptic-DeepLab subclasses
    y = decoder({k: v.to(cuda) for k, v in feats.items()})
    assert tuple(y.shape) == (2, 32, 16, 32)


def test_v3_head_matches_the_stock_torch_restatement(cuda, f32_math):
    from jtsm_amd.modeling.meta_arch.deeplab import DeepLabV3Head
    feats, target, shapes = _head_inputs(cuda, False)
    cfg = _cfg(V3, "MODEL.SEM_SEG_HEAD.ASPP_DROPOUT", 0.0, "MODEL.SEM_SEG_HEAD.LOSS_TYPE", "cross_entropy",
               "MODEL.SEM_SEG_HEAD.NORM", "BN")
    torch.manual_seed(3)
    head = DeepLabV3Head(cfg, {"res5": shapes["res5"]}).to(cuda)
    _check_head(head, R.RefV3Head(64, 32, [6, 12, 18], 5, 16, 255), feats, target, cuda)


def _step(model, seed):
    model.train()
    model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    losses = model(_batch())
    loss = sum(losses.values())
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def test_training_step_moves_every_parameter_and_every_running_mean(cuda, model):
    from jtsm_amd.layers.batch_norm import BatchNorm2d
    assert model.sem_seg_head.loss_type == "hard_pixel_mining"
    norms = [m for m in model.modules() if isinstance(m, BatchNorm2d)]
    assert norms and all(m.sync for m in norms)
    before = [m.running_mean.clone() for m in norms]
    tracked = [int(m.num_batches_tracked) for m in norms]
    loss, grads = _step(model, 0)
    assert torch.isfinite(loss)
    for name, g in grads.items():
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, name
    for m, b, t in zip(norms, before, tracked):
        assert not torch.equal(m.running_mean, b) and int(m.num_batches_tracked) == t + 1 == 1


def test_two_seeded_steps_give_the_same_bits(cuda, model):
    assert model.sem_seg_head.decoder["res5"]["project_conv"].dropout > 0          # dropout is on
    a, b = _step(model, 7), _step(model, 7)
    assert torch.equal(a[0], b[0])
    for name in a[1]:
        assert torch.equal(a[1][name], b[1][name]), name


def test_one_sgd_step_with_the_norm_weight_decay_group(cuda, model):
    from jtsm_amd.solver.build import build_optimizer
    cfg = _cfg(V3PLUS, "SOLVER.WEIGHT_DECAY_NORM", 0.125)
    opt = build_optimizer(cfg, model)
    norm_params = {id(p) for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d) for p in m.parameters()}
    assert norm_params
    for group in opt.param_groups:
        assert all((group["weight_decay"] == 0.125) == (id(p) in norm_params) for p in group["params"])
    _step(model, 1)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p, before[n]), n


def test_inference_feeds_the_evaluator(cuda, model):
    from jtsm_amd.evaluation import SemSegEvaluator
    model.eval()
    batch = _batch(seed=5)
    with torch.no_grad():
        out = model([{k: v for k, v in item.items() if k != "sem_seg"} for item in batch])
    assert len(out) == 2
    for o in out:
        assert tuple(o["sem_seg"].shape) == (5, 64, 128) and torch.isfinite(o["sem_seg"]).all()
    gt = {item["image_id"]: item["sem_seg"].numpy().astype(np.uint8) for item in batch}
    ev = SemSegEvaluator(["c%d" % i for i in range(5)], 255, gt)
    ev.process(batch, out)
    miou = ev.evaluate()["sem_seg"]["mIoU"]
    assert np.isfinite(miou)
    # a larger map with the (64, 128)-derived pooling window (4, 8): the window slides.  The reference's rule asks that
    # the window divides the map: 64 x 256 (a 4 x 16 map) runs; 64 x 192 (4 x 12) and a 65-pixel-high image (5 rows)
    # raise its ValueError
    with torch.no_grad():
        wide = model(_batch(seed=6, h=64, w=256, labels=False))
        assert tuple(wide[0]["sem_seg"].shape) == (5, 64, 256) and torch.isfinite(wide[0]["sem_seg"]).all()
        for h, w in ((64, 192), (65, 128)):
            with pytest.raises(ValueError, match="pool_kernel_size"):
                model(_batch(seed=6, h=h, w=w, labels=False))


def test_pooled_branch_broadcast_is_the_interpolation_bit_for_bit(cuda):
    from jtsm_amd.layers.aspp import broadcast_or_resize
    from jtsm_amd.layers.batch_norm import image_mean
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(2, 24, 4, 8, generator=g) + 3).to(cuda).contiguous(memory_format=torch.channels_last)
    pooled = image_mean(x)
    assert tuple(pooled.shape) == (2, 24, 1, 1)
    assert R.max_rel(pooled, F.adaptive_avg_pool2d(x.double(), 1)) <= REL
    want = F.interpolate(pooled, size=(4, 8), mode="bilinear", align_corners=False)
    assert torch.equal(broadcast_or_resize(pooled, (4, 8)), want)
