"""GPU suite: Panoptic-DeepLab end to end — the two heads against stock-torch restatements in fp64 under the reference's
module names (tests/deeplab_ref.py's building blocks), a training step with generated targets, its reproducibility, one
Adam step, and inference through the three evaluators — on the flattened project config shrunk to narrow heads and a
(64, 128) crop."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deeplab_ref as D
import panoptic_deeplab_ref as R

pytestmark = pytest.mark.gpu

from jtsm_amd.config import add_panoptic_deeplab_config, get_cfg  # noqa: E402
from jtsm_amd.layers.shape_spec import ShapeSpec  # noqa: E402
from jtsm_amd.modeling import build_model  # noqa: E402

REL = 1e-4                      # the bar of tests/test_hip_deeplab_model.py
FLAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "configs",
                    "panoptic_deeplab_R_52_os16_mg124_poly_90k_bs32_crop_512_1024.yaml")
SHRINK = ["MODEL.SEM_SEG_HEAD.ASPP_CHANNELS", 32, "MODEL.SEM_SEG_HEAD.CONVS_DIM", 32,
          "MODEL.SEM_SEG_HEAD.HEAD_CHANNELS", 32, "MODEL.SEM_SEG_HEAD.PROJECT_CHANNELS", [16, 16],
          "MODEL.INS_EMBED_HEAD.ASPP_CHANNELS", 32, "MODEL.INS_EMBED_HEAD.CONVS_DIM", 32,
          "MODEL.INS_EMBED_HEAD.HEAD_CHANNELS", 16, "MODEL.INS_EMBED_HEAD.PROJECT_CHANNELS", [8, 16],
          "MODEL.PANOPTIC_DEEPLAB.STUFF_AREA", 32, "MODEL.PANOPTIC_DEEPLAB.TOP_K_INSTANCE", 20,
          "INPUT.CROP.SIZE", [64, 128], "INPUT.GAUSSIAN_SIGMA", 4, "INPUT.SMALL_INSTANCE_AREA", 200]
THINGS = tuple(range(11, 19))


def _cfg(*overrides):
    cfg = get_cfg()
    add_panoptic_deeplab_config(cfg)
    cfg.merge_from_file(FLAT)
    cfg.merge_from_list(SHRINK + list(overrides))
    return cfg


def _batch(cfg, seed=0, h=64, w=128, targets=True):
    """Two images; the targets come from PanopticDeepLabTargetGenerator on a map of two stuff bands, three elliptic
    things and an unlabelled band."""
    from jtsm_amd.data import PanopticDeepLabTargetGenerator
    gen = PanopticDeepLabTargetGenerator(cfg.MODEL.SEM_SEG_HEAD.IGNORE_VALUE, THINGS, sigma=cfg.INPUT.GAUSSIAN_SIGMA,
                                         ignore_stuff_in_offset=cfg.INPUT.IGNORE_STUFF_IN_OFFSET,
                                         small_instance_area=cfg.INPUT.SMALL_INSTANCE_AREA,
                                         small_instance_weight=cfg.INPUT.SMALL_INSTANCE_WEIGHT,
                                         ignore_crowd_in_semantic=cfg.INPUT.IGNORE_CROWD_IN_SEMANTIC)
    g = torch.Generator().manual_seed(seed)
    ys, xs = np.mgrid[:h, :w]
    out = []
    for i in range(2):
        item = {"image": torch.randint(0, 256, (3, h, w), generator=g).float(), "image_id": i, "height": h, "width": w}
        if targets:
            pan = np.zeros((h, w), np.int32)
            pan[:h // 2], pan[h // 2:] = 1, 2
            pan[:, 40:48] = 0
            segments = [dict(id=1, category_id=0, iscrowd=0), dict(id=2, category_id=8, iscrowd=0)]
            for k in range(3):
                cy, cx = (int(v) for v in torch.randint(8, 56, (2,), generator=g))
                pan[((ys - cy) / 7.0) ** 2 + ((xs - 2 * cx) / (6.0 + 4 * k)) ** 2 <= 1] = 100 + k
                segments.append(dict(id=100 + k, category_id=11 + 2 * k + i, iscrowd=0))
            item.update({k: v for k, v in gen(pan, segments).items() if k != "center_points"})
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


def test_the_config_loads_and_builds(cuda, model):
    from jtsm_amd.modeling.meta_arch.panoptic_deeplab import (PanopticDeepLab, PanopticDeepLabInsEmbedHead,
                                                              PanopticDeepLabSemSegHead)
    assert type(model) is PanopticDeepLab and model.thing_ids == THINGS and model.label_divisor == 1000
    assert type(model.sem_seg_head) is PanopticDeepLabSemSegHead and model.sem_seg_head.decoder_only
    assert type(model.ins_embed_head) is PanopticDeepLabInsEmbedHead
    assert (model.ins_embed_head.center_loss_weight, model.ins_embed_head.offset_loss_weight) == (200.0, 0.01)
    assert model.sem_seg_head.loss_type == "hard_pixel_mining" and model.sem_seg_head.loss_top_k == 0.2
    assert (model.stuff_area, model.threshold, model.nms_kernel, model.top_k) == (32, 0.1, 7, 20)
    keys = set(model.state_dict())
    for k in ("sem_seg_head.head.0.weight", "sem_seg_head.head.1.norm.running_mean", "sem_seg_head.predictor.bias",
              "ins_embed_head.center_head.0.weight", "ins_embed_head.center_predictor.weight",
              "ins_embed_head.offset_head.1.norm.weight", "ins_embed_head.offset_predictor.bias",
              "ins_embed_head.decoder.res3.fuse_conv.0.weight", "sem_seg_head.decoder.res5.project_conv.project.weight"):
        assert k in keys, k
    assert tuple(model.ins_embed_head.offset_predictor.weight.shape) == (2, 16, 1, 1)


# ---- the heads against stock torch -------------------------------------------------------------------------------------
class RefDecoder(torch.nn.Module):
    """The v3+ decoder over [res2, res3, res5] with batch norm everywhere and no dropout."""

    def __init__(self, channels, project, dims, dilations):
        super().__init__()
        self.names = ["res2", "res3", "res5"]
        self.decoder = torch.nn.ModuleDict()
        for i, name in enumerate(self.names):
            if i == len(self.names) - 1:
                self.decoder[name] = torch.nn.ModuleDict({"project_conv": D.RefASPP(channels[i], dims[i], dilations)})
            else:
                self.decoder[name] = torch.nn.ModuleDict({
                    "project_conv": D.RefConv(channels[i], project[i], 1),
                    "fuse_conv": torch.nn.Sequential(D.RefConv(project[i] + dims[i + 1], dims[i], 3, padding=1),
                                                     D.RefConv(dims[i], dims[i], 3, padding=1))})

    def decode(self, features):
        y = self.decoder["res5"]["project_conv"](features["res5"])
        for name in self.names[-2::-1]:
            proj = self.decoder[name]["project_conv"](features[name])
            y = F.interpolate(y, size=proj.shape[2:], mode="bilinear", align_corners=False)
            y = self.decoder[name]["fuse_conv"](torch.cat([proj, y], dim=1))
        return y


def _two(cin, mid, cout):
    return torch.nn.Sequential(D.RefConv(cin, mid, 3, padding=1), D.RefConv(mid, cout, 3, padding=1))


class RefSemSegHead(RefDecoder):
    def __init__(self, channels, project, dims, dilations, head_channels, classes, ignore):
        super().__init__(channels, project, dims, dilations)
        self.head = _two(dims[0], dims[0], head_channels)
        self.predictor = D.RefConv(head_channels, classes, 1, norm=False, relu=False)
        self.ignore = ignore

    def forward(self, features, targets, weights, top_k):
        y = F.interpolate(self.predictor(self.head(self.decode(features))), scale_factor=4, mode="bilinear",
                          align_corners=False)
        pixel = (F.cross_entropy(y, targets, ignore_index=self.ignore, reduction="none") * weights).contiguous().view(-1)
        return pixel.mean() if top_k == 1.0 else torch.topk(pixel, int(top_k * pixel.numel()))[0].mean()


class RefInsEmbedHead(RefDecoder):
    def __init__(self, channels, project, dims, dilations, head_channels):
        super().__init__(channels, project, dims, dilations)
        self.center_head = _two(dims[0], dims[0], head_channels)
        self.center_predictor = D.RefConv(head_channels, 1, 1, norm=False, relu=False)
        self.offset_head = _two(dims[0], dims[0], head_channels)
        self.offset_predictor = D.RefConv(head_channels, 2, 1, norm=False, relu=False)

    def forward(self, features, center_targets, center_weights, offset_targets, offset_weights):
        y = self.decode(features)
        center = self.center_predictor(self.center_head(y))
        offset = self.offset_predictor(self.offset_head(y))
        return (R.center_loss(center, center_targets, center_weights, 4) * 200.0,
                R.offset_loss(offset, offset_targets, offset_weights, 4) * 0.01)


CHANNELS, PROJECT, DIMS, DILATIONS = [32, 48, 64], [8, 16], [32, 32, 32], [6, 12, 18]
SHAPES = {"res2": ShapeSpec(channels=32, stride=4), "res3": ShapeSpec(channels=48, stride=8),
          "res5": ShapeSpec(channels=64, stride=16)}


def _features():
    g = torch.Generator().manual_seed(4)
    feats = {"res2": torch.randn(2, 32, 16, 32, generator=g), "res3": torch.randn(2, 48, 8, 16, generator=g),
             "res5": torch.randn(2, 64, 4, 8, generator=g)}
    return feats, g


def _prepare(head, ref, predictors):
    with torch.no_grad():                       # norm parameters off their defaults, so that their role shows
        for m in head.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
        for p in predictors:
            p.weight.normal_(0, 0.5)
    D.load_double(ref, head.state_dict())
    head.train()


def _compare(head, ref, dev, f64):
    got_params, want_params = dict(head.named_parameters()), dict(ref.named_parameters())
    assert sorted(got_params) == sorted(want_params)
    for name, p in got_params.items():
        err = D.max_rel(p.grad, want_params[name].grad)
        print(name, err)
        assert err <= REL, (name, err)
    for k in dev:
        assert D.max_rel(dev[k].grad, f64[k].grad) <= REL, k
    for (name, b), (_, rb) in zip(head.named_buffers(), ref.named_buffers()):
        assert D.max_rel(b.double(), rb.double()) <= REL, name


def _head_kwargs():
    return dict(in_features=["res2", "res3", "res5"], project_channels=PROJECT, aspp_dilations=DILATIONS,
                aspp_dropout=0.0, decoder_channels=DIMS, common_stride=4, norm="BN", train_size=(64, 128))


def test_semantic_head_matches_the_stock_torch_restatement(cuda, f32_math):
    from jtsm_amd.layers.conv import planes_clear
    from jtsm_amd.modeling.meta_arch.panoptic_deeplab import PanopticDeepLabSemSegHead
    feats, g = _features()
    target = torch.randint(0, 5, (2, 64, 128), generator=g)
    target[:, :, 40:48] = 255
    weights = 1.0 + 2.0 * (torch.rand(2, 64, 128, generator=g) < 0.3).float()
    torch.manual_seed(2)
    # loss_top_k = 1.0: the weighted mean over all pixels — no other value reaches the kernel if `loss_top_k` is dropped
    # on the way, and no pixel sits at a cut where fp32 and fp64 may choose differently
    head = PanopticDeepLabSemSegHead(SHAPES, head_channels=24, loss_weight=1.0, loss_type="hard_pixel_mining",
                                     loss_top_k=1.0, ignore_value=255, num_classes=5, **_head_kwargs()).to(cuda)
    ref = RefSemSegHead(CHANNELS, PROJECT, DIMS, DILATIONS, 24, 5, 255)
    _prepare(head, ref, [head.predictor])
    planes_clear()
    dev = {k: v.to(cuda).contiguous(memory_format=torch.channels_last).requires_grad_(True) for k, v in feats.items()}
    _, losses = head(dev, target.to(cuda), weights.to(cuda))
    losses["loss_sem_seg"].backward()
    f64 = {k: v.double().requires_grad_(True) for k, v in feats.items()}
    want = ref(f64, target, weights.double(), 1.0)
    want.backward()
    torch.cuda.synchronize()
    assert D.max_rel(losses["loss_sem_seg"], want) <= REL
    _compare(head, ref, dev, f64)
    head.loss_type = "cross_entropy"            # the plain mean has no per-pixel weights: refused, not dropped
    with pytest.raises(ValueError):
        head({k: v.detach() for k, v in dev.items()}, target.to(cuda), weights.to(cuda))
    assert torch.isfinite(head({k: v.detach() for k, v in dev.items()}, target.to(cuda))[1]["loss_sem_seg"])
    head.eval()
    with torch.no_grad():
        logits, none = head({k: v.detach() for k, v in dev.items()})
    assert tuple(logits.shape) == (2, 5, 64, 128) and none == {}


def test_instance_head_matches_the_stock_torch_restatement(cuda, f32_math):
    from jtsm_amd.layers.conv import planes_clear
    from jtsm_amd.modeling.meta_arch.panoptic_deeplab import PanopticDeepLabInsEmbedHead
    feats, g = _features()
    center_t = torch.rand(2, 1, 64, 128, generator=g)
    center_w = (torch.rand(2, 1, 64, 128, generator=g) < 0.8).float()
    offset_t = torch.randn(2, 2, 64, 128, generator=g) * 10
    offset_w = (torch.rand(2, 1, 64, 128, generator=g) < 0.4).float()
    torch.manual_seed(3)
    head = PanopticDeepLabInsEmbedHead(SHAPES, head_channels=16, center_loss_weight=200.0, offset_loss_weight=0.01,
                                       **_head_kwargs()).to(cuda)
    ref = RefInsEmbedHead(CHANNELS, PROJECT, DIMS, DILATIONS, 16)
    _prepare(head, ref, [head.center_predictor, head.offset_predictor])
    planes_clear()
    dev = {k: v.to(cuda).contiguous(memory_format=torch.channels_last).requires_grad_(True) for k, v in feats.items()}
    _, _, lc, lo = head(dev, center_t.to(cuda), center_w.to(cuda), offset_t.to(cuda), offset_w.to(cuda))
    (lc["loss_center"] + lo["loss_offset"]).backward()
    f64 = {k: v.double().requires_grad_(True) for k, v in feats.items()}
    want_c, want_o = ref(f64, center_t, center_w, offset_t, offset_w)
    (want_c + want_o).backward()
    torch.cuda.synchronize()
    assert D.max_rel(lc["loss_center"], want_c) <= REL and D.max_rel(lo["loss_offset"], want_o) <= REL
    _compare(head, ref, dev, f64)
    head.eval()
    with torch.no_grad():
        center, offset, a, b = head({k: v.detach() for k, v in dev.items()})
    assert tuple(center.shape) == (2, 1, 64, 128) and tuple(offset.shape) == (2, 2, 64, 128) and a == {} and b == {}


# ---- the model ---------------------------------------------------------------------------------------------------------
def _step(model, cfg, seed):
    model.train()
    model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    losses = model(_batch(cfg))
    assert set(losses) == {"loss_sem_seg", "loss_center", "loss_offset"}
    loss = sum(losses.values())
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def test_two_seeded_steps_give_the_same_bits(cuda, model):
    cfg = _cfg()
    a, b = _step(model, cfg, 7), _step(model, cfg, 7)
    assert torch.isfinite(a[0]) and torch.equal(a[0], b[0])
    for name in a[1]:
        assert torch.equal(a[1][name], b[1][name]), name


def test_one_adam_step_moves_every_parameter(cuda, model):
    from jtsm_amd.solver import Adam, build_optimizer
    cfg = _cfg()
    opt = build_optimizer(cfg, model)
    assert type(opt) is Adam and len(opt.param_groups) == len(list(model.parameters()))
    _, grads = _step(model, cfg, 1)
    for name, g in grads.items():
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, name
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p, before[n]), n
        assert float((p - before[n]).abs().max()) <= 1.001 * cfg.SOLVER.BASE_LR * cfg.SOLVER.BIAS_LR_FACTOR, n


def test_inference_feeds_the_three_evaluators(cuda):
    from jtsm_amd.evaluation import (COCOEvaluator, COCOGroundTruth, COCOPanopticEvaluator, PanopticGroundTruth,
                                     SemSegEvaluator)
    cfg = _cfg()
    torch.manual_seed(5)
    model = build_model(cfg)
    with torch.no_grad():       # an untrained net predicts (almost) nothing: spread the classes and lift the heat
        model.sem_seg_head.predictor.weight.normal_(0, 0.5)
        model.ins_embed_head.center_predictor.weight.normal_(0, 0.3)
        model.ins_embed_head.center_predictor.bias.fill_(0.5)
        model.ins_embed_head.offset_predictor.weight.normal_(0, 0.5)
    model.eval()
    batch = _batch(cfg, seed=5)
    inputs = [{k: item[k] for k in ("image", "image_id", "height", "width")} for item in batch]
    with torch.no_grad():
        out = model(inputs)
    assert len(out) == 2
    things = 0
    for o in out:
        assert set(o) <= {"sem_seg", "panoptic_seg", "instances"}
        assert tuple(o["sem_seg"].shape) == (19, 64, 128) and torch.isfinite(o["sem_seg"]).all()
        pan, info = o["panoptic_seg"]
        assert pan.dtype == torch.int32 and tuple(pan.shape) == (64, 128) and info.table.shape == (len(info), 5)
        ids = set(torch.unique(pan).tolist()) - {0}
        assert ids == {s["id"] for s in info} and all((s["id"] - 1) // 1000 == s["category_id"] for s in info)
        n = sum(s["isthing"] for s in info)
        assert ("instances" in o) == (n > 0)
        if n:
            inst = o["instances"]
            assert len(inst) == n and inst.pred_masks.dtype == torch.bool and tuple(inst.pred_masks.shape) == (n, 64, 128)
            assert inst.pred_classes.tolist() == [s["category_id"] for s in info if s["isthing"]]
            assert [int(m.sum()) for m in inst.pred_masks] == [s["area"] for s in info if s["isthing"]]
            assert bool((inst.scores > 0).all()) and bool(torch.isfinite(inst.scores).all())
            boxes = inst.pred_boxes.tensor
            for m, b in zip(inst.pred_masks.cpu(), boxes.cpu()):
                yy, xx = torch.nonzero(m, as_tuple=True)
                assert b.tolist() == [float(xx.min()), float(yy.min()), float(xx.max() + 1), float(yy.max() + 1)]
        things += n
    assert things > 0
    # semantic: any finite mIoU against the generated labels
    sem = SemSegEvaluator(["c%d" % i for i in range(19)], 255,
                          {item["image_id"]: item["sem_seg"].numpy().astype(np.uint8) for item in batch})
    sem.process(inputs, out)
    assert np.isfinite(sem.evaluate()["sem_seg"]["mIoU"])
    # panoptic and instances: the prediction as its own ground truth scores 100
    pan_gt, coco_gt = PanopticGroundTruth(), COCOGroundTruth(19)
    for item, o in zip(inputs, out):
        pan, info = o["panoptic_seg"]
        pan = pan.cpu().numpy()
        dense = np.zeros(pan.shape, np.int32)
        for r, s in enumerate(info):
            dense[pan == s["id"]] = r + 1
        pan_gt.add(item["image_id"], dense, [[s["category_id"], 0] for s in info])
        if "instances" in o:
            inst = o["instances"]
            b = inst.pred_boxes.tensor.cpu().numpy().astype(np.float64)
            masks = inst.pred_masks.cpu().numpy()
            coco_gt.add(item["image_id"], inst.pred_classes.cpu().numpy(),
                        np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1), masks.sum((1, 2)),
                        np.zeros(len(inst)), masks=masks)
        else:
            coco_gt.add(item["image_id"], [], np.zeros((0, 4)), [], [], masks=np.zeros((0, 64, 128), bool))
    isthing = [c in THINGS for c in range(19)]
    pq = COCOPanopticEvaluator(pan_gt, [c if t else -1 for c, t in enumerate(isthing)],
                               [-1 if t else c for c, t in enumerate(isthing)], isthing, device=cuda)
    pq.process(inputs, out)
    res = pq.evaluate()["panoptic_seg"]
    assert abs(res["PQ"] - 100.0) < 1e-9 and abs(res["PQ_th"] - 100.0) < 1e-9 and abs(res["PQ_st"] - 100.0) < 1e-9
    coco = COCOEvaluator(coco_gt, tasks=("segm",), device=cuda)
    coco.process(inputs, out)
    segm = coco.evaluate()["segm"]
    assert abs(segm["AP"] - 100.0) < 1e-6
