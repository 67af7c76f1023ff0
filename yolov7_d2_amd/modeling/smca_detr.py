"""`SMCADetr` meta-architecture - the drop-in for yolov7/modeling/meta_arch/smca_detr.py (configs/coco/detr/smcadetr_origin.yaml):
`SMCADETR` is that file's inner `DETR` (smca_detr.py:405-517, use_focal_loss=True), `SMCADetr` the registered class around it
(smca_detr.py:38-273), with the reference's state_dict keys (detr.transformer.*, detr.class_embed, detr.bbox_embed.layers.N,
detr.query_embed, detr.input_proj, detr.backbone.0.backbone.<resnet>, criterion.empty_weight) and initialisation.

Compute: ResNet-50 (res5 is the one map taken, whatever OUT_FEATURES lists), `SMCATransformer` (modeling/smca.py), the focal
matcher and criterion (modeling/focal_criterion.py), and two pieces of csrc/detr_topk.hip:
  the box head tail  sigmoid(bbox_embed(hs) + (reference points, 0, 0))  as one launch forward and one backward
  (mi_box_ref_sigmoid_fwd / _bwd: the reference's in-place slice add, repeat and sigmoid), and
  the inference step `focal_topk_postprocess` (mi_focal_topk_postprocess): sigmoid over all Q x C logits of an image, the best
  100, their boxes gathered, converted, scaled to the image and - with `out_sizes` - detector_postprocess's scale and clip, one
  launch for the batch; Anchor DETR's PostProcess is the same rule.
The host / device split of the training step (batch_key, prepare_batch, forward_prepared, grad_cut_modules, shape_bucket,
target_capacity) is `Detr`'s, inherited: graph_step.GraphedTrainStep serves this model unchanged.

Not built, refused by name: MODEL.MASK_ON (DETRsegm), MODEL.DETR.NUM_FEATURE_LEVELS != 1 (the reference's multi-level branch hands
a ModuleList to a call and cannot run) and MODEL.DETR.PRE_NORM (its decoder's forward_pre has another signature).
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import _lib as L
from ..d2shim import META_ARCH_REGISTRY, Boxes, ImageList, Instances, detector_postprocess
from .detr import MLP, _linear
from .detr_meta import Detr, Joiner, MaskedBackbone, NestedTensor
from .focal_criterion import HungarianMatcherSMCA, SMCASetCriterion
from .position_encoding import PositionEmbeddingSine
from .smca import SMCATransformer
from .transformer import _LinearFn, _tok

TopK = namedtuple("TopK", "scores labels query boxes")


def bias_init_with_prob(prior_prob):
    """smca_detr.py:276-279"""
    return float(-np.log((1 - prior_prob) / prior_prob))


# ------------------------------------------------------------------ the two operators of csrc/detr_topk.hip
def _topk_views(buf, B, k):
    """the four outputs as views of ONE byte buffer (labels | boxes | scores | query): a caller that wants them on the host
    copies the buffer once"""
    n = B * k
    labels = buf[: 8 * n].view(torch.int64).view(B, k)
    boxes = buf[8 * n: 24 * n].view(torch.float32).view(B, k, 4)
    scores = buf[24 * n: 28 * n].view(torch.float32).view(B, k)
    query = buf[28 * n: 32 * n].view(torch.int32).view(B, k)
    return TopK(scores, labels, query, boxes)


def _topk_launch(logits, boxes, sizes_dev, out_sizes, k):
    if not (logits.is_cuda and boxes.is_cuda and sizes_dev.is_cuda and (out_sizes is None or out_sizes.is_cuda)):
        raise L.MI355Error("focal_topk_postprocess: the MI355X path needs device tensors (no CPU fallback)")
    if logits.dim() != 3 or tuple(boxes.shape) != (logits.shape[0], logits.shape[1], 4):
        raise ValueError(f"focal_topk_postprocess: logits {tuple(logits.shape)} / boxes {tuple(boxes.shape)}")
    B, Q, C = logits.shape
    for name, t in (("sizes_dev", sizes_dev), ("out_sizes", out_sizes)):
        if t is not None and (tuple(t.shape) != (B, 2) or t.dtype != torch.int64):
            raise ValueError(f"focal_topk_postprocess: {name} must be int64 [{B}, 2], got {t.dtype} {tuple(t.shape)}")
    logits, boxes = logits.float().contiguous(), boxes.float().contiguous()
    sizes_dev = sizes_dev.contiguous()
    out_sizes = None if out_sizes is None else out_sizes.contiguous()
    k = int(k)
    buf = torch.empty(32 * B * max(k, 0), dtype=torch.uint8, device=logits.device)
    v = _topk_views(buf, B, max(k, 0))
    L.check(L.lib().mi_focal_topk_postprocess(logits.data_ptr(), boxes.data_ptr(), sizes_dev.data_ptr(), L.ptr(out_sizes), B, Q, C, k,
                                              v.scores.data_ptr(), v.labels.data_ptr(), v.query.data_ptr(), v.boxes.data_ptr(),
                                              L.stream_ptr()), "mi_focal_topk_postprocess")
    return buf, v


@torch.no_grad()
def focal_topk_postprocess(logits, boxes, sizes_dev, out_sizes=None, k=100):
    """logits [B, Q, C], boxes [B, Q, 4] normalised cxcywh, sizes_dev int64 [B, 2] = (h, w), out_sizes int64 [B, 2] =
    (out_h, out_w) or None  ->  TopK(scores fp32 [B, k], labels int64 [B, k], query int32 [B, k], boxes fp32 [B, k, 4] absolute
    xyxy), best first, ties towards the lower flat index.  Without out_sizes the boxes are scaled to the image
    (SMCADetr.inference / Anchor DETR's PostProcess); with it they are also scaled by out / image and clipped
    (detector_postprocess, before its nonempty() filter).  k > Q * C raises, as torch.topk does."""
    return _topk_launch(logits, boxes, sizes_dev, out_sizes, k)[1]


class _BoxRefSigmoidFn(torch.autograd.Function):
    """(x [L, B, Q, 4], p [B, Q, 2]) -> sigmoid(x + (p, 0, 0)) in fp32"""

    @staticmethod
    def forward(ctx, x, p):
        if not (x.is_cuda and p.is_cuda):
            raise L.MI355Error("box_ref_sigmoid: the MI355X path needs device tensors (no CPU fallback)")
        Lv, B, Q, four = x.shape
        if four != 4 or tuple(p.shape) != (B, Q, 2):
            raise ValueError(f"box_ref_sigmoid: x {tuple(x.shape)} / p {tuple(p.shape)}")
        x, p = x.float().contiguous(), p.float().contiguous()
        y = torch.empty_like(x)
        L.check(L.lib().mi_box_ref_sigmoid_fwd(x.data_ptr(), p.data_ptr(), y.data_ptr(), Lv, B, Q, L.stream_ptr()),
                "mi_box_ref_sigmoid_fwd")
        ctx.save_for_backward(x, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, p = ctx.saved_tensors
        Lv, B, Q, _ = x.shape
        dy = dy.float().contiguous()
        dx, dp = torch.empty_like(x), torch.empty_like(p)
        L.check(L.lib().mi_box_ref_sigmoid_bwd(x.data_ptr(), p.data_ptr(), dy.data_ptr(), dx.data_ptr(), dp.data_ptr(), Lv, B, Q,
                                               L.stream_ptr()), "mi_box_ref_sigmoid_bwd")
        return dx, dp


def box_ref_sigmoid(x, points):
    """the SMCA box head tail: x [L, B, Q, 4] (bbox_embed of every decoder level), points [B, Q, 2] (layer 0's reference
    points before the sigmoid) -> fp32 [L, B, Q, 4]; gradients for both"""
    return _BoxRefSigmoidFn.apply(x, points)


# ------------------------------------------------------------------ the reference's inference, restated in plain torch
@torch.no_grad()
def inference_torch(box_cls, box_pred, image_sizes, out_sizes=None, k=100):
    """smca_detr.py:216-264 followed by detector_postprocess (smca_detr.py:193-197), operation for operation, on whatever device
    the tensors live (the tests run it on the CPU as the yardstick of the kernel).  image_sizes / out_sizes: (h, w) per image;
    out_sizes None = the image sizes.  -> [Instances(pred_boxes, scores, pred_classes)]"""
    assert len(box_cls) == len(image_sizes)
    box_cls, box_pred = box_cls.float(), box_pred.float()
    prob = box_cls.sigmoid()
    scores, topk_indexes = torch.topk(prob.view(box_cls.shape[0], -1), k, dim=1)
    topk_boxes = torch.div(topk_indexes, box_cls.shape[2], rounding_mode="floor")
    labels = topk_indexes % box_cls.shape[2]
    results = []
    for i, (s, l, b, image_size) in enumerate(zip(scores, labels, box_pred, image_sizes)):
        image_size = (int(image_size[0]), int(image_size[1]))
        result = Instances(image_size)
        x_c, y_c, w, h = b.unbind(-1)           # (box_cxcywh_to_xyxy of utils/boxes.py, as plain torch)
        xyxy = torch.stack([(x_c - 0.5 * w), (y_c - 0.5 * h), (x_c + 0.5 * w), (y_c + 0.5 * h)], dim=-1)
        boxes = torch.gather(xyxy, 0, topk_boxes[i].unsqueeze(-1).repeat(1, 4))
        result.pred_boxes = Boxes(boxes)
        result.pred_boxes.scale(scale_x=image_size[1], scale_y=image_size[0])
        result.scores = s
        result.pred_classes = l
        oh, ow = image_size if out_sizes is None else (int(out_sizes[i][0]), int(out_sizes[i][1]))
        results.append(detector_postprocess(result, oh, ow))
    return results


# ------------------------------------------------------------------ the model
class MaskedBackboneRes5(MaskedBackbone):
    """smca_detr.py:282-402 with num_feature_levels 1: of the maps the backbone returns only res5 goes on (the reference YAML
    lists res2 - res5), with its padding mask"""
    level = "res5"

    def __init__(self, cfg):
        super().__init__(cfg)
        shape = self.backbone.output_shape()[self.level]
        self.feature_strides = [shape.stride]
        self.strides = [shape.stride]
        self.num_channels = [shape.channels]
        self.return_interm_layers = [self.level]

    def forward(self, images):
        tensor = images.tensor if isinstance(images, ImageList) else images.tensors
        feat = self.backbone(tensor)[self.level]
        if isinstance(images, ImageList) and getattr(images, "sizes_dev", None) is not None:
            mask = self.mask_out_padding_dev([feat.shape], images.sizes_dev)[0]
        elif isinstance(images, ImageList):
            mask = self.mask_out_padding([feat.shape], images.image_sizes, tensor.device)[0]
        else:       # a NestedTensor carries its own pixel mask: nearest down-sampling, as in MaskedBackbone
            mask = F.interpolate(images.mask[None].float(), size=feat.shape[-2:]).to(torch.bool)[0]
        return {self.level: NestedTensor(feat, mask)}


class SMCADETR(nn.Module):
    """smca_detr.py:405-517"""

    def __init__(self, backbone, transformer, num_classes, num_queries, num_feature_levels=1, aux_loss=False, use_focal_loss=True):
        super().__init__()
        if num_feature_levels != 1:
            raise NotImplementedError("SMCADETR: MODEL.DETR.NUM_FEATURE_LEVELS != 1 is not served (the reference's multi-level "
                                      "branch cannot run: it calls a ModuleList)")
        self.num_queries = num_queries
        self.transformer = transformer
        hidden_dim = transformer.d_model
        self.class_embed = nn.Linear(hidden_dim, num_classes if use_focal_loss else num_classes + 1)
        nn.init.constant_(self.class_embed.bias, bias_init_with_prob(0.01))
        self.bbox_embed = MLP(hidden_dim, hidden_dim, 4, 3)
        self.query_embed = nn.Embedding(num_queries, hidden_dim)
        self.input_proj = nn.Conv2d(backbone.num_channels[-1], hidden_dim, kernel_size=1)
        self.backbone = backbone
        self.aux_loss = aux_loss

    def forward(self, samples):
        features, pos = self.backbone(samples)
        src, mask = features[-1].decompose()
        assert mask is not None
        if not src.is_cuda:
            raise L.MI355Error("SMCADETR: the MI355X path needs device tensors (no CPU fallback)")
        # h_w [1, B, 2] = (width, height) of every image.  From the device copy of the sizes when the batch was prepared
        # (Detr.prepare_batch): no host value of the batch enters a launch and a captured step serves every batch of its shape
        sizes_dev = getattr(samples, "sizes_dev", None)
        if sizes_dev is None:
            sizes_dev = torch.tensor([[int(h), int(w)] for h, w in samples.image_sizes], dtype=torch.int64).to(src.device)
        h_w = sizes_dev.flip(-1).unsqueeze(0)
        proj = _input_proj(self.input_proj, src)
        hs, points = self.transformer(proj, mask, self.query_embed.weight, pos[-1], h_w)
        outputs_class = _linear(hs, self.class_embed).float()
        outputs_coord = box_ref_sigmoid(self.bbox_embed(hs), points)
        out = {"pred_logits": outputs_class[-1], "pred_boxes": outputs_coord[-1]}
        if self.aux_loss:
            out["aux_outputs"] = [{"pred_logits": a, "pred_boxes": b} for a, b in zip(outputs_class[:-1], outputs_coord[:-1])]
        return out


def _input_proj(conv, src):
    """DETR.forward's input projection (modeling/detr.py): the 1x1 conv with bias as a linear over the pixel rows, read in place
    from the backbone's channels_last memory"""
    B, Cc, H, W = src.shape
    tok = _tok(src.permute(0, 2, 3, 1)).reshape(B * H * W, Cc)
    w = conv.weight.view(conv.out_channels, Cc)
    if Cc % 32:
        tok, w = F.pad(tok, (0, -Cc % 32)), F.pad(w, (0, -Cc % 32))
    proj = _LinearFn.apply(tok, w, conv.bias)
    return proj.reshape(B, H, W, -1).permute(0, 3, 1, 2)


@META_ARCH_REGISTRY.register()
class SMCADetr(Detr):
    max_detections = 100          # the reference's fixed top-100 (smca_detr.py:233)

    def __init__(self, cfg):
        nn.Module.__init__(self)
        self.device = torch.device(cfg.MODEL.DEVICE)
        self.conf_thresh = cfg.MODEL.YOLO.CONF_THRESHOLD
        self.ignore_thresh = cfg.MODEL.YOLO.IGNORE_THRESHOLD
        self.num_classes = cfg.MODEL.DETR.NUM_CLASSES
        self.mask_on = cfg.MODEL.MASK_ON
        d = cfg.MODEL.DETR
        if self.mask_on:
            raise NotImplementedError("SMCADetr: MODEL.MASK_ON (DETRsegm mask head) is not on this path")
        if d.NUM_FEATURE_LEVELS != 1:
            raise NotImplementedError(f"SMCADetr: MODEL.DETR.NUM_FEATURE_LEVELS = {d.NUM_FEATURE_LEVELS} is not served (the "
                                      "reference's multi-level branch cannot run: it calls a ModuleList)")
        if d.PRE_NORM:
            raise NotImplementedError("SMCADetr: MODEL.DETR.PRE_NORM is not served (the reference's decoder cannot call its "
                                      "forward_pre)")
        self.num_queries = d.NUM_OBJECT_QUERIES
        deep_supervision = d.DEEP_SUPERVISION
        d2_backbone = MaskedBackboneRes5(cfg)
        backbone = Joiner(d2_backbone, PositionEmbeddingSine(d.HIDDEN_DIM // 2, normalize=True))
        backbone.num_channels = d2_backbone.num_channels
        transformer = SMCATransformer(d_model=d.HIDDEN_DIM, dropout=d.DROPOUT, nhead=d.NHEADS, dim_feedforward=d.DIM_FEEDFORWARD,
                                      num_encoder_layers=d.ENC_LAYERS, num_decoder_layers=d.DEC_LAYERS, normalize_before=d.PRE_NORM,
                                      return_intermediate_dec=deep_supervision, dynamic_scale="type3")
        self.detr = SMCADETR(backbone, transformer, num_classes=self.num_classes, num_queries=self.num_queries,
                             num_feature_levels=d.NUM_FEATURE_LEVELS, aux_loss=deep_supervision)
        matcher = HungarianMatcherSMCA(cost_class=1, cost_bbox=d.L1_WEIGHT, cost_giou=d.GIOU_WEIGHT)
        weight_dict = {"loss_ce": 2, "loss_bbox": d.L1_WEIGHT, "loss_giou": d.GIOU_WEIGHT}
        if deep_supervision:
            aux = {}
            for i in range(d.DEC_LAYERS - 1):
                aux.update({k + f"_{i}": v for k, v in weight_dict.items()})
            weight_dict.update(aux)
        self.criterion = SMCASetCriterion(self.num_classes, matcher=matcher, weight_dict=weight_dict, eos_coef=d.NO_OBJECT_WEIGHT,
                                          losses=["labels", "boxes", "cardinality"])
        self.register_buffer("pixel_mean", torch.Tensor(cfg.MODEL.PIXEL_MEAN).view(3, 1, 1), persistent=False)
        self.register_buffer("pixel_std", torch.Tensor(cfg.MODEL.PIXEL_STD).view(3, 1, 1), persistent=False)
        self.pixel_mean_host, self.pixel_std_host = [float(v) for v in cfg.MODEL.PIXEL_MEAN], [float(v) for v in cfg.MODEL.PIXEL_STD]
        self.normalizer = lambda x: (x - self.pixel_mean) / self.pixel_std
        self.iter = 0
        self.to(self.device)

    def forward(self, batched_inputs):
        if self.device.type != "cuda":
            raise L.MI355Error(f"SMCADetr on MODEL.DEVICE={self.device}: the MI355X path needs a HIP device (no CPU fallback)")
        images = self.preprocess_image(batched_inputs)
        output = self.detr(images)
        if self.training:
            gt_instances = [x["instances"].to(self.device) for x in batched_inputs]
            targets = self.prepare_targets(gt_instances)
            loss_dict = self.criterion(output, targets)
            weight_dict = self.criterion.weight_dict
            # (smca_detr.py:178-185: only the weighted entries are returned, the *_error statistics are dropped)
            return {k: v * weight_dict[k] for k, v in loss_dict.items() if k in weight_dict}
        out_sizes = [(int(inp.get("height", s[0])), int(inp.get("width", s[1]))) for inp, s in zip(batched_inputs, images.image_sizes)]
        results = self.inference(output["pred_logits"], output["pred_boxes"], images.image_sizes, out_sizes)
        return [{"instances": r} for r in results]

    def inference(self, box_cls, box_pred, image_sizes, out_sizes=None):
        """smca_detr.py:216-264 + detector_postprocess: one launch for the batch and one read-back; detector_postprocess's
        nonempty() filter runs on the host copy.  -> [Instances(pred_boxes, scores, pred_classes)] of host tensors, in the
        reference's order (best first)"""
        assert len(box_cls) == len(image_sizes)
        B = len(image_sizes)
        out_sizes = [tuple(s) for s in image_sizes] if out_sizes is None else out_sizes
        host = torch.tensor([[int(h), int(w)] for h, w in image_sizes] + [[int(h), int(w)] for h, w in out_sizes], dtype=torch.int64)
        dev = host.to(box_cls.device)
        buf, _ = _topk_launch(box_cls, box_pred, dev[:B], dev[B:], self.max_detections)
        v = _topk_views(buf.cpu(), B, self.max_detections)
        results = []
        for i in range(B):
            r = Instances((int(out_sizes[i][0]), int(out_sizes[i][1])))
            r.pred_boxes = Boxes(v.boxes[i])
            r.scores = v.scores[i]
            r.pred_classes = v.labels[i]
            results.append(r[r.pred_boxes.nonempty()])
        return results

    inference_torch = staticmethod(inference_torch)
