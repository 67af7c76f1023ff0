"""The focal matcher and set criterion of SMCA-DETR and Anchor DETR - drop-ins for HungarianMatcherSMCA /
HungarianMatcherAnchorDETR (yolov7/utils/detr_utils.py:94-262, the same computation twice) and for SetCriterion of
yolov7/modeling/meta_arch/smca_detr.py:520-713 and anchor_detr.py:547-742.

Against the DETR pair (detr_matcher.HungarianMatcher, detr_criterion.SetCriterion) three things differ: the class cost of the
matching and the classification loss are the sigmoid focal loss over num_classes channels - there is NO no-object channel, a
row's one-hot target is 1 only at its matched label - and `cardinality_error` counts the rows whose arg max is not the LAST
channel of that head (the reference's own convention, smca_detr.py:587-588 / anchor_detr.py:607: restated, not fixed).  The two
families' loss_ce agree: smca sums the focal terms and divides by num_boxes (mode "box"), anchor takes mean(1).sum() / num_boxes
* Q.  Everything else - call forms (eager host lists, PackedTargets per level, weighted_packed for a captured step), return
layouts, launch counts per level (matching: cost + assignment; loss: rows + reduction; backward: one) - is the DETR pair's,
inherited; libmi355det: mi_hungarian_match_focal, mi_focal_set_loss_fwd / _bwd.

'masks' (DETRsegm's mask losses) is out of this path's scope and raises, as in SetCriterion.
"""
import torch

from .. import _lib as L
from .detr_criterion import SetCriterion, set_loss_backward, set_loss_forward
from .detr_matcher import HungarianMatcher


class HungarianMatcherFocal(HungarianMatcher):
    """same constructor, forward / match_device / match_device_levels contracts and return layouts as HungarianMatcher; the
    class cost is alpha (1 - p)^2 (-log(p + 1e-8)) - (1 - alpha) p^2 (-log(1 - p + 1e-8)) at p = sigmoid(logit[label]).
    A NaN / inf cost raises ValueError in forward (nmatch < 0), as scipy does in the reference."""
    alpha = 0.25        # fixed in both reference matchers

    def _launch(self, logits, boxes, tl, tb, off, bs, nq, nc, gmax, cost, mq, mt, nm, what):
        L.check(L.lib().mi_hungarian_match_focal(logits.data_ptr(), boxes.data_ptr(), tl.data_ptr(), tb.data_ptr(),
                                                 off.data_ptr(), bs, nq, nc, gmax, float(self.cost_class),
                                                 float(self.cost_bbox), float(self.cost_giou), float(self.alpha),
                                                 cost.data_ptr(), mq.data_ptr(), mt.data_ptr(), nm.data_ptr(), L.stream_ptr()),
                "mi_hungarian_match_focal" + what)


HungarianMatcherSMCA = HungarianMatcherFocal
HungarianMatcherAnchorDETR = HungarianMatcherFocal


class _FocalSetLossFn(torch.autograd.Function):
    """(logits, boxes) -> tensor[5] = loss_ce, class_error, cardinality_error, loss_bbox, loss_giou"""

    @staticmethod
    def forward(ctx, logits, boxes, m, alpha, num_boxes):
        return set_loss_forward(ctx, logits, boxes, m, alpha, num_boxes,
                                ("mi_focal_loss_desc", "alpha", "mi_focal_set_loss_fwd", "mi_focal_set_loss_bwd"))

    @staticmethod
    def backward(ctx, g):
        return set_loss_backward(ctx, g)


class FocalSetCriterion(SetCriterion):
    """Anchor DETR's constructor (anchor_detr.py:554); no parameters or buffers, like the reference's.  focal_alpha < 0: no
    alpha weighting (the reference's `if alpha >= 0`)."""
    channels_extra, ce_per_box = 0, True

    def __init__(self, num_classes, matcher, weight_dict, losses, focal_alpha=0.25):
        torch.nn.Module.__init__(self)
        self.num_classes, self.matcher, self.weight_dict, self.losses, self.focal_alpha = (num_classes, matcher, weight_dict,
                                                                                         losses, focal_alpha)
        for l_ in losses:
            if l_ == "masks":
                raise NotImplementedError("FocalSetCriterion: 'masks' losses (DETR segmentation variant) are out of scope")
            assert l_ in ("labels", "cardinality", "boxes"), f"do you really want to compute {l_} loss?"

    def _set_loss(self, logits, boxes, m, num_boxes):
        return _FocalSetLossFn.apply(logits, boxes, m, self.focal_alpha, num_boxes)

    @staticmethod
    def _weigh(V, w, s):
        return (V * s) * w      # the per-level order (value / num_boxes, then the weight): the two packed forms agree bit for bit


class SMCASetCriterion(FocalSetCriterion):
    """SMCA's constructor (smca_detr.py:527): alpha is sigmoid_focal_loss_with_mode's default 0.25; `empty_weight` is registered
    for state_dict compatibility and, like eos_coef, otherwise unused - as in the reference"""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses):
        super().__init__(num_classes, matcher, weight_dict, losses, focal_alpha=0.25)
        self.eos_coef = eos_coef
        empty_weight = torch.ones(num_classes + 1)
        empty_weight[-1] = eos_coef
        self.register_buffer("empty_weight", empty_weight)
