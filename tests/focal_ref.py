"""Reference restatement of the focal matcher and set criterion of SMCA-DETR / Anchor DETR (utils/detr_utils.py:94-262,
meta_arch/smca_detr.py:520-713, anchor_detr.py:547-742, detr_seg.py:207-270), loop-free torch on the CPU, in the dtype of its
inputs (float64: the yardstick, pinned to the reference's own classes by tests/golden/focal_criterion.npz; float32: the kernels'
operation order), with the closed-form gradient the backward kernel uses and the seeded input recipe of the fixture.  The
inputs are never stored: tools/gen_focal_golden.py and the tests both call `inputs`.

Test infrastructure: the assignment is scipy's, as in the reference."""
import math

import torch
from scipy.optimize import linear_sum_assignment

ALPHA = 0.25
WEIGHTS = {"loss_ce": 2.0, "loss_bbox": 5.0, "loss_giou": 2.0}
COSTS = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)      # (the SMCA / Anchor DETR configs' matcher weights)
LEVELS = 3
# name -> B, Q, C, targets per image, seed, whether the logits carry bias_init_with_prob(0.01) (p near 0.01: start of training)
GOLD_CASES = {
    "a": (2, 50, 20, (5, 9), 101, True),
    "b": (3, 100, 91, (0, 17, 70), 102, True),
    "c": (2, 7, 5, (9, 3), 103, False),
    "d": (2, 9, 3, (0, 0), 104, True),
    "e": (1, 6, 130, (2,), 105, False),
    "f": (1, 5, 1, (1,), 106, False),
    "g": (2, 10, 64, (3, 4), 107, True),
    "h": (2, 10, 65, (3, 4), 108, False),
}
SECOND_SEED = {"a": 201}          # another batch of the same shape (the captured step's refill)


def weight_dict(levels=LEVELS):
    wd = dict(WEIGHTS)
    for i in range(levels - 1):
        wd.update({f"{k}_{i}": v for k, v in WEIGHTS.items()})
    return wd


def inputs(name, seed=None, dtype=torch.float64, sizes=None):
    """-> ([(logits [B, Q, C], boxes [B, Q, 4]) per level, LAST level last], targets).  Drawn in float32, so the float64 and
    the float32 runs see the same numbers."""
    B, Q, C, sz, sd, bias = GOLD_CASES[name]
    sz = sz if sizes is None else sizes
    g = torch.Generator().manual_seed(sd if seed is None else seed)
    off = -math.log((1 - 0.01) / 0.01) if bias else 0.0
    levels = []
    for _ in range(LEVELS):
        logits = torch.randn(B, Q, C, generator=g) + off
        cxcy = 0.2 + 0.6 * torch.rand(B, Q, 2, generator=g)
        wh = 0.05 + 0.3 * torch.rand(B, Q, 2, generator=g)
        levels.append((logits.to(dtype), torch.cat([cxcy, wh], -1).to(dtype)))
    targets = []
    for n in sz:
        cxcy = 0.2 + 0.6 * torch.rand(n, 2, generator=g)
        wh = 0.05 + 0.3 * torch.rand(n, 2, generator=g)
        targets.append({"labels": torch.randint(0, C, (n,), generator=g), "boxes": torch.cat([cxcy, wh], -1).to(dtype)})
    return levels, targets


def as_outputs(levels):
    return {"pred_logits": levels[-1][0], "pred_boxes": levels[-1][1],
            "aux_outputs": [{"pred_logits": l, "pred_boxes": b} for l, b in levels[:-1]]}


def xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def giou_pairwise(a, b):
    """generalized_box_iou (utils/boxes.py:85-122) of xyxy boxes [N, 4] x [M, 4]"""
    a1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    a2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = a1[:, None] + a2 - inter
    iou = inter / union
    ewh = (torch.max(a[:, None, 2:], b[:, 2:]) - torch.min(a[:, None, :2], b[:, :2])).clamp(min=0)
    area = ewh[..., 0] * ewh[..., 1]
    return iou - (area - union) / area


def matching_cost(logits, boxes, targets, cost_class=1.0, cost_bbox=1.0, cost_giou=1.0, alpha=ALPHA):
    """[B, Q, T]: the cost matrix over ALL targets of the batch (image b's block is its own columns)"""
    B, Q, _ = logits.shape
    p = logits.flatten(0, 1).sigmoid()
    ob = boxes.flatten(0, 1)
    ids = torch.cat([t["labels"] for t in targets])
    tb = torch.cat([t["boxes"] for t in targets]).to(boxes.dtype)
    neg = (1 - alpha) * (p * p) * (-(1 - p + 1e-8).log())
    pos = alpha * ((1 - p) * (1 - p)) * (-(p + 1e-8).log())
    cc = pos[:, ids] - neg[:, ids]
    d = (ob[:, None, :] - tb[None, :, :]).abs()
    cb = ((d[..., 0] + d[..., 1]) + d[..., 2]) + d[..., 3]
    cg = -giou_pairwise(xyxy(ob), xyxy(tb))
    return (cost_bbox * cb + cost_class * cc + cost_giou * cg).view(B, Q, -1)


def match(logits, boxes, targets, **kw):
    Cm = matching_cost(logits, boxes, targets, **kw)
    out, off = [], 0
    for b, t in enumerate(targets):
        n = len(t["boxes"])
        i, j = linear_sum_assignment(Cm[b, :, off:off + n].numpy())
        out.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
        off += n
    return out


def onehot(logits, targets, indices):
    t = torch.zeros_like(logits)
    for b, (i, j) in enumerate(indices):
        t[b, i, targets[b]["labels"][j]] = 1
    return t


def focal_terms(x, t, alpha=ALPHA):
    """sigmoid_focal_loss elementwise, gamma = 2; ce in binary_cross_entropy_with_logits' form"""
    p = x.sigmoid()
    ce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    p_t = p * t + (1 - p) * (1 - t)
    m = 1 - p_t
    loss = ce * (m * m)
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss


def focal_grad(x, t, alpha=ALPHA):
    """d focal_terms / dx in closed form (the backward kernel's): logs as -softplus(-+x)"""
    p = x.sigmoid()
    sp = lambda z: z.clamp(min=0) + torch.log1p(torch.exp(-z.abs()))
    a1, a0 = (alpha, 1 - alpha) if alpha >= 0 else (1.0, 1.0)
    g1 = a1 * ((1 - p) * (1 - p)) * (2 * p * -sp(-x) - (1 - p))
    g0 = a0 * (p * p) * (p - 2 * (1 - p) * -sp(x))
    return torch.where(t > 0, g1, g0)


def level_losses(logits, boxes, targets, indices, num_boxes, alpha=ALPHA, log=True):
    """one decoder level's dict (loss_ce, class_error, cardinality_error, loss_bbox, loss_giou), differentiable"""
    B, Q, C = logits.shape
    dt = logits.dtype
    t = onehot(logits, targets, indices)
    out = {"loss_ce": focal_terms(logits, t, alpha).sum() / num_boxes}
    bi = torch.cat([torch.full_like(i, b) for b, (i, _) in enumerate(indices)])
    qi = torch.cat([i for i, _ in indices])
    lab = torch.cat([tg["labels"][j] for tg, (_, j) in zip(targets, indices)])
    am = logits.detach().argmax(-1)
    # the two counted outputs are float32 in the reference whatever the inputs' dtype (accuracy: `.float()`, utils/misc.py:225;
    # loss_cardinality: `card_pred.float()`)
    if log:
        n = lab.numel()
        correct = (am[bi, qi] == lab).float().sum() if n else torch.zeros([], device=logits.device)
        out["class_error"] = 100 - (correct.mul_(100.0 / n) if n else correct)
    G = torch.tensor([float(len(tg["labels"])) for tg in targets], device=logits.device)
    out["cardinality_error"] = ((am != C - 1).sum(1).float() - G).abs().sum() / B
    sb = boxes[bi, qi]
    tb = torch.cat([tg["boxes"][j] for tg, (_, j) in zip(targets, indices)]).to(dt)
    out["loss_bbox"] = (sb - tb).abs().sum() / num_boxes
    out["loss_giou"] = (1 - torch.diag(giou_pairwise(xyxy(sb), xyxy(tb)))).sum() / num_boxes
    return out


def criterion(levels, targets, indices=None, alpha=ALPHA, costs=COSTS):
    """the whole dict over the decoder levels (last level unsuffixed, aux `_i`); indices: per level, or None = matched here"""
    num_boxes = max(float(sum(len(t["labels"]) for t in targets)), 1.0)
    order = [len(levels) - 1] + list(range(len(levels) - 1))
    out, used = {}, {}
    for n, l in enumerate(order):
        lg, bx = levels[l]
        idx = indices[l] if indices is not None else match(lg.detach(), bx.detach(), targets, alpha=ALPHA, **costs)
        used[l] = idx
        sfx = "" if n == 0 else f"_{l}"
        out.update({k + sfx: v for k, v in level_losses(lg, bx, targets, idx, num_boxes, alpha, log=n == 0).items()})
    return out, [used[l] for l in range(len(levels))]


def total(losses, wd=None):
    wd = weight_dict() if wd is None else wd
    return sum(losses[k] * wd[k] for k in losses if k in wd)
