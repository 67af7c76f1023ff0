"""numpy restatement of mi_focal_topk_postprocess (csrc/detr_topk.hip) and of the SMCA box head tail, for tests/test_gpu_detr_topk.py.

Selection: a stable sort on (key descending, flat index ascending) of the order-preserving key of the fp32 logit - NaN greatest,
-0 == +0, +-inf ordinary - then the first K.  Boxes: the fp32 arithmetic of box_cxcywh_to_xyxy, Boxes.scale and
detector_postprocess in their operation order, one rounding per operation.  Scores: float64.  No device, no torch needed.
"""
import numpy as np


def keys(logits):
    """uint32 keys of a float32 array: larger float <=> larger key"""
    u = np.ascontiguousarray(logits, dtype=np.float32).view(np.uint32).copy()
    mag = u & np.uint32(0x7FFFFFFF)
    nan = mag > np.uint32(0x7F800000)
    u[mag == 0] = 0
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[nan] = np.uint32(0xFFFFFFFF)
    return k


def select(logits, K):
    """logits [B, Q, C] float32 -> flat indices [B, K] (int64), best first"""
    B = logits.shape[0]
    k = keys(logits).reshape(B, -1).astype(np.int64)
    return np.stack([np.argsort(-k[b], kind="stable")[:K] for b in range(B)])


def sigmoid64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(x))
        return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)) + np.where(np.isnan(x), np.nan, 0.0)


def _clamp(v, hi):
    v = v.copy()
    v[v < 0] = np.float32(0)
    v[v > hi] = hi
    return v            # (NaN stays NaN, as torch.clamp)


def postprocess(logits, boxes, sizes, out_sizes, K):
    """-> dict(idx [B, K], labels, query, logit [B, K] float32, score64 [B, K] float64, boxes [B, K, 4] float32)"""
    logits = np.asarray(logits, dtype=np.float32)
    boxes = np.asarray(boxes, dtype=np.float32)
    B, Q, C = logits.shape
    idx = select(logits, K)
    q, c = idx // C, idx % C
    lg = np.take_along_axis(logits.reshape(B, -1), idx, 1)
    out = np.empty((B, K, 4), np.float32)
    half = np.float32(0.5)
    for b in range(B):
        bx = boxes[b][q[b]]
        h, w = np.float32(int(sizes[b][0])), np.float32(int(sizes[b][1]))
        x0 = (bx[:, 0] - half * bx[:, 2]) * w
        y0 = (bx[:, 1] - half * bx[:, 3]) * h
        x1 = (bx[:, 0] + half * bx[:, 2]) * w
        y1 = (bx[:, 1] + half * bx[:, 3]) * h
        if out_sizes is not None:
            oh, ow = int(out_sizes[b][0]), int(out_sizes[b][1])
            sx, sy = np.float32(ow / int(sizes[b][1])), np.float32(oh / int(sizes[b][0]))     # the quotient in double, rounded once
            x0, y0, x1, y1 = _clamp(x0 * sx, np.float32(ow)), _clamp(y0 * sy, np.float32(oh)), _clamp(x1 * sx, np.float32(ow)), _clamp(y1 * sy, np.float32(oh))
        out[b] = np.stack([x0, y0, x1, y1], 1)
    return dict(idx=idx, labels=c, query=q, logit=lg, score64=sigmoid64(lg), boxes=out)


def ulp_error(got, ref64):
    """|got - ref64| in units of the float32 spacing at ref64, elementwise (inf where exactly one side is not finite)"""
    got = np.asarray(got, dtype=np.float64)
    ref64 = np.asarray(ref64, dtype=np.float64)
    r32 = ref64.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        sp = np.spacing(np.abs(r32)).astype(np.float64)
        e = np.abs(got - ref64) / sp
    both_nan = np.isnan(got) & np.isnan(ref64)
    same_inf = np.isinf(got) & (got == ref64)
    e = np.where(both_nan | same_inf, 0.0, e)
    return np.where(np.isnan(e), np.inf, e)


def dp_sum(dx):
    """dx [L, B, Q, 4] float32 -> dp [B, Q, 2]: a float32 sum over the levels in ascending order"""
    dx = np.asarray(dx, dtype=np.float32)
    acc = np.zeros(dx.shape[1:3] + (2,), np.float32)
    for l in range(dx.shape[0]):
        acc = (acc + dx[l, :, :, :2]).astype(np.float32)
    return acc


def distinct_logits(B, Q, C, seed):
    """float32 [B, Q, C]: per image a random permutation of an evenly spaced grid inside (-8, 8), spacing >= 1e-3 - their float32
    sigmoids are pairwise distinct too (the tests assert it), so torch.topk on the probabilities has one right answer"""
    n = Q * C
    step = 15.9 / n
    assert step >= 1e-3, (Q, C)
    rng = np.random.default_rng(seed)
    return np.stack([(-7.95 + step * rng.permutation(n)).astype(np.float32).reshape(Q, C) for _ in range(B)])


def random_boxes(B, Q, seed):
    """normalised cxcywh in (0.05, 0.95): no zero sizes, some boxes reach over the image border"""
    return np.random.default_rng(seed).uniform(0.05, 0.95, (B, Q, 4)).astype(np.float32)
