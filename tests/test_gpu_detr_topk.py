"""GPU (-m gpu): csrc/detr_topk.hip exactly.  mi_focal_topk_postprocess against its numpy restatement tests/topk_ref.py (a stable
sort on (key descending, index ascending)): labels, query and order equal, boxes bit-equal, on every path of the kernel (keys in
registers / re-read, Q * C == K, K = 1, K = 1000) and on inputs built to tie: all equal, a block of duplicates straddling the
K-th place, {-inf, -0, +0, +inf, NaN} sprinkled in, eight distinct values.  Scores and the box head tail are held to float64: no
fixed tolerance - the bound is what torch's own fp32 composition deviates from float64 on the same inputs on the same device, or
1 ulp, whichever is larger, and it is printed."""
import numpy as np
import pytest
import torch

import topk_ref as R
from yolov7_d2_amd import _lib as L
from yolov7_d2_amd.modeling import box_ref_sigmoid, focal_topk_postprocess

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [(2, 30, 80, 100), (1, 3, 40, 100), (1, 10, 10, 100), (5, 300, 91, 100), (1, 900, 91, 100), (3, 7, 13, 1), (2, 37, 29, 64),
         (2, 37, 29, 1000)]
FAMILIES = ["distinct", "equal", "straddle", "special", "eight"]


def _logits(family, B, Q, C, K, seed):
    rng = np.random.default_rng(seed)
    n = Q * C
    if family == "distinct":
        x = ((np.stack([rng.permutation(n) for _ in range(B)]) - n / 2) * (24.0 / n)).astype(np.float32)      # distinct, inside (-12, 12)
        assert all(len(np.unique(r)) == n for r in x)
    elif family == "equal":
        x = np.full((B, n), -1.25, np.float32)
    elif family == "straddle":        # K // 2 larger values, then duplicates of one value well past the K-th place, then smaller ones
        x = rng.standard_normal((B, n)).astype(np.float32) - np.float32(10)
        for b in range(B):
            p = rng.permutation(n)
            x[b, p[: K // 2]] = np.float32(5) + rng.random(K // 2).astype(np.float32)
            x[b, p[K // 2: min(n, K // 2 + K + 7)]] = np.float32(2.5)
    elif family == "special":
        x = rng.standard_normal((B, n)).astype(np.float32)
        sp = np.array([-np.inf, -0.0, 0.0, np.inf, np.nan], np.float32)
        m = rng.random((B, n)) < 0.3
        x[m] = sp[rng.integers(0, 5, int(m.sum()))]
    else:
        x = rng.integers(0, 8, (B, n)).astype(np.float32) * np.float32(0.75) - np.float32(3)
    return x.reshape(B, Q, C)


def _sizes(B, seed, mode):
    rng = np.random.default_rng(seed)
    sizes = np.stack([rng.integers(64, 1400, B), rng.integers(64, 1400, B)], 1).astype(np.int64)
    if mode == "none":
        return sizes, None
    if mode == "smaller":         # an output smaller than the image and than many boxes: the clip acts
        return sizes, np.stack([sizes[:, 0] // 3 + 1, sizes[:, 1] // 2 + 3], 1).astype(np.int64)
    return sizes, np.stack([sizes[:, 0] * 2 + 1, sizes[:, 1] * 3 - 2], 1).astype(np.int64)


def _run(lg, bx, sizes, outs, K):
    t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    r = focal_topk_postprocess(t(lg), t(bx), t(sizes), t(outs), k=K)
    torch.cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


def _torch_sigmoid_bound(x32, ref64):
    """torch.sigmoid's own largest deviation from float64 on these inputs on this device, in float32 ulps, or 1 ulp"""
    own = torch.sigmoid(torch.from_numpy(np.ascontiguousarray(x32)).to(DEV)).cpu().numpy()
    return max(float(R.ulp_error(own, ref64).max()), 1.0)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,Q,C,K", CASES)
def test_topk_equals_the_numpy_restatement(B, Q, C, K, family):
    seed = 1000 * FAMILIES.index(family) + Q + C + K
    lg = _logits(family, B, Q, C, K, seed)
    bx = R.random_boxes(B, Q, seed + 1)
    worst = 0.0
    for mode in ("none", "smaller", "larger"):
        sizes, outs = _sizes(B, seed + 2, mode)
        ref = R.postprocess(lg, bx, sizes, outs, K)
        got = _run(lg, bx, sizes, outs, K)
        assert got["labels"].dtype == np.int64 and got["query"].dtype == np.int32
        assert np.array_equal(got["query"].astype(np.int64) * C + got["labels"], ref["idx"]), (mode, "selection / order")
        assert np.array_equal(got["labels"], ref["labels"]) and np.array_equal(got["query"], ref["query"])
        assert np.array_equal(got["boxes"].view(np.uint32), ref["boxes"].view(np.uint32)), (mode, "boxes")
        if mode == "smaller" and family == "distinct" and K >= 64 and Q >= 30:      # (enough boxes for one to reach over the border)
            assert (got["boxes"][..., 2] == outs[:, None, 1]).any() or (got["boxes"][..., 3] == outs[:, None, 0]).any()   # the clip acted
        err = R.ulp_error(got["scores"], ref["score64"])
        bound = _torch_sigmoid_bound(ref["logit"], ref["score64"])
        worst = max(worst, float(err.max()))
        assert err.max() <= bound, (mode, float(err.max()), bound)
    if family == "equal":
        assert np.array_equal(ref["idx"], np.tile(np.arange(K), (B, 1)))
    print(f"topk {B, Q, C, K} {family}: score error {worst:.3f} ulp (bound: torch.sigmoid's own {bound:.3f})")


@pytest.mark.parametrize("B,Q,C,K", [(2, 30, 80, 100), (1, 3, 40, 100), (3, 7, 13, 1), (2, 37, 29, 64), (2, 37, 29, 1000)])
def test_topk_equals_torch_topk_on_distinct_probabilities(B, Q, C, K):
    lg = R.distinct_logits(B, Q, C, seed=Q * C + K)
    prob = torch.from_numpy(lg).to(DEV).sigmoid().flatten(1)
    assert all(len(torch.unique(p)) == p.numel() for p in prob)         # (also holds for the CPU's sigmoid: tests/test_smcadetr_ref.py)
    sizes, _ = _sizes(B, 5, "none")
    got = _run(lg, R.random_boxes(B, Q, 3), sizes, None, K)
    idx = torch.topk(prob, K, dim=1)[1].cpu().numpy()
    assert np.array_equal(got["query"].astype(np.int64) * C + got["labels"], idx)


def test_topk_is_reproducible_and_refuses_k_above_qc():
    lg, bx = _logits("eight", 4, 300, 91, 100, 7), R.random_boxes(4, 300, 8)
    sizes, outs = _sizes(4, 9, "smaller")
    a, b = _run(lg, bx, sizes, outs, 100), _run(lg, bx, sizes, outs, 100)
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)
    t = torch.zeros(1, 3, 40, device=DEV)
    with pytest.raises(L.MI355Error, match="K 121 > Q"):
        focal_topk_postprocess(t, torch.zeros(1, 3, 4, device=DEV), torch.ones(1, 2, dtype=torch.int64, device=DEV), k=121)
    with pytest.raises(RuntimeError):
        torch.topk(t.flatten(1), 121)                                   # the rule the refusal restates


# ------------------------------------------------------------------ the box head tail
def _tail_inputs(Lv, B, Q):
    g = torch.Generator().manual_seed(17 * Lv + B + Q)
    x = torch.randn(Lv, B, Q, 4, generator=g) * 2.5
    p = torch.randn(B, Q, 2, generator=g) * 1.5
    dy = torch.randn(Lv, B, Q, 4, generator=g)
    return x, p, dy


def _composition(x, p, dy):
    """smca_detr.py:500-503 and its autograd backward, in the tensors' dtype and on their device"""
    x, p = x.clone().requires_grad_(True), p.clone().requires_grad_(True)
    coord = x + 0
    coord[..., :2] = coord[..., :2] + p.unsqueeze(0).repeat(x.shape[0], 1, 1, 1)
    y = coord.sigmoid()
    y.backward(dy)
    return y.detach(), x.grad, p.grad


@pytest.mark.parametrize("Lv,B,Q", [(1, 1, 1), (2, 2, 9), (6, 4, 300)])
def test_box_head_tail_against_float64(Lv, B, Q):
    x, p, dy = _tail_inputs(Lv, B, Q)
    ref = [t.numpy() for t in _composition(x.double(), p.double(), dy.double())]
    own = [t.cpu().numpy() for t in _composition(x.to(DEV), p.to(DEV), dy.to(DEV))]          # torch's fp32 composition, same device
    xd, pd = x.to(DEV).requires_grad_(True), p.to(DEV).requires_grad_(True)
    y = box_ref_sigmoid(xd, pd)
    y.backward(dy.to(DEV))
    got = [y.detach().cpu().numpy(), xd.grad.cpu().numpy(), pd.grad.cpu().numpy()]
    xd2, pd2 = x.to(DEV).requires_grad_(True), p.to(DEV).requires_grad_(True)
    box_ref_sigmoid(xd2, pd2).backward(dy.to(DEV))
    assert torch.equal(xd2.grad, xd.grad) and torch.equal(pd2.grad, pd.grad)                  # the backward twice: same bits
    assert np.array_equal(got[2].view(np.uint32), R.dp_sum(got[1]).view(np.uint32))            # dp: fp32 sum, l ascending
    for name, g_, o_, r_ in zip(("y", "dx", "dp"), got, own, ref):
        err, bound = float(R.ulp_error(g_, r_).max()), max(float(R.ulp_error(o_, r_).max()), 1.0)
        print(f"box head tail {Lv, B, Q} {name}: {err:.3f} ulp (bound: the torch composition's own {bound:.3f})")
        assert err <= bound, (name, err, bound)
