"""The focal set criterion of SMCA-DETR / Anchor DETR over six decoder levels, forward + backward, two forms on the device,
interleaved in one process:

  fused       FocalSetCriterion.weighted_packed on PackedTargets: one mi_hungarian_match_focal launch pair for all levels, then per
              level mi_focal_set_loss_fwd (rows + reduction) and, in the backward, mi_focal_set_loss_bwd;
  composition the float32 torch composition of the same arithmetic with tests/focal_ref.py's formulas (cost matrix, one-hot target,
              sigmoid focal loss, arg-max counts, L1, GIoU; autograd for the backward).  Its assignment comes from mi_lsap on its own
              cost matrix, so both sides pay for the same assignment; the number of targets per image is a host value on both sides
              (no device-to-host copy in either).

Also timed alone: the matching of all levels (cost + assignment), the assignment alone on the same costs (mi_lsap; the cost launch
alone is not measured: it is the difference at most), one level's loss forward and one level's loss backward.
Shapes: B 4, Q 300, C 91 and B 4, Q 100, C 80, 8 to 40 targets per image.  HIP events around 10 back-to-back calls, median of 7
windows after a warm-up, the forms alternating window by window.

  python tools/focal_criterion_probe.py [--out profiles/focal_criterion_probe.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch                        # noqa: E402

SHAPES = [(4, 300, 91, (8, 40, 17, 29)), (4, 100, 80, (8, 40, 17, 29))]
LEVELS, CAP = 6, 48


def window(fn, n=10):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / n


def interleaved(fns, reps=7):
    """median us of each of fns: their windows alternate"""
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(ts, fns):
            t.append(window(f))
    return [statistics.median(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focal_criterion_probe.txt"))
    args = ap.parse_args()
    import focal_ref as R
    from yolov7_d2_amd import _lib as L
    from yolov7_d2_amd.modeling import FocalSetCriterion, HungarianMatcherFocal
    from yolov7_d2_amd.modeling.detr_matcher import PackedTargets
    from yolov7_d2_amd.modeling.focal_criterion import _FocalSetLossFn
    dev = "cuda"
    wd = R.weight_dict(LEVELS)
    lines = [f"focal set criterion, {LEVELS} decoder levels, forward + backward: fused (weighted_packed) vs the float32 torch composition of "
             f"the same arithmetic (assignment by mi_lsap on both sides); {torch.cuda.get_device_name(0)}",
             "times: microseconds per call, median of 7 interleaved windows of 10 calls; x = composition / fused",
             f"{'B':>2} {'Q':>4} {'C':>3} | {'fused':>8} {'compos.':>9} {'x':>6} | {'match all':>9} {'lsap all':>9} {'loss fwd':>9} {'loss bwd':>9} | "
             "|total fused - composition| / |composition|"]
    slower = []
    for B, Q, C, sizes in SHAPES:
        g = torch.Generator().manual_seed(Q * 1000 + C)
        box = lambda *s: torch.cat([0.2 + 0.6 * torch.rand(*s, 2, generator=g), 0.05 + 0.3 * torch.rand(*s, 2, generator=g)], -1)
        levels = [((torch.randn(B, Q, C, generator=g) - 4.595).to(dev).requires_grad_(True), box(B, Q).to(dev).requires_grad_(True))
                  for _ in range(LEVELS)]
        targets = [{"labels": torch.randint(0, C, (n,), generator=g).to(dev), "boxes": box(n).to(dev)} for n in sizes]
        off = [0]
        for n in sizes:
            off.append(off[-1] + n)
        pt = PackedTargets(targets, CAP, torch.tensor(off, dtype=torch.int32, device=dev), torch.zeros(B * CAP, dtype=torch.int64, device=dev),
                           torch.zeros(B * CAP, 4, device=dev), torch.tensor([1.0 / off[-1]], device=dev), levels=LEVELS)
        labels, boxes = torch.cat([t["labels"] for t in targets]), torch.cat([t["boxes"] for t in targets])
        pt.tgt_labels[:off[-1]].copy_(labels)
        pt.tgt_boxes[:off[-1]].copy_(boxes)
        pt.fill_levels(off, labels.cpu(), boxes.cpu())
        matcher = HungarianMatcherFocal(**R.COSTS)
        crit = FocalSetCriterion(C, matcher, wd, ["labels", "boxes", "cardinality"])
        outputs = R.as_outputs(levels)
        leaves = [t for lv in levels for t in lv]

        def fused():
            return torch.autograd.grad(crit.weighted_packed(outputs, pt)["total"], leaves)

        toff = torch.tensor(off, dtype=torch.int32, device=dev)

        def lsap(cost):
            mq = torch.empty(cost.shape[0], CAP, dtype=torch.int64, device=dev)
            mt = torch.empty(cost.shape[0], CAP, dtype=torch.int64, device=dev)
            nm = torch.zeros(cost.shape[0], dtype=torch.int32, device=dev)
            L.check(L.lib().mi_lsap(cost.data_ptr(), toff.data_ptr() if cost.shape[0] == B else pt.lv["off"].data_ptr(), cost.shape[0], Q, CAP,
                                    mq.data_ptr(), mt.data_ptr(), nm.data_ptr(), L.stream_ptr()), "mi_lsap")
            return mq, mt

        def composition():
            losses = {}
            order = [LEVELS - 1] + list(range(LEVELS - 1))
            for n, l in enumerate(order):
                lg, bx = levels[l]
                with torch.no_grad():
                    cm = R.matching_cost(lg, bx, targets, **R.COSTS)
                    cost = torch.zeros(B, Q, CAP, device=dev)
                    for b in range(B):
                        cost[b, :, :sizes[b]] = cm[b, :, off[b]:off[b + 1]]
                    mq, mt = lsap(cost)
                idx = [(mq[b, :sizes[b]], mt[b, :sizes[b]]) for b in range(B)]
                sfx = "" if n == 0 else f"_{l}"
                losses.update({k + sfx: v for k, v in R.level_losses(lg, bx, targets, idx, float(off[-1]), log=n == 0).items()})
            tot = R.total(losses, wd)
            return torch.autograd.grad(tot, leaves), tot.detach()

        tf, tc = interleaved([fused, lambda: composition()[0]])
        lv_list = [{"pred_logits": l, "pred_boxes": b} for l, b in levels]
        ms = matcher.match_device_levels(lv_list, pt)
        cost_all = torch.zeros(LEVELS * B, Q, CAP, device=dev)      # the same costs, for the assignment alone
        with torch.no_grad():
            for l, (lg, bx) in enumerate(levels):
                cm = R.matching_cost(lg, bx, targets, **R.COSTS)
                for b in range(B):
                    cost_all[l * B + b, :, :sizes[b]] = cm[b, :, off[b]:off[b + 1]]
        lg0, bx0 = levels[-1]
        out0 = _FocalSetLossFn.apply(lg0, bx0, ms[-1], R.ALPHA, 1.0)
        gsum = torch.ones(5, device=dev)
        tm, tl, tfw, tbw = interleaved([lambda: matcher.match_device_levels(lv_list, pt), lambda: lsap(cost_all),
                                        lambda: _FocalSetLossFn.apply(lg0, bx0, ms[-1], R.ALPHA, 1.0),
                                        lambda: torch.autograd.grad(out0, [lg0, bx0], gsum, retain_graph=True)])
        a, b = float(crit.weighted_packed(outputs, pt)["total"].detach()), float(composition()[1])
        lines.append(f"{B:>2} {Q:>4} {C:>3} | {tf:>8.1f} {tc:>9.1f} {tc / tf:>6.1f} | {tm:>9.1f} {tl:>9.1f} {tfw:>9.1f} {tbw:>9.1f} | {abs(a - b) / abs(b):.1e}")
        if tf > tc:
            slower.append(f"B {B} Q {Q} C {C}: fused {tf:.1f} us > composition {tc:.1f} us")
    lines.append("('lsap all': mi_lsap for all levels on the same costs; the cost launch alone was not measured - match all minus lsap all "
                 "bounds it)")
    lines.append("slower than the composition: " + ("; ".join(slower) if slower else "nowhere"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
