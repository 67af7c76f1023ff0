"""Writes tests/golden/focal_criterion.npz from the reference's OWN HungarianMatcherSMCA / HungarianMatcherAnchorDETR
(yolov7/utils/detr_utils.py) and SetCriterion of meta_arch/smca_detr.py and meta_arch/anchor_detr.py, loaded by path through
oracle/ref_loader.py's stubs (needs the reference tree), in float64 on the CPU.

The inputs are NOT stored: they are the seeded recipe of tests/focal_ref.py (GOLD_CASES, three decoder levels).  Stored per
case, for each of the two families ("smca", "anchor"): the match index pairs per level and image, every entry of the loss dict,
the total under focal_ref.weight_dict() and the gradients of that total with respect to every level's logits and boxes.  Case a
is also stored for its second seed ("a2": what the captured step is refilled with).
For every case and level the reference matcher must give the same pairs in float32 as in float64 (asserted here: that is what
lets the GPU tests demand the pairs exactly); a case that fails gets another seed in focal_ref.GOLD_CASES.
Data only; the tests never read the reference.

    python tools/gen_focal_golden.py
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_loader  # noqa: E402
import focal_ref as R  # noqa: E402


def load_reference():
    r = ref_loader.load()
    ref_loader.load_detr()
    # the two meta-arch files also import alfred.dl.torch.common.device
    ref_loader._stub("alfred.dl").__path__ = []
    ref_loader._stub("alfred.dl.torch").__path__ = []
    ref_loader._stub("alfred.dl.torch.common", device=torch.device("cpu"))
    smca = importlib.import_module("yolov7.modeling.meta_arch.smca_detr")
    anchor = importlib.import_module("yolov7.modeling.meta_arch.anchor_detr")
    return r.detr_utils, smca, anchor


def run(crit, levels, targets):
    leaves = [(l.clone().requires_grad_(True), b.clone().requires_grad_(True)) for l, b in levels]
    ld = crit(R.as_outputs(leaves), targets)
    wd = R.weight_dict()
    tot = sum(ld[k] * wd[k] for k in ld if k in wd)
    tot.backward()
    return ld, tot, leaves


def main():
    if not ref_loader.available():
        sys.exit("gen_focal_golden.py: the reference tree is not there")
    du, smca, anchor = load_reference()
    fams = {
        "smca": (du.HungarianMatcherSMCA(**R.COSTS),
                 lambda m, C: smca.SetCriterion(C, m, R.weight_dict(), 0.1, ["labels", "boxes", "cardinality"])),
        "anchor": (du.HungarianMatcherAnchorDETR(**R.COSTS),
                   lambda m, C: anchor.SetCriterion(C, m, R.weight_dict(), ["labels", "boxes", "cardinality"], focal_alpha=R.ALPHA)),
    }
    data = {}
    runs = [(n, n, None) for n in R.GOLD_CASES] + [(n + "2", n, s) for n, s in R.SECOND_SEED.items()]
    for key, name, seed in runs:
        C = R.GOLD_CASES[name][2]
        levels, targets = R.inputs(name, seed)
        lv32, tg32 = R.inputs(name, seed, torch.float32)
        for fam, (matcher, mk) in fams.items():
            for l, ((lg, bx), (lg32, bx32)) in enumerate(zip(levels, lv32)):
                i64 = matcher({"pred_logits": lg, "pred_boxes": bx}, targets)
                i32 = matcher({"pred_logits": lg32, "pred_boxes": bx32}, tg32)
                for b, ((i, j), (i2, j2)) in enumerate(zip(i64, i32)):
                    assert torch.equal(i, i2) and torch.equal(j, j2), f"case {key} level {l} image {b}: float32 and float64 match differently - another seed"
                # rows of (image, query, target), images in order, queries ascending within an image
                data[f"{key}/{fam}/match{l}"] = np.concatenate(
                    [np.stack([np.full(len(i), b), i.numpy(), j.numpy()], 1) for b, (i, j) in enumerate(i64)]).astype(np.int16)
            ld, tot, leaves = run(mk(matcher, C), levels, targets)
            data[f"{key}/{fam}/loss_names"] = np.array("\n".join(ld))          # (the dict's keys, in its order)
            data[f"{key}/{fam}/losses"] = np.array([float(v.detach()) for v in ld.values()], dtype=np.float64)
            data[f"{key}/{fam}/total"] = np.float64(tot.detach())
            for l, (lg, bx) in enumerate(leaves):
                if fam == "anchor" and key in ("b", "a2"):
                    # 1 MiB does not hold case b's 3 x 3 x 100 x 91 float64 gradients twice: the second family's are held
                    # against the first's here instead of being stored
                    for n, t in (("dlogits", lg), ("dboxes", bx)):
                        ref = data[f"{key}/smca/{n}{l}"]
                        assert np.abs(t.grad.numpy() - ref).max() <= 1e-12 * np.abs(ref).max(), (key, n, l)
                    continue
                data[f"{key}/{fam}/dlogits{l}"], data[f"{key}/{fam}/dboxes{l}"] = lg.grad.numpy(), bx.grad.numpy()
    path = os.path.join(ROOT, "tests", "golden", "focal_criterion.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes;", len(data), "arrays")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
