"""GPU (-m gpu): the focal matcher and set criterion (HungarianMatcherFocal, FocalSetCriterion / SMCASetCriterion on
mi_hungarian_match_focal, mi_focal_set_loss_fwd / _bwd) against the fixture tests/golden/focal_criterion.npz - the reference's own
matchers and criteria of SMCA-DETR and Anchor DETR in float64 - and against tests/focal_ref.py.

Bounds.  Match pairs: exact (the generator asserted that the reference finds the same pairs in float32 as in float64).  class_error
and cardinality_error: exact against focal_ref in float32 (ratios of small integers, computed the same way).  Losses: rtol 1e-5 /
atol 1e-6 against float64, gradients rtol 2e-4 with atol 1e-8 (logits) / 1e-7 (boxes): the values tests/test_gpu_detr.py applies to
the sibling criterion against its fixture.  The three call forms: bit-equal between the PackedTargets per-level call and
weighted_packed (both divide by num_boxes outside the kernels), the tolerances above against the eager call (which divides inside).
Inputs are focal_ref's seeded recipe; every case of GOLD_CASES is used."""
import os

import numpy as np
import pytest
import torch

import focal_ref as R
from yolov7_d2_amd.modeling import FocalSetCriterion, HungarianMatcherFocal, SMCASetCriterion
from yolov7_d2_amd.modeling.detr_matcher import PackedTargets

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = list(R.GOLD_CASES)
LOSSES = ["labels", "boxes", "cardinality"]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "focal_criterion.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def gold_pairs(gold, key, level, B, fam="smca"):
    m = gold[f"{key}/{fam}/match{level}"].astype(np.int64)
    return [(torch.from_numpy(m[m[:, 0] == b, 1]), torch.from_numpy(m[m[:, 0] == b, 2])) for b in range(B)]


def gold_losses(gold, key, fam="smca"):
    return dict(zip(str(gold[f"{key}/{fam}/loss_names"]).split("\n"), gold[f"{key}/{fam}/losses"]))


def host_case(key, dtype=torch.float32):
    name = key[0]
    return R.inputs(name, R.SECOND_SEED[name] if key.endswith("2") else None, dtype)


def leaves_of(levels):
    return [(l.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)) for l, b in levels]


def to_dev(targets):
    return [{"labels": t["labels"].to(DEV), "boxes": t["boxes"].float().to(DEV)} for t in targets]


def fill_packed(pt, targets):
    """what Detr.prepare_batch does with a batch's ground truth, in place"""
    off = [0]
    for t in targets:
        off.append(off[-1] + len(t["labels"]))
    n = off[-1]
    assert max(len(t["labels"]) for t in targets) <= pt.cap
    labels = torch.cat([t["labels"] for t in targets]).to(torch.int64)
    boxes = torch.cat([t["boxes"] for t in targets]).float()
    pt.tgt_off.copy_(torch.tensor(off, dtype=torch.int32))
    if n:
        pt.tgt_labels[:n].copy_(labels)
        pt.tgt_boxes[:n].copy_(boxes)
    pt.fill_levels(off, labels if n else None, boxes if n else None)
    pt.inv_num_boxes.copy_(torch.tensor([1.0 / max(float(n), 1.0)]))
    for b in range(len(targets)):
        pt[b] = {"labels": pt.tgt_labels[off[b]:off[b + 1]], "boxes": pt.tgt_boxes[off[b]:off[b + 1]]}
    return pt


def packed(targets, cap, levels=R.LEVELS):
    B = len(targets)
    pt = PackedTargets([None] * B, cap, torch.zeros(B + 1, dtype=torch.int32, device=DEV),
                       torch.zeros(B * cap, dtype=torch.int64, device=DEV), torch.zeros(B * cap, 4, device=DEV),
                       torch.ones(1, device=DEV), levels=levels)
    return fill_packed(pt, targets)


def cap_of(targets):
    return max(16, max(len(t["labels"]) for t in targets) + 2)


def crit_for(key, alpha=R.ALPHA, matcher=None):
    return FocalSetCriterion(R.GOLD_CASES[key[0]][2], matcher or HungarianMatcherFocal(**R.COSTS), R.weight_dict(), LOSSES,
                             focal_alpha=alpha)


def grads(leaves):
    out = [(l.grad.clone(), b.grad.clone()) for l, b in leaves]
    for l, b in leaves:
        l.grad = b.grad = None
    return out


class ListMatcher:
    """a foreign matcher: the reference's interface, index lists per image"""

    def __init__(self, per_level):
        self.per_level, self.calls = per_level, 0

    def __call__(self, outputs, targets):
        order = [len(self.per_level) - 1] + list(range(len(self.per_level) - 1))       # the last level is matched first
        idx = self.per_level[order[self.calls % len(order)]]
        self.calls += 1
        return idx


# ------------------------------------------------------------------------------------------ matching
@pytest.mark.parametrize("key", KEYS)
def test_match_pairs_are_the_reference_s(key, gold):
    levels, targets = host_case(key)
    tg = to_dev(targets)
    m = HungarianMatcherFocal(**R.COSTS)
    B = len(targets)
    for l, (lg, bx) in enumerate(levels):
        got = m({"pred_logits": lg.to(DEV), "pred_boxes": bx.to(DEV)}, tg)
        off = 0
        Cref = R.matching_cost(lg, bx, targets, **R.COSTS)
        for b, ((i, j), (wi, wj)) in enumerate(zip(got, gold_pairs(gold, key, l, B))):
            assert i.dtype == torch.int64 and j.dtype == torch.int64
            assert torch.equal(i.cpu(), wi) and torch.equal(j.cpu(), wj), (key, l, b)
            G = len(targets[b]["labels"])       # the cost matrix itself: float parity with the float32 restatement
            np.testing.assert_allclose(m.last_cost[b, :, :G].cpu().numpy(), Cref[b, :, off:off + G].numpy(), rtol=1e-5, atol=1e-6)
            off += G
    pt = packed(targets, cap_of(targets))
    ms = m.match_device_levels([{"pred_logits": lg.to(DEV), "pred_boxes": bx.to(DEV)} for lg, bx in levels], pt)
    for l, d in enumerate(ms):
        n = d["nmatch"].tolist()
        for b, (wi, wj) in enumerate(gold_pairs(gold, key, l, B)):
            assert n[b] == len(wi)
            assert torch.equal(d["match_q"][b, :n[b]].cpu(), wi) and torch.equal(d["match_t"][b, :n[b]].cpu(), wj), (key, l, b)


# ------------------------------------------------------------------------------------------ criterion against the fixture
def check_against_gold(gold, key, ld, total, gr, fam="smca"):
    want = gold_losses(gold, key, fam)
    assert set(ld) == set(want)
    for k, w in want.items():
        np.testing.assert_allclose(float(ld[k].detach()), w, rtol=1e-5, atol=1e-6, err_msg=k)
    np.testing.assert_allclose(float(total.detach()), float(gold[f"{key}/{fam}/total"]), rtol=1e-5)
    for l, (dl, db) in enumerate(gr):
        np.testing.assert_allclose(dl.cpu().numpy(), gold[f"{key}/smca/dlogits{l}"], rtol=2e-4, atol=1e-8, err_msg=f"dlogits{l}")
        np.testing.assert_allclose(db.cpu().numpy(), gold[f"{key}/smca/dboxes{l}"], rtol=2e-4, atol=1e-7, err_msg=f"dboxes{l}")


@pytest.mark.parametrize("key", KEYS)
def test_criterion_against_the_reference_fixture(key, gold):
    levels, targets = host_case(key)
    B, Q, C = levels[0][0].shape
    leaves, tg = leaves_of(levels), to_dev(targets)
    crit = crit_for(key)
    wd = R.weight_dict()

    def run():
        ld = crit(R.as_outputs(leaves), tg)
        total = sum(ld[k] * wd[k] for k in ld if k in wd)
        total.backward()
        return ld, total, grads(leaves)

    ld, total, gr = run()
    check_against_gold(gold, key, ld, total, gr)
    check_against_gold(gold, key, ld, total, [], fam="anchor")        # the other family's numbers are the same numbers
    # the counted outputs: exactly focal_ref's in float32
    pairs = [gold_pairs(gold, key, l, B) for l in range(R.LEVELS)]
    ref32, _ = R.criterion(levels, targets, indices=pairs)
    for k in ref32:
        if k.startswith("class_error") or k.startswith("cardinality_error"):
            assert ld[k].dtype == torch.float32 and float(ld[k]) == float(ref32[k]), (k, float(ld[k]), float(ref32[k]))
            assert not ld[k].requires_grad
    # structure: finite class gradients everywhere, exactly no box gradient in a row without a match
    for l, (dl, db) in enumerate(gr):
        assert bool(torch.isfinite(dl).all())
        matched = torch.zeros(B, Q, dtype=torch.bool)
        for b, (i, _) in enumerate(pairs[l]):
            matched[b, i] = True
        assert float(db.cpu()[~matched].abs().sum()) == 0.0
        if matched.any():
            assert bool((db.cpu()[matched].abs().sum(-1) > 0).all())
    # a second run: bit for bit
    ld2, total2, gr2 = run()
    assert torch.equal(total, total2) and all(torch.equal(ld[k], ld2[k]) for k in ld)
    for (a, b), (c, d) in zip(gr, gr2):
        assert torch.equal(a, c) and torch.equal(b, d)


def test_smca_signature_is_the_same_criterion(gold):
    levels, targets = host_case("a")
    tg = to_dev(targets)
    out = R.as_outputs([(l.to(DEV), b.to(DEV)) for l, b in levels])
    a = crit_for("a")(out, tg)
    b = SMCASetCriterion(20, HungarianMatcherFocal(**R.COSTS), R.weight_dict(), 0.1, LOSSES).to(DEV)(out, tg)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------ the three call forms
@pytest.mark.parametrize("key", KEYS)
def test_eager_packed_and_weighted_packed_agree(key):
    levels, targets = host_case(key)
    leaves, tg = leaves_of(levels), to_dev(targets)
    crit, wd = crit_for(key), R.weight_dict()
    pt = packed(targets, cap_of(targets))
    le = crit(R.as_outputs(leaves), tg)
    sum(le[k] * wd[k] for k in le if k in wd).backward()
    ge = grads(leaves)
    lp = crit(R.as_outputs(leaves), pt)
    sum(lp[k] * wd[k] for k in lp if k in wd).backward()
    gp = grads(leaves)
    lw = crit.weighted_packed(R.as_outputs(leaves), pt)
    lw["total"].backward()
    gw = grads(leaves)
    assert set(lw) == set(lp) | {"total"} and set(le) == set(lp)
    for k in lp:
        assert torch.equal((lp[k] * wd[k] if k in wd else lp[k]).detach(), lw[k].detach()), k
        np.testing.assert_allclose(float(lp[k].detach()), float(le[k].detach()), rtol=1e-5, atol=1e-6, err_msg=k)
    np.testing.assert_allclose(float(lw["total"].detach()), float(sum(le[k].detach() * wd[k] for k in le if k in wd)), rtol=1e-5)
    for (a, b), (c, d), (e, f) in zip(gp, gw, ge):
        assert torch.equal(a, c) and torch.equal(b, d)
        np.testing.assert_allclose(a.cpu().numpy(), e.cpu().numpy(), rtol=2e-4, atol=1e-8)
        np.testing.assert_allclose(b.cpu().numpy(), f.cpu().numpy(), rtol=2e-4, atol=1e-7)


def test_gradients_come_back_in_the_input_dtypes():
    levels, targets = host_case("g")
    lg, bx = levels[-1]
    lg, bx = lg.to(DEV).bfloat16().requires_grad_(True), bx.to(DEV).double().requires_grad_(True)
    ld = crit_for("g")({"pred_logits": lg, "pred_boxes": bx}, to_dev(targets))
    (ld["loss_ce"] + ld["loss_bbox"] + ld["loss_giou"]).backward()
    assert lg.grad.dtype == torch.bfloat16 and bx.grad.dtype == torch.float64


# ------------------------------------------------------------------------------------------ saturated logits, no alpha weighting
def against_focal_ref(levels32, targets, pairs, alpha):
    """the device criterion on float32 inputs with the given matches against focal_ref in float64 on the same numbers"""
    leaves, tg = leaves_of(levels32), to_dev(targets)
    crit = crit_for("a", alpha=alpha, matcher=ListMatcher(pairs))
    wd = R.weight_dict()
    ld = crit(R.as_outputs(leaves), tg)
    total = sum(ld[k] * wd[k] for k in ld if k in wd)
    total.backward()
    ref_leaves = [(l.double().requires_grad_(True), b.double().requires_grad_(True)) for l, b in levels32]
    t64 = [{"labels": t["labels"], "boxes": t["boxes"].double()} for t in targets]
    rd, _ = R.criterion(ref_leaves, t64, indices=pairs, alpha=alpha)
    R.total(rd).backward()
    assert set(ld) == set(rd)
    for k in rd:
        assert bool(torch.isfinite(ld[k]))
        np.testing.assert_allclose(float(ld[k].detach()), float(rd[k].detach()), rtol=1e-5, atol=1e-6, err_msg=k)
    for (l, b), (rl, rb) in zip(leaves, ref_leaves):
        assert bool(torch.isfinite(l.grad).all()) and bool(torch.isfinite(b.grad).all())
        np.testing.assert_allclose(l.grad.cpu().numpy(), rl.grad.numpy(), rtol=2e-4, atol=1e-8)
        np.testing.assert_allclose(b.grad.cpu().numpy(), rb.grad.numpy(), rtol=2e-4, atol=1e-7)


def test_saturated_logits_stay_finite_and_right(gold):
    """case a's logits times 30 and rows at +-100; the matches are the moderate-logit ones, handed in by a foreign matcher (the
    matcher is not run on saturated costs, where ties are legitimate)"""
    levels, targets = host_case("a")
    pairs = [gold_pairs(gold, "a", l, len(targets)) for l in range(R.LEVELS)]
    hot = []
    ramp = torch.arange(levels[0][0].shape[-1]) * 0.01        # (no two channels equal: the arg max stays unique)
    for l, (lg, bx) in enumerate(levels):
        lg = lg * 30
        lg[0, 0], lg[0, 1] = 100.0 - ramp, -100.0 + ramp
        q = int(pairs[l][1][0][0])           # a matched row, saturated both ways
        lg[1, q] = torch.where(torch.arange(len(ramp)) % 2 == 0, 100.0 - ramp, -100.0 + ramp)
        hot.append((lg, bx))
    against_focal_ref(hot, targets, pairs, R.ALPHA)


def test_no_alpha_weighting(gold):
    levels, targets = host_case("a")
    pairs = [gold_pairs(gold, "a", l, len(targets)) for l in range(R.LEVELS)]
    against_focal_ref(levels, targets, pairs, -1.0)


# ------------------------------------------------------------------------------------------ foreign matcher, errors
def test_foreign_matcher_and_errors(gold):
    levels, targets = host_case("a")
    tg = to_dev(targets)
    pairs = [gold_pairs(gold, "a", l, len(targets)) for l in range(R.LEVELS)]
    out = R.as_outputs([(l.to(DEV), b.to(DEV)) for l, b in levels])
    a = crit_for("a", matcher=ListMatcher(pairs))(out, tg)
    b = crit_for("a")(out, tg)
    assert set(a) == set(b)
    for k in a:
        assert float(a[k]) == float(b[k]), k
    with pytest.raises(NotImplementedError):
        FocalSetCriterion(20, ListMatcher(pairs), {}, ["labels", "masks"])
    with pytest.raises(ValueError, match="num_classes channels"):
        FocalSetCriterion(19, HungarianMatcherFocal(**R.COSTS), {}, LOSSES)(out, tg)        # a head with a no-object channel
    # a NaN cost: the matcher's ordinary error return (nmatch < 0), as scipy raises in the reference
    lg, bx = levels[-1]
    lg = lg.clone()
    lg[0, 3, int(targets[0]["labels"][0])] = float("nan")
    with pytest.raises(ValueError, match="invalid numeric"):
        HungarianMatcherFocal(**R.COSTS)({"pred_logits": lg.to(DEV), "pred_boxes": bx.to(DEV)}, tg)
    m = HungarianMatcherFocal(**R.COSTS).match_device({"pred_logits": lg.to(DEV), "pred_boxes": bx.to(DEV)}, tg)
    assert m["nmatch"].tolist() == [-1, len(targets[1]["labels"])]          # the other image is matched as usual


# ------------------------------------------------------------------------------------------ capture
class _Head(torch.nn.Module):
    """the smallest model GraphedTrainStep drives: the decoder levels' outputs as parameters, the criterion as the forward"""

    def __init__(self, levels, crit):
        super().__init__()
        self.lg = torch.nn.ParameterList([torch.nn.Parameter(l.to(DEV)) for l, _ in levels])
        self.bx = torch.nn.ParameterList([torch.nn.Parameter(b.to(DEV)) for _, b in levels])
        self.criterion, self.device = crit, torch.device(DEV)

    def batch_key(self, batch):
        return len(batch[1])

    def prepare_batch(self, batch, static=None):
        levels, targets = batch
        if static is None:
            static = {"targets": packed(targets, 16)}
        else:
            fill_packed(static["targets"], targets)
        with torch.no_grad():
            for p, (l, _) in zip(self.lg, levels):
                p.copy_(l)
            for p, (_, b) in zip(self.bx, levels):
                p.copy_(b)
        return static

    def forward_prepared(self, static):
        return self.criterion.weighted_packed(R.as_outputs(list(zip(self.lg, self.bx))), static["targets"])


class _NoUpdate:
    """the optimizer slot of GraphedTrainStep, empty: the step under test ends at the gradients"""

    def __init__(self, params):
        self.param_groups, self.state = [{"params": list(params)}], {}

    def zero_grad(self, set_to_none=True):
        for p in self.param_groups[0]["params"]:
            p.grad = None

    def step(self):
        pass


def test_weighted_packed_and_its_backward_replay_as_one_graph(gold):
    from yolov7_d2_amd.graph_step import GraphedTrainStep
    first, second = host_case("a"), host_case("a2")
    model = _Head(first[0], crit_for("a"))
    step = GraphedTrainStep(model, _NoUpdate(model.parameters()), warmup=1, batch_packs=False)
    try:
        for it, (key, batch) in enumerate((("a", first), ("a2", second), ("a", first))):
            out = step(batch)                    # the first call captures, the later ones refill in place and replay
            assert len(step.graphs) == 1
            total = out["total"].clone()
            gr = [(l.grad.clone(), b.grad.clone()) for l, b in zip(model.lg, model.bx)]
            leaves = leaves_of(batch[0])
            want = crit_for("a").weighted_packed(R.as_outputs(leaves), packed(batch[1], 16))
            want["total"].backward()
            assert torch.equal(total, want["total"].detach()), (it, float(total), float(want["total"]))
            for k in want:
                assert torch.equal(out[k], want[k].detach()), (it, k)
            for (dl, db), (l, b) in zip(gr, leaves):
                assert torch.equal(dl, l.grad) and torch.equal(db, b.grad), it
            np.testing.assert_allclose(float(total), float(gold[f"{key}/smca/total"]), rtol=1e-5)
            for l, (dl, db) in enumerate(gr):
                np.testing.assert_allclose(dl.cpu().numpy(), gold[f"{key}/smca/dlogits{l}"], rtol=2e-4, atol=1e-8)
                np.testing.assert_allclose(db.cpu().numpy(), gold[f"{key}/smca/dboxes{l}"], rtol=2e-4, atol=1e-7)
    finally:
        step.close()
