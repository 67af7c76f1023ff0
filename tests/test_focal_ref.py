"""CPU, no device: the focal matcher / set criterion restatement of tests/focal_ref.py against the fixture
tests/golden/focal_criterion.npz (the reference's own HungarianMatcherSMCA / HungarianMatcherAnchorDETR and the SetCriterion of
smca_detr.py / anchor_detr.py in float64, tools/gen_focal_golden.py).

  * focal_ref in float64: the match pairs are the fixture's, every loss entry, the weighted total and every stored gradient agree
    to 1e-10 relative - for BOTH reference families, which is what lets one implementation serve both;
  * the closed-form class gradient (the backward kernel's) equals autograd through the restated forward, also without alpha
    weighting and at saturated logits;
  * focal_ref in float32 finds the same pairs (the generator asserted it for the reference)."""
import os

import numpy as np
import pytest
import torch

import focal_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "focal_criterion.npz")
TOL = 1e-10
FAMS = ("smca", "anchor")
KEYS = list(R.GOLD_CASES) + [n + "2" for n in R.SECOND_SEED]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def case_inputs(key, dtype=torch.float64):
    name = key[0]
    return R.inputs(name, R.SECOND_SEED[name] if key.endswith("2") else None, dtype)


def gold_pairs(gold, key, fam, level, B):
    m = gold[f"{key}/{fam}/match{level}"].astype(np.int64)
    return [(torch.from_numpy(m[m[:, 0] == b, 1]), torch.from_numpy(m[m[:, 0] == b, 2])) for b in range(B)]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def test_fixture_holds_data_only_and_stays_small(gold):
    assert os.path.getsize(GOLD) < 1 << 20
    for k, v in gold.items():
        assert v.dtype in (np.float64, np.int16) or v.dtype.kind == "U", k
    for key in KEYS:
        for l in range(R.LEVELS):      # the two reference matchers are the same computation
            assert np.array_equal(gold[f"{key}/smca/match{l}"], gold[f"{key}/anchor/match{l}"])


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("key", KEYS)
def test_restatement_in_float64_equals_the_reference(key, fam, gold):
    levels, targets = case_inputs(key)
    leaves = [(l.clone().requires_grad_(True), b.clone().requires_grad_(True)) for l, b in levels]
    ld, used = R.criterion(leaves, targets)
    for l, idx in enumerate(used):
        want = gold_pairs(gold, key, fam, l, len(targets))
        for (i, j), (wi, wj) in zip(idx, want):
            assert torch.equal(i, wi) and torch.equal(j, wj), (key, l)
    names = str(gold[f"{key}/{fam}/loss_names"]).split("\n")
    assert set(ld) == set(names) and len(names) == 5 + 4 * (R.LEVELS - 1)
    for n, want in zip(names, gold[f"{key}/{fam}/losses"]):
        assert abs(float(ld[n].detach()) - want) <= TOL * abs(want), (n, float(ld[n].detach()), want)
    tot = R.total(ld)
    want = float(gold[f"{key}/{fam}/total"])
    assert abs(float(tot) - want) <= TOL * abs(want)
    tot.backward()
    checked = 0
    for l, (lg, bx) in enumerate(leaves):
        if f"{key}/{fam}/dlogits{l}" not in gold:        # (case b and a2 store one family's gradients: see the generator)
            continue
        assert rel(lg.grad.numpy(), gold[f"{key}/{fam}/dlogits{l}"]) < TOL, l
        wb = gold[f"{key}/{fam}/dboxes{l}"]
        assert rel(bx.grad.numpy(), wb) < TOL or (not wb.any() and not bx.grad.numpy().any()), l
        checked += 1
    assert checked == (0 if (fam == "anchor" and key in ("b", "a2")) else R.LEVELS)


def test_cases_cover_what_they_are_for(gold):
    B, Q, C, sz = R.GOLD_CASES["b"][:4]
    assert 0 in sz and max(sz) > 64 and C == 91
    assert R.GOLD_CASES["c"][1] % 4 and max(R.GOLD_CASES["c"][3]) > R.GOLD_CASES["c"][1]
    assert sum(R.GOLD_CASES["d"][3]) == 0 and R.GOLD_CASES["e"][2] > 128 and R.GOLD_CASES["f"][2] == 1
    assert (R.GOLD_CASES["g"][2], R.GOLD_CASES["h"][2]) == (64, 65)
    names = str(gold["d/smca/loss_names"]).split("\n")
    d = dict(zip(names, gold["d/smca/losses"]))
    assert d["class_error"] == 100.0 and d["loss_bbox"] == 0.0 and d["loss_ce"] > 0      # no pair anywhere; num_boxes clamped to 1
    # p sits near 0.01 where the recipe adds the prior-probability bias
    lg = R.inputs("a")[0][0][0]
    assert 0.005 < float(lg.sigmoid().median()) < 0.02


@pytest.mark.parametrize("alpha", [0.25, -1.0, 0.6])
def test_closed_form_gradient_equals_autograd(alpha):
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(64, 33, generator=g, dtype=torch.float64) * 4).requires_grad_(True)
    t = (torch.rand(64, 33, generator=g) < 0.1).double()
    R.focal_terms(x, t, alpha).sum().backward()
    got = R.focal_grad(x.detach(), t, alpha)
    assert rel(got.numpy(), x.grad.numpy()) < TOL
    # saturated logits: finite, and still autograd's
    xs = torch.tensor([-100.0, -40.0, 40.0, 100.0], dtype=torch.float64).repeat(2).requires_grad_(True)
    ts = torch.tensor([0.0] * 4 + [1.0] * 4, dtype=torch.float64)
    loss = R.focal_terms(xs, ts, alpha)
    loss.sum().backward()
    gs = R.focal_grad(xs.detach(), ts, alpha)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(gs).all())
    assert rel(gs.numpy(), xs.grad.numpy()) < TOL


def test_loss_terms_are_binary_cross_entropy_with_logits_times_the_modulator():
    g = torch.Generator().manual_seed(8)
    x = torch.randn(5, 9, generator=g, dtype=torch.float64) * 3
    t = (torch.rand(5, 9, generator=g) < 0.3).double()
    p = x.sigmoid()
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    want = (0.25 * t + 0.75 * (1 - t)) * ce * (1 - (p * t + (1 - p) * (1 - t))) ** 2
    assert rel(R.focal_terms(x, t).numpy(), want.numpy()) < 1e-14


@pytest.mark.parametrize("key", list(R.GOLD_CASES))
def test_restatement_in_float32_finds_the_same_pairs(key, gold):
    levels, targets = case_inputs(key, torch.float32)
    for l, (lg, bx) in enumerate(levels):
        got = R.match(lg, bx, targets, **R.COSTS)
        for (i, j), (wi, wj) in zip(got, gold_pairs(gold, key, "smca", l, len(targets))):
            assert torch.equal(i, wi) and torch.equal(j, wj)
