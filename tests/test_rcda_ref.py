"""CPU: the float64 restatement of row-column decoupled attention (tests/rcda_ref.py) against the fixture the reference's own
MultiheadRCDA wrote (tests/golden/rcda.npz, tools/gen_rcda_golden.py) - this is where the definition is pinned to the
reference -, the mean-before-projection identity, a gradcheck of the core at a ragged case, and the exactness conditions of
the exact families the device tests use."""
import os

import numpy as np
import pytest
import torch

import rcda_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rcda.npz")
INPUTS = ("query_row", "query_col", "key_row", "key_col", "value")
PARAMS = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")


def _run(gold, mean_first):
    xs = [torch.from_numpy(gold["in/" + k]).requires_grad_(True) for k in INPUTS]
    ps = {k: torch.from_numpy(gold["param/" + k]).requires_grad_(True) for k in PARAMS}
    out = R.module(ps, *xs, torch.from_numpy(gold["mask"]), int(gold["heads"]), mean_first=mean_first)
    out.backward(torch.from_numpy(gold["dout"]))
    return out.detach(), dict(zip(INPUTS, (x.grad for x in xs))), {k: p.grad for k, p in ps.items()}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("mean_first", [True, False])
def test_restatement_equals_the_reference_fixture(gold, mean_first):
    """output and every gradient to 1e-12 relative, in the reference's order (project, then average) and in the order the
    kernels use (average, then project): the two differ in the order of roundings only"""
    out, gin, gpar = _run(gold, mean_first)
    assert gold["out"].dtype == np.float64 and out.shape == gold["out"].shape
    assert _rel(out, torch.from_numpy(gold["out"])) < 1e-12
    for k in INPUTS:
        assert _rel(gin[k], torch.from_numpy(gold["grad_in/" + k])) < 1e-12, k
    for k in PARAMS:
        assert _rel(gpar[k], torch.from_numpy(gold["grad_param/" + k])) < 1e-12, k


def test_fixture_is_the_case_the_issue_names(gold):
    assert gold["in/query_row"].shape == (2, 70, 64) and gold["in/value"].shape == (2, 5, 7, 64) and int(gold["heads"]) == 2
    m = gold["mask"]
    assert not m[0].any() and m[1, :, 5:].all() and m[1, 4:, :].all() and not m[1, :4, :5].any()
    for k in INPUTS:      # bf16 numbers: a device test feeds exactly these
        assert R.is_bf16(torch.from_numpy(gold["in/" + k]))
    assert os.path.getsize(GOLD) < 1 << 20


def test_core_gradcheck_ragged():
    ops, _, mr, mc = R.random_core_case(2, 2, 5, 3, 5, seed=4)
    xs = [(ops[n] * 0.5).requires_grad_(True) for n in R.CORE_NAMES]
    assert torch.autograd.gradcheck(lambda *a: R.core(*a, mr, mc, 2), xs, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_all_keys_padded_gives_zero_and_no_gradient():
    ops, dout, mr, mc = R.random_core_case(2, 1, 4, 3, 5, seed=5)
    mr[1, :] = True
    o, g = R.core_with_grads(ops, dout, mr, mc, 1, torch.float64, False)
    assert bool(torch.isfinite(o).all()) and float(o[1].abs().max()) == 0 and float(o[0].abs().max()) > 0
    for n in R.CORE_NAMES:
        assert bool(torch.isfinite(g[n]).all()) and float(g[n][1].abs().max()) == 0, n


def test_emulation_is_close_to_float64():
    ops, dout, mr, mc = R.random_core_case(2, 2, 70, 5, 7, seed=6)
    o64, g64 = R.core_with_grads(ops, dout, mr, mc, 2, torch.float64, False)
    o32, g32 = R.core_with_grads(ops, dout, mr, mc, 2, torch.float32, True)
    assert R.is_bf16(o32) and 0 < R.rel_l2(o32, o64) < 1e-2
    for n in R.CORE_NAMES:
        assert R.is_bf16(g32[n]) and 0 < R.rel_l2(g32[n], g64[n]) < 2e-2, n


@pytest.mark.parametrize("shape", R.EXACT_SHAPES)
def test_exact_families_satisfy_their_conditions(shape):
    B, heads, Lq, H, W = shape
    ops, dout, mr, mc = R.uniform_case(*shape, seed=1)
    R.check_uniform_conditions(ops, dout, mr, mc, heads)
    o, g = R.core_with_grads(ops, dout, mr, mc, heads, torch.float64, False)
    assert all(bool(torch.isfinite(x).all()) for x in [o, *g.values()])
    if H > 1 and W > 1 and Lq > 1:
        assert float(g["k_row"].abs().max()) > 0 and float(g["k_col"].abs().max()) > 0 and float(g["v"].abs().max()) > 0
    ops, dout, mr, mc, hs, ws = R.gather_case(*shape, seed=2)
    R.check_gather_conditions(ops, mr, mc, hs, ws, heads)
    o, g = R.core_with_grads(ops, dout, mr, mc, heads, torch.float64, False)
    eo, edv = R.gather_expected(ops, dout, hs, ws, heads)
    # (in float64 the other weights are 2^-1000, not yet 0: what they add is below 1e-290)
    assert torch.equal(o, eo) and float((g["v"] - edv).abs().max()) < 1e-290
    for n in ("q_row", "q_col", "k_row", "k_col"):
        assert float(g[n].abs().max()) < 1e-290, n
