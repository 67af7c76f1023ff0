"""CPU: tests/pool_ref.py - the references tests/test_gpu_pool_exact.py holds the pooling, resampling, copy and SGD kernels
to.  The first-maximum rule is pinned three ways on tie-heavy input (the scan, np.argmax over padded windows, F.max_pool2d
and its float64 autograd gradient: all array_equal), the upsample against F.interpolate, the SGD step against
torch.optim.SGD in float64, round_bf16 against torch's conversion on random and on constructed half-way values; the two
exactness predicates must hold on the families of the GPU tables and fail on a counter-example of each."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_ref as R

KSP = [(5, 1, 2), (9, 1, 4), (13, 1, 6), (3, 2, 1)]
PLANES = [(7, 9), (1, 14), (23, 23), (26, 20)]


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).transpose(0, 3, 1, 2)))


def nhwc(t):
    return t.detach().numpy().transpose(0, 2, 3, 1)


@pytest.mark.parametrize("plane", PLANES)
@pytest.mark.parametrize("ksp", KSP)
def test_first_maximum_rule_is_torch_cpu_rule(ksp, plane):
    """values and gradient of F.max_pool2d in float64 on {-1, 0, 1}, constant planes, constant rows and constant columns:
    with ties everywhere the gradient lands where the reference's first maximum is, and nowhere else"""
    k, s, p = ksp
    H, W = plane
    for fam in ("levels", "const", "rows", "cols"):
        x = R.family(fam, (2, H, W, 8), 100 * H + W + k)
        vals, pos = R.maxpool_first(x, k, s, p)
        v2, p2 = R.maxpool_first_windows(x, k, s, p)
        assert np.array_equal(vals, v2) and np.array_equal(pos, p2), fam
        g = R.grads(vals.shape, k + H)
        xt = nchw(x).requires_grad_(True)
        yt = F.max_pool2d(xt, k, s, p)
        assert np.array_equal(nhwc(yt), vals), fam
        (yt * nchw(g)).sum().backward()
        assert np.array_equal(nhwc(xt.grad), R.maxpool_bwd(pos, g, k, s, p, H, W)), fam
        if fam == "const":                              # the first in-bounds cell of every window
            oy, ox = np.arange(vals.shape[1]).reshape(-1, 1), np.arange(vals.shape[2])
            first = np.maximum(0, p - oy * s) * k + np.maximum(0, p - ox * s)
            assert np.array_equal(pos, np.broadcast_to(first[None, :, :, None], pos.shape))


def test_rows_and_cols_take_the_rules_apart():
    """constant rows: every maximum sits in the first in-bounds COLUMN of its window and in the first of the rows that hold
    the largest value; constant columns: the transpose"""
    x = R.family("rows", (1, 9, 11, 8), 3)
    _, pos = R.maxpool_first(x, 5, 1, 2)
    assert np.array_equal(pos % 5, np.broadcast_to(np.maximum(0, 2 - np.arange(11))[None, None, :, None], pos.shape))
    xt = R.family("cols", (1, 9, 11, 8), 3)
    _, post = R.maxpool_first(xt, 5, 1, 2)
    assert np.array_equal(post // 5, np.broadcast_to(np.maximum(0, 2 - np.arange(9))[None, :, None, None], post.shape))
    assert len(np.unique(pos // 5)) > 1 and len(np.unique(post % 5)) > 1


def test_maxpool_code_is_the_window_position():
    x = np.zeros((1, 4, 4, 8))
    x[0, 2, 1, :] = 1                                   # output (1, 1): rows 1..3, columns 1..3; output (1, 0): columns -1..1
    _, pos = R.maxpool_first(x, 3, 2, 1)
    code = R.maxpool_code(pos)
    assert code.dtype == np.uint8 and int(code[0, 1, 1, 0]) == 1 * 3 + 0 and int(code[0, 1, 0, 0]) == 1 * 3 + 2
    assert int(code[0, 0, 0, 0]) == 4                   # a window of zeros: the first in-bounds cell, (1, 1)


def test_upsample_is_interpolate_nearest():
    x = R.family("silu", (2, 6, 5, 8), 1)
    xt = nchw(x).requires_grad_(True)
    yt = F.interpolate(xt, scale_factor=2, mode="nearest")
    assert np.array_equal(nhwc(yt), R.upsample2x(x))
    g = R.grads((2, 12, 10, 8), 2)
    (yt * nchw(g)).sum().backward()
    assert np.array_equal(nhwc(xt.grad), R.upsample2x_bwd(g))


def test_sgd_step_is_torch_sgd_in_float64():
    rng = np.random.default_rng(0)
    n = 300
    p0, m0 = rng.standard_normal(n), np.zeros(n)
    segs = [(0, 100, 1e-4, 0.01), (120, 77, 5e-3, 0.1)]
    params = [torch.from_numpy(p0[o:o + c].copy()).requires_grad_(True) for o, c, _, _ in segs]
    opt = torch.optim.SGD([dict(params=[q], weight_decay=wd, lr=lr) for q, (_, _, wd, lr) in zip(params, segs)], lr=1.0, momentum=0.9)
    p, m = p0, m0
    for step in range(3):
        g = rng.standard_normal(n)
        for q, (o, c, _, _) in zip(params, segs):
            q.grad = torch.from_numpy(g[o:o + c] * 0.25)
        opt.step()
        p, m = R.sgd_step(p, g, m, segs, 0.9, 0.25, step == 0)
        for q, (o, c, _, _) in zip(params, segs):
            np.testing.assert_allclose(p[o:o + c], q.detach().numpy(), rtol=1e-14, atol=0)
    assert np.array_equal(p[100:120], p0[100:120]) and np.array_equal(p[197:], p0[197:]) and not m[100:120].any()


def test_round_bf16_is_torch_conversion():
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(20000) * np.ldexp(1.0, rng.integers(-140, 120, 20000))).astype(np.float32)
    k = rng.integers(128, 256, 4000).astype(np.float64)
    half = np.concatenate([(k + 0.5) * np.ldexp(1.0, rng.integers(-130, 118, 4000)), -(k + 0.5) / 256,      # exact ties
                           (np.arange(8) + 0.5) * 2.0 ** -133, [R.BF16_MAX + 2.0 ** 119, R.BF16_MAX + 2.0 ** 118, 257.0, 259.0, 0.0, -0.0,
                                                               np.inf, -np.inf]]).astype(np.float32)
    for v in (a, half):
        got = R.round_bf16(v.astype(np.float64))
        ref = torch.from_numpy(v).to(torch.bfloat16).to(torch.float64).numpy()
        assert np.array_equal(got, ref) and np.array_equal(np.signbit(got), np.signbit(ref))
    assert R.round_bf16(257.0) == 256 and R.round_bf16(259.0) == 260 and np.isinf(R.round_bf16(R.BF16_MAX + 2.0 ** 119))
    assert R.round_bf16(R.BF16_MAX + 2.0 ** 118) == R.BF16_MAX and np.isnan(R.round_bf16(np.nan))
    assert R.round_bf16(1 + 2.0 ** -8 + 2.0 ** -40) == 1 + 2.0 ** -7       # one rounding: fp32 first would give a tie, then 1
    assert R.bf16_ulp(1.0) == 2.0 ** -7 and R.bf16_ulp(255.0) == 1 and R.bf16_ulp(256.0) == 2 and R.bf16_ulp(0.0) == 2.0 ** -133


def test_copy_acc_rounds_twice():
    a, b = R.acc_pairs(4096, 5)
    t = lambda v: torch.from_numpy(v).to(torch.bfloat16)
    ref = (t(a).float() + t(b).float()).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(R.copy_acc(a, b), ref, equal_nan=True)
    assert R.copy_acc(256.0, 1.0) == 256 and R.copy_acc(258.0, 1.0) == 260 and R.copy_acc(1.0, 2.0 ** -30) == 1
    assert np.isinf(R.copy_acc(R.BF16_MAX, R.BF16_MAX)) and np.isnan(R.copy_acc(np.inf, -np.inf))


def test_scale_rows_is_one_rounding():
    rng = np.random.default_rng(2)
    g, sc = rng.standard_normal((7, 36)).astype(np.float32), rng.standard_normal(7).astype(np.float32)
    assert np.array_equal(R.scale_rows(g, sc), g * sc[:, None]) and R.scale_rows(g, sc).dtype == np.float32


def test_gradient_predicate_holds_on_the_gpu_families_and_fails_on_2_to_20():
    """the worst case of the GPU tables: a constant 32 x 32 plane (all 25 + 81 + 169 windows of a corner's neighbourhood
    choose one pixel) with |dy| = 64 everywhere and a prior of 64"""
    x = R.family("const", (1, 32, 32, 8), 0)
    poss = [p for _, p in R.spp_fwd(x)]
    gs = [np.full(x.shape, 64.0)] * 3
    prior = np.full(x.shape, -64.0)
    ab = R.spp_bwd(poss, gs, prior, np.abs)
    assert R.grad_family_ok(ab, prior, *gs) and ab.max() == 64 * (1 + 9 + 25 + 49)
    nt = R.spp_bwd(poss, gs, None, np.ones_like)
    assert nt.max() == 9 + 25 + 49 and nt.sum() == 3 * x.size
    for fam in R.FAMILIES:
        x = R.family(fam, (2, 19, 27, 8), 4)
        poss = [p for _, p in R.spp_fwd(x)]
        gs = [R.grads(x.shape, 10 + i) for i in range(3)]
        prior = R.grads(x.shape, 20)
        assert R.grad_family_ok(R.spp_bwd(poss, gs, prior, np.abs), prior, *gs)
        ref = R.spp_bwd(poss, gs, prior)
        assert fam != "const" or (np.abs(ref) > 256).any() and (R.round_bf16(ref) != ref).any()    # ties are rounded
    big = [np.full(x.shape, 2.0 ** 20)] * 3
    poss = [p for _, p in R.spp_fwd(R.family("const", x.shape, 4))]
    assert not R.grad_family_ok(R.spp_bwd(poss, big, None, np.abs), *big)
    assert not R.grad_family_ok(np.ones(4), np.full(4, 0.5))
    assert not R.grad_family_ok(np.ones(4), np.full(4, 257.0))


def test_sgd_predicate_holds_for_two_steps_and_fails_for_a_third():
    p, g, m = R.sgd_operands(7)
    segs = R.sgd_segs()
    assert len({(wd, lr) for _, _, wd, lr in segs}) == 2
    for step in range(3):
        ok = R.sgd_family_ok(p, g, m, segs, R.SGD_MOMENTUM, R.SGD_GRAD_SCALE, step == 0)
        assert ok == (step < 2), step
        p, m = R.sgd_step(p, g, m, segs, R.SGD_MOMENTUM, R.SGD_GRAD_SCALE, step == 0)


def test_labels_and_tables():
    """the branch labels the GPU test counts, from the shapes alone"""
    assert [R.spp_remap(N * C // 8)[0] for N, C in R.SPP_NC] == ["identity", "permuted", "off", "off"]
    assert R.spp_remap(16)[1][:4] == [0, 2, 4, 6] and R.spp_remap(24)[0] == "permuted"
    rounds = {pl: -(-pl[0] * pl[1] // R.SPP_T) for pl in R.SPP_PLANES}
    assert rounds[(19, 27)] == 2 and 19 * 27 == 513 and rounds[(32, 32)] == 2 and rounds[(7, 9)] == 1
    for pl in R.SPP_PLANES:
        cs = R.spp_cases(pl)
        assert {R.spp_remap(N * C // 8)[0] for N, C, _, _ in cs} == {"identity", "permuted", "off"}
        assert {f for c in cs for f in c[2:]} == set(R.FAMILIES)
    assert R.trips(4096 * 256) == 1 and R.trips(4096 * 256 + 1) == 2 and R.trips(5) == 1
    lab = set()
    for o, c, _ in R.SGD_SEGS:
        lab |= R.sgd_labels(o, c)
    assert lab == {"sgd:float4_only", "sgd:tail", "sgd:scalar_only", "sgd:two_on", "sgd:two_off"}
    assert R.sgd_labels(0, 16384) == {"sgd:float4_only", "sgd:two_on"} and R.sgd_labels(17600, 3) == {"sgd:tail"}
    assert R.sgd_labels(16392, 1203) == {"sgd:tail", "sgd:two_on", "sgd:two_off"} and R.sgd_labels(17610, 1030) == {"sgd:scalar_only"}
    own = R.sgd_owned()
    assert own.sum() == 16384 + 1203 + 3 + 1030 and not own[16384:16392].any() and not own[-8:].any()
    assert len(R.REQUIRED) == len(set(R.REQUIRED)) == 38
    for name in R.FAMILIES:
        x = R.family(name, (2, 5, 6, 64), 1)
        assert x.shape == (2, 5, 6, 64) and R.is_bf16(x)
    x = R.family("planes", (2, 5, 6, 64), 1).reshape(2, 30, 64)
    lo, hi = x.min(axis=1).reshape(-1), x.max(axis=1).reshape(-1)
    assert (hi[:-1] < lo[1:]).all()                     # disjoint ranges per (n, c)
    assert R.is_bf16(R.specials(64, 0)) and np.isinf(R.specials(64, 0)).sum() == 2
