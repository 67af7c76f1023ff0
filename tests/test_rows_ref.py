"""CPU: tests/rows_ref.py - the references tests/test_gpu_rows_exact.py holds the row-wise kernels and the column sums to.
The RNG model is pinned with hand-computed words (an index at and above 2^32 included: the only test of the high index
word anywhere) and against a second, scalar implementation; the LayerNorm reference is pinned to torch's float64
layer_norm autograd; the conditions of the exact families are checked on every case of the GPU tables together with an fp32
emulation in two summation orders that must reproduce the reference bit for bit; the derived bounds are checked against
fp32 emulations; and mutants of host emulations of the launch structures are compared with the unmutated emulation for
exact equality (np.array_equal, the host's counterpart of the GPU file's whole-buffer comparison) on the exact cases, and
judged by the old criteria of tests/test_gpu_detr.py."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref as BN
import rows_ref as R


# ------------------------------------------------------------------------------------------------------------ the RNG
def scalar_word(seed, idx):
    """csrc/common.h once more, one element at a time in Python integers"""
    m = (1 << 64) - 1
    z = (seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    key = z ^ (z >> 31)
    hi = idx >> 32
    x = (idx ^ key ^ hi ^ ((hi << 16) | (hi >> 16))) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x ^ (key >> 32)


def test_rng_model_pinned_words():
    """words worked out by hand from the formulas of csrc/common.h; 2^32 and 2^32 + 5 exercise the high index word, which
    no GPU test can reach (2^32 elements)"""
    assert R.rng_key(0) == 0x6db6ca64564daeaa and R.rng_key(1) == 0x5cc60547776902ba and R.rng_key(R.M64) == 0xd4143a080f05246d
    assert R.rng_key(R.SEED) == 0xdc00cd6d125f74ab
    pins = [(0, 0, 0x505870d2), (1, 5, 0x4c9a60ef), (R.SEED, 5, 0xcdb6268d), (R.SEED, 1 << 32, 0x6a473445),
            (R.SEED, (1 << 32) + 5, 0x827c5719), (R.SEED, 0x123456789A, 0xa0c80da5)]
    for seed, idx, word in pins:
        assert int(R.rng32k(R.rng_key(seed), [idx])[0]) == word == scalar_word(seed, idx), (seed, idx)
    g = np.random.default_rng(0)
    idx = np.concatenate([g.integers(0, 1 << 32, 500, dtype=np.uint64), g.integers(1 << 32, 1 << 63, 500, dtype=np.uint64)])
    for seed in (0, 7, R.SEED, R.M64):
        w = R.rng32k(R.rng_key(seed), idx)
        assert [int(v) for v in w] == [scalar_word(seed, int(i)) for i in idx]
    # the high word enters through xor and rotate: hi = 1 gives lo ^ 0x00010001
    assert int(R.rng32k(R.rng_key(3), [(1 << 32) + 5])[0]) == int(R.rng32k(R.rng_key(3), [5 ^ 0x00010001])[0])


def test_threshold_rule_and_scale():
    assert [R.drop_threshold(p) for p in R.DROP_PS] == [1 << 31, 429496736, 1, 0]
    assert R.drop_threshold(2.0 ** -32) == 1 and R.drop_threshold(2.0 ** -31) == 2 and R.drop_threshold(2.0 ** -60) == 1
    assert float(R.drop_scale(0.5)) == 2.0 and float(R.drop_scale(2.0 ** -33)) == 1.0 and float(R.drop_scale(0.0)) == 1.0
    assert float(R.drop_scale(0.1)) == float(np.float32(1) / np.float32(0.9))
    idx = np.arange(100000, dtype=np.uint64)
    for p in (0.5, 0.1):
        assert abs(R.keep_mask(R.SEED, None, idx, p).mean() - (1 - p)) < 0.005
    assert R.keep_mask(R.SEED, None, idx, 0.0).all() and R.keep_mask(R.SEED, None, idx, 2.0 ** -33).all()
    # the offset is added to the seed, mod 2^64, before the key
    assert np.array_equal(R.keep_mask(R.SEED, R.M64, idx, 0.5), R.keep_mask(R.SEED - 1, None, idx, 0.5))
    assert np.array_equal(R.keep_mask(R.M64, 7, idx, 0.5), R.keep_mask(6, 0, idx, 0.5))


def test_crafted_seed_draws_exactly_the_threshold():
    for p in (0.5, 0.1, 2.0 ** -33):
        thr = R.drop_threshold(p)
        for idx in (0, 5, 2047):
            seed = R.seed_with_word(idx, thr)
            assert scalar_word(seed, idx) == thr
            assert scalar_word(R.seed_with_word(idx, thr - 1), idx) == thr - 1
            i = np.array([idx], dtype=np.uint64)
            assert R.keep_mask(seed, None, i, p)[0] and not R.keep_mask(seed, None, i, p, "keep_gt")[0]


def test_dropout_reference_rounds_once_then_once_more():
    x = R.bf16_pool(4096, 1)
    for p in (0.5, 0.1):
        keep = R.keep_mask(R.SEED, None, np.arange(x.size, dtype=np.uint64), p)
        t = torch.from_numpy(x).float()
        exp = torch.where(torch.from_numpy(keep), (t * float(R.drop_scale(p))).bfloat16().float(), torch.zeros_like(t)).double().numpy()
        assert np.array_equal(R.dropout_ref(x, None, p, R.SEED), exp)
        res = R.bf16_pool(4096, 2)
        exp2 = (torch.from_numpy(res).float() + torch.from_numpy(exp).float()).bfloat16().double().numpy()
        assert np.array_equal(R.dropout_ref(x, res, p, R.SEED), exp2)
    assert not np.array_equal(R.dropout_ref(x, None, 0.1, R.SEED), x * float(R.drop_scale(0.1)))     # the rounding is real


# ----------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("T,E", [(5, 64), (37, 192), (16, 1024)])
def test_reference_is_torch_layer_norm_autograd(T, E):
    g = torch.Generator().manual_seed(T + E)
    x = (torch.randn(T, E, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_()
    gamma = (1 + 0.1 * torch.randn(E, generator=g, dtype=torch.float64)).requires_grad_()
    beta = (0.1 * torch.randn(E, generator=g, dtype=torch.float64)).requires_grad_()
    dy = torch.randn(T, E, generator=g, dtype=torch.float64)
    eps = float(np.float32(1e-5))
    y = F.layer_norm(x, (E,), gamma, beta, eps)
    y.backward(dy)
    yr, mean, rstd = R.ln_fwd(x.detach().numpy(), gamma.detach().numpy(), beta.detach().numpy(), 1e-5)
    dx, dg, db = R.ln_bwd(x.detach().numpy(), dy.numpy(), gamma.detach().numpy(), mean, rstd)
    for a, b in ((yr, y), (dx, x.grad), (dg, gamma.grad), (db, beta.grad)):
        assert np.abs(a - b.detach().numpy()).max() < 1e-11


def as_real(o, beta=None, eps=0.0):
    return types.SimpleNamespace(T=o.T, E=o.E, x=o.x, dy=getattr(o, "dy", np.zeros_like(o.x)), gamma=o.gamma,
                                 beta=o.beta if beta is None else beta, eps=eps)


@pytest.mark.parametrize("E", R.FWD_ES)
def test_forward_families_are_exact_in_fp32_in_two_orders(E):
    """the conditions on every case of the GPU table, and an fp32 emulation (sequential and pairwise sums) that reproduces
    the float64 reference bit for bit; the fused family likewise, its sum res + d formed in fp32"""
    for T in R.FWD_TS:
        for fam in (0, 1):
            o = R.fwd_exact_case(T, E, fam, 1000 * fam + 10 * E + T)
            R.assert_fwd_conditions(o)
            for order in (0, 1):
                e = R.emulate_real_fp32(as_real(o, eps=o.eps), order, o.mean, o.rstd)
                assert np.array_equal(e.y, R.bf16_rne(o.y)) and np.array_equal(e.mean, o.mean) and np.array_equal(e.rstd, o.rstd)
    for T in (1, 5, 37):
        for k, p in enumerate((0.5, 0.1)):
            o = R.fused_fwd_case(T, E, (T + k) % 2, p, R.SEED + 10 * E + T)
            R.assert_fused_conditions(o)
            assert np.array_equal(R.dropout_ref(o.xin.reshape(-1), o.res.reshape(-1), p, o.seed).reshape(T, E), o.t)
    # gamma and beta vary per channel, rows differ: a channel permutation or a row mix-up shows
    assert len(set(o.gamma)) > 2 and len(set(o.beta)) > 2


@pytest.mark.parametrize("E,T", R.bwd_cases())
def test_backward_family_is_exact_in_fp32_and_in_the_launch_structure(E, T):
    o = R.bwd_exact_case(T, E, 7 * E + T)
    R.assert_bwd_conditions(o)
    if T in R.BWD_TS:
        assert R.bwd_rows_per_block(T) == 16
    else:
        assert R.bwd_rows_per_block(T) == 20
    dxr = R.bf16_rne(o.dx)
    e = R.emulate_ln_bwd(o, 0.5)
    assert np.array_equal(e.dx, dxr) and np.array_equal(e.dgamma, o.dgamma) and np.array_equal(e.dbeta, o.dbeta)
    idx = np.arange(T * E, dtype=np.uint64).reshape(T, E)
    assert np.array_equal(e.dx_drop, R.dropped(dxr, R.keep_mask(o.seed, None, idx, 0.5), 0.5))
    if T * E <= 1 << 17:
        for order in (0, 1):
            f = R.emulate_real_fp32(as_real(o, beta=np.zeros(E)), order, o.mean, o.rstd)
            assert np.array_equal(f.dx, dxr) and np.array_equal(f.dgamma, o.dgamma) and np.array_equal(f.dbeta, o.dbeta)


def test_backward_table_covers_the_block_counts_and_last_blocks():
    assert sorted(v[0] for v in R.BWD_TS.values()) == [1, 8, 9, 25, 32, 33, 40]
    assert {v[1] for v in R.BWD_TS.values()} == {1, 15, 16}
    for T, (nblk, last) in R.BWD_TS.items():
        assert -(-T // 16) == nblk and T - (nblk - 1) * 16 == last
    assert {E // 64 for E, _ in R.bwd_cases()} == {1, 2, 4, 8, 16}


@pytest.mark.parametrize("T,E", [(37, 64), (143, 256), (100, 1024), (64, 512), (33, 128), (5, 192), (37, 960)])
def test_real_statistics_bounds_hold_for_an_fp32_emulation(T, E):
    """the bounds of real_fwd_bounds / real_bwd_bounds against fp32 emulations in two summation orders, and they are more
    than an order of magnitude below the old 2e-2"""
    o = R.real_case(T, E, T + E)
    (yr, mr, rr), (by, bm, br) = R.real_fwd_bounds(o)
    m32, r32 = R.f32(mr), R.f32(rr)
    (dxr, dgr, dbr), (bdx, bdg, bdb) = R.real_bwd_bounds(o, m32, r32)
    for order in (0, 1):
        e = R.emulate_real_fp32(o, order, m32, r32)
        rat = [R.ratio(e.y, yr, by), R.ratio(e.mean, mr, bm), R.ratio(e.rstd, rr, br), R.ratio(e.dx, dxr, bdx),
               R.ratio(e.dgamma, dgr, bdg), R.ratio(e.dbeta, dbr, bdb)]
        print("T %d E %d order %d: y %.3f mean %.3f rstd %.3f dx %.3f dgamma %.3f dbeta %.3f" % ((T, E, order) + tuple(rat)))
        assert max(rat) <= 1.0, rat
    assert np.all(by <= 1.25 * R.bf16_half_ulp(np.abs(yr) + by) + 1e-4)       # the bf16 store dominates
    assert by.max() < 2e-2 and np.median(by / (2e-2 + 2e-2 * np.abs(yr))) < 0.1
    assert np.median(bdx / (2e-2 + 2e-2 * np.abs(dxr))) < 0.1 and bdg.max() < 0.1 * 1e-3 * T ** 0.5 and br.max() / rr.max() < 1e-4


# ------------------------------------------------------------------------------------------------- ew and the sigmoid
def test_ew_exact_reference_is_fp32_arithmetic_on_bf16():
    a, b = R.ew_edge_operands(4096, 5)
    ta, tb = torch.from_numpy(a).float(), torch.from_numpy(b).float()
    assert np.array_equal(R.ew_exact(0, a, b), (ta + tb).bfloat16().double().numpy())
    assert np.array_equal(R.ew_exact(1, a, b), torch.relu(ta).double().numpy())
    assert np.array_equal(R.ew_exact(7, a, b), torch.relu((ta + tb).bfloat16().float()).bfloat16().double().numpy())
    assert np.array_equal(R.ew_exact(2, a, b), torch.where(tb > 0, ta, torch.zeros_like(ta)).double().numpy())
    s = R.ew_exact(0, a, b)
    assert np.isinf(s).any() and (s == 0).any() and (np.abs(a) < 2.0 ** -126).any() and (np.abs(a) == R.BF16_MAX).any()


def test_ew_bounds_hold_for_an_fp32_emulation():
    """ops 3 and 5 over every finite bf16 argument, ops 4 and 6 on their grids: torch's fp32 expression (correctly rounded
    operations, an accurate exp) within the bound, and the bound never above one bf16 ulp plus the floor"""
    a = R.all_finite_bf16()
    ta = torch.from_numpy(a).float()
    sg = BN.emulate_sigmoid_fp32(ta)
    for op, emu in ((3, sg), (5, ta / (1.0 + torch.exp(-ta)))):
        ref, bound = R.ew_bound(op, a)
        r = R.ratio(emu.bfloat16().double().numpy(), ref, bound)
        print("op %d: fp32 emulation / bound %.3f" % (op, r))
        assert r <= 1.0 and np.all(bound <= 2.2 * R.bf16_half_ulp(ref) + 1e-29)
    for op in (4, 6):
        a, b = R.ew_grid(op)
        ta, tb = torch.from_numpy(a).float(), torch.from_numpy(b).float()
        s = BN.emulate_sigmoid_fp32(tb)
        emu = ta * tb * (1.0 - tb) if op == 4 else ta * s * (1.0 + tb * (1.0 - s))
        ref, bound = R.ew_bound(op, a, b)
        r = R.ratio(emu.bfloat16().double().numpy(), ref, bound)
        print("op %d: fp32 emulation / bound %.3f over %d points" % (op, r, a.size))
        assert r <= 1.0 and a.size % 8 == 0 and a.size > 8 * 1000


def test_sigmoid_f32_reference_and_exact_backward():
    x = R.sigmoid_f32_args()
    e = R.f32(np.exp(-x))                                     # a correctly rounded expf, then two IEEE operations
    emu = R.f32(1.0 / R.f32(1.0 + e))
    d = float(R.ulps32(emu, R.sigmoid_ref(x)).max())
    print("three correctly rounded fp32 operations: %.3f ulps from float64" % d)
    assert d <= R.SIGMOID_F32_MEASURED + 0.5                   # see the comment at SIGMOID_F32_ULPS
    assert R.SIGMOID_F32_ULPS == R.SIGMOID_F32_MEASURED + 1 == 3.282
    for n in R.SIG_NS[:3]:
        y, dy, ref = R.sigmoid_bwd_case(n, n)
        y32, dy32 = y.astype(np.float32), dy.astype(np.float32)
        assert np.array_equal((dy32 * y32 * (np.float32(1) - y32)).astype(np.float64), ref)
        assert np.array_equal((dy32 * (y32 * (np.float32(1) - y32))).astype(np.float64), ref)


# --------------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("C", [8, 60, 72, 200])
@pytest.mark.parametrize("npix", [1, 257, 2049])
def test_colsum_reference_and_block_structure(npix, C):
    x = R.col_values(npix, C, C + npix)
    assert np.array_equal(x, R.col_values(npix, C, C + npix, "cpu").numpy())
    for sq in (0, 1):
        R.assert_col_conditions(x, sq)
        for narrow in ((False, True) if C <= 128 and not sq else (False,)):
            assert np.array_equal(R.emulate_colsum(x, C, sq, narrow), R.col_ref(x, sq))
    assert [R.col_path(c, False) for c in (4096, 4104)] == ["colsum_wide_fused", "colsum_wide_stage1+2"]
    assert R.col_blocks(128 * 256 + 1, 64, False) == 128 and R.col_blocks(257, 64, False) == 2 and R.col_cp(60) == 64


# ------------------------------------------------------------------------------------------------------------- mutants
def same(a, b):
    return np.array_equal(a, b)


# which outputs of a mutant the OLD criteria of tests/test_gpu_detr.py (2e-2 on y / dx, 1e-3 * sqrt(T) on dgamma / dbeta and
# the column sums, a keep rate for the dropout masks) accept.  Mutants whose every changed output the old criteria reject
# too: dgamma_last_row, s2_no_1_over_E, mean_wrong_row, skip_unroll_boundary, wrong_c0 (gross on that data); fwd_lane_map is
# rejected by test_gpu_detr_meta.py at E = 256 and by nothing at the four other widths.
def test_every_mutant_is_caught_by_an_exact_case_and_what_the_old_criteria_say():
    caught, old = {}, {}
    # --- the backward kernels, on the exact family (nblk = 33, a last block of 15 rows) and on Gaussian data
    o = R.bwd_exact_case(527, 128, 9)
    R.assert_bwd_conditions(o)
    ref = R.emulate_ln_bwd(o, 0.5)
    assert ref.nblk == 33 and same(ref.dgamma, o.dgamma) and same(ref.dx, R.bf16_rne(o.dx))
    rc = R.real_case(527, 128, 4)
    _, rc.mean, rc.rstd = R.ln_fwd(rc.x, rc.gamma, rc.beta, rc.eps)
    rc.seed = 9
    rref = R.emulate_ln_bwd(rc, 0.5)
    T = rc.T
    for m in ("fwd_lane_map", "dgamma_last_row", "s2_no_1_over_E", "mean_wrong_row", "skip_unroll_boundary"):
        e, r = R.emulate_ln_bwd(o, 0.5, mutant=m), R.emulate_ln_bwd(rc, 0.5, mutant=m)
        caught[m] = [k for k in ("dx", "dx_drop", "dgamma", "dbeta") if not same(getattr(e, k), getattr(ref, k))]
        old[m] = dict(dx=R.old_ln_close(r.dx, rref.dx), dgamma=R.old_param_close(r.dgamma, rref.dgamma, T),
                      dbeta=R.old_param_close(r.dbeta, rref.dbeta, T), dx_drop=R.old_keep_rate_ok(r.dx_drop != 0, 0.5))
    # the forward's lane map is the backward's only at PER = 1
    o64 = R.bwd_exact_case(33, 64, 1)
    assert same(R.emulate_ln_bwd(o64, 0.5, mutant="fwd_lane_map").dx_drop, R.emulate_ln_bwd(o64, 0.5).dx_drop)
    # --- the keep test and the offset, on mi_dropout_bf16
    n = 8 * 255
    x = R.bf16_pool(n, 3)
    for p in (0.5, 2.0 ** -33):
        seed = R.seed_with_word(5, R.drop_threshold(p))
        a, b = R.dropout_ref(x, None, p, seed), R.dropout_ref(x, None, p, seed, mutant="keep_gt")
        assert not same(a, b) and np.flatnonzero(a != b).tolist() == [5]
    caught["keep_gt"] = ["out"]
    idx = np.arange(100000, dtype=np.uint64)
    old["keep_gt"] = dict(out=R.old_keep_rate_ok(R.keep_mask(R.SEED, None, idx, 0.5, "keep_gt"), 0.5))
    assert same(R.dropout_ref(x, None, 0.5, R.SEED, 0, "offset_after_key"), R.dropout_ref(x, None, 0.5, R.SEED, 0))
    caught["offset_after_key"] = ["out"] if all(
        not same(R.dropout_ref(x, None, 0.5, R.SEED, off, "offset_after_key"), R.dropout_ref(x, None, 0.5, R.SEED, off)) for off in (7, R.M64)) else []
    old["offset_after_key"] = dict(out=R.old_keep_rate_ok(R.keep_mask(R.SEED, 7, idx, 0.5, "offset_after_key"), 0.5))
    # --- the threshold floor: at p = 2^-33 only the word 0 separates thr = 1 from thr = 0.  R.SEED and the seed crafted for
    # `>=` (word 1) drop nothing either way, so they cannot catch it; the seed whose element 5 draws 0 does, at that element
    p = R.FLOOR_P
    assert R.drop_threshold(p) == 1 and R.drop_threshold(p, floor=False) == 0 and R.drop_threshold(0.5, floor=False) == 1 << 31
    for seed in (R.SEED, R.seed_with_word(5, 1)):
        assert same(R.dropout_ref(x, None, p, seed, mutant="thr_floor_missing"), R.dropout_ref(x, None, p, seed)) and same(R.dropout_ref(x, None, p, seed), x)
    seed = R.seed_with_word(5, 0)
    a, b = R.dropout_ref(x, None, p, seed), R.dropout_ref(x, None, p, seed, mutant="thr_floor_missing")
    assert np.flatnonzero(a != x).tolist() == [5] and a[5] == 0 and same(b, x)
    caught["thr_floor_missing"] = ["out"] if np.flatnonzero(a != b).tolist() == [5] else []
    old["thr_floor_missing"] = dict(out=R.old_keep_rate_ok(R.keep_mask(seed, None, idx, p, "thr_floor_missing"), p))
    # --- the column sums: two chunks
    xc = R.col_values(257, 72, 1)
    caught["wrong_c0"] = ["out"] if not same(R.emulate_colsum(xc, 72, 0, False, "wrong_c0"), R.col_ref(xc, 0)) else []
    g = np.random.default_rng(1).standard_normal((4200, 256))
    old["wrong_c0"] = dict(out=R.old_param_close(R.emulate_colsum(g, 256, 0, False, "wrong_c0"), g.sum(0), 4200))
    # --- relu(a + b): rounding is monotone and fixes 0, so rounding once IS rounding twice - an equivalent mutant, shown
    # here on every pair of the edge table; what a fused add + relu can get wrong is the order, relu_before_add
    a, b = R.ew_edge_operands(4096, 5)
    assert same(R.ew_exact(7, a, b, "relu_add_rounded_once"), R.ew_exact(7, a, b))
    caught["relu_add_rounded_once"] = ["equivalent"]
    assert not same(R.ew_exact(7, a, b, "relu_before_add"), R.ew_exact(7, a, b))
    for m in R.MUTANTS:
        print("%-24s caught through %-28s old criteria accept: %s" % (m, caught[m], old.get(m)))
        assert caught[m], m
    assert caught["fwd_lane_map"] == ["dx_drop"] and caught["dgamma_last_row"] == ["dgamma", "dbeta"]
    assert caught["skip_unroll_boundary"] == ["dgamma", "dbeta"] and "dx" in caught["s2_no_1_over_E"] and "dx" in caught["mean_wrong_row"]
    # the old criteria: the masks pass a keep-rate test whatever their indexing, threshold or seed
    assert old["fwd_lane_map"]["dx_drop"] and old["keep_gt"]["out"] and old["offset_after_key"]["out"] and old["thr_floor_missing"]["out"]
    assert all(old[m]["dx_drop"] for m in ("dgamma_last_row", "s2_no_1_over_E", "mean_wrong_row", "skip_unroll_boundary"))
    # ... and these the old criteria reject as well
    assert not old["dgamma_last_row"]["dgamma"] and not old["skip_unroll_boundary"]["dgamma"] and not old["s2_no_1_over_E"]["dx"]
    assert not old["wrong_c0"]["out"] and not old["mean_wrong_row"]["dgamma"] and not old["mean_wrong_row"]["dx"]
    assert len(R.MUTANTS) == 10 and [m for m in R.MUTANTS if caught[m] == ["equivalent"]] == ["relu_add_rounded_once"]
