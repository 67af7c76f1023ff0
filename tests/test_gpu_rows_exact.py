"""GPU (-m gpu): the row-wise kernels of csrc/transformer_ops.hip - LayerNorm forward / backward and their fused dropout
forms, mi_dropout_bf16 / mi_dropout_add_bf16, mi_ew_bf16, mi_sigmoid_f32 - and the column sums of csrc/misc_ops.hip against
the plain float64 / integer references of tests/rows_ref.py with NO tolerance, through the C ABI by ctypes.

The method (tests/rows_ref.py): the keep bits of every dropout form come from an integer model of the RNG on the host; the
LayerNorm and column-sum operands are families on which every fp32 operation is exact in any order, so the device must
equal float64, rounded once where a kernel stores bf16, bit for bit.  The conditions are asserted on the reference of every
case before anything is launched.  What the exact families cannot reach - rsqrtf, __expf, expf, real statistics - is held to
a measured ulp cap (RSTD_ULPS, SIGMOID_F32_ULPS: printed before they are asserted) or to derived elementwise bounds.

Hygiene of every launch: every output lives in a buffer of sentinel words that must survive, is pre-filled with NaN and must
have been written entirely; inputs hold NaN outside their views; workspaces are NaN-filled and guarded.  The launched
instantiations are counted and the table must be complete.

Not seen from here: the high index word of the RNG (idx >= 2^32 needs 2^32 elements)."""
import collections
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rows_ref as R
from yolov7_d2_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -1536.0
GUARD = 64
NAN = float("nan")
F64 = torch.float64
BF, F32 = torch.bfloat16, torch.float32
SEEN = collections.Counter()


@pytest.fixture(autouse=True)
def no_colsum_switch(monkeypatch):
    """mi_colsum_*_wide reads MI_COLSUM_TWO_STAGE on every call: with it set the one-launch form would never run, and the
    coverage labels, which come from rows_ref.col_path on the host, would claim a kernel that was not launched"""
    monkeypatch.delenv("MI_COLSUM_TWO_STAGE", raising=False)


def sp():
    return L.stream_ptr()


def T_(a, dtype=F64):
    """numpy -> device tensor"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV).to(dtype)


class Buf:
    """rows x width elements at row stride ld inside a flat buffer with GUARD elements before and after: `fill` in the view,
    `other` everywhere else (SENT for outputs, NaN for inputs)"""

    def __init__(self, nrows, width, ld, dtype, fill=NAN, other=SENT):
        self.nrows, self.width, self.ld, self.other = nrows, width, ld, other
        self.flat = torch.full((nrows * ld + 2 * GUARD,), other, dtype=dtype, device=DEV)
        self.set(fill)

    def _v(self):
        return self.flat[GUARD:GUARD + self.nrows * self.ld].view(self.nrows, self.ld)[:, :self.width]

    def set(self, fill):
        if isinstance(fill, np.ndarray):
            fill = T_(fill)
        if torch.is_tensor(fill):
            fill = fill.reshape(self.nrows, self.width).to(DEV).to(self.flat.dtype)
        self._v()[...] = fill

    @property
    def ptr(self):
        return self.flat.data_ptr() + GUARD * self.flat.element_size()

    def view(self):
        return self._v().to(F64)

    def np(self):
        return self.view().cpu().numpy()

    def complaint(self, name, value):
        """None if the WHOLE buffer is `value` (NaN = NaN) in the view and untouched elsewhere"""
        if isinstance(value, np.ndarray):
            value = T_(value)
        exp = torch.full(self.flat.shape, self.other, dtype=F64, device=DEV)
        exp[GUARD:GUARD + self.nrows * self.ld].view(self.nrows, self.ld)[:, :self.width] = value.reshape(self.nrows, self.width).to(DEV).to(F64)
        got = self.flat.to(F64)
        bad = ~((got == exp) | (got.isnan() & exp.isnan()))
        if not bool(bad.any()):
            return None
        i = int(torch.nonzero(bad)[0])
        return "%s: %d elements differ (%d NaN in the view), first at flat %d (row %d, column %d): got %r, expected %r" % (
            name, int(bad.sum()), int(self.view().isnan().sum()), i - GUARD, (i - GUARD) // self.ld, (i - GUARD) % self.ld,
            float(got[i]), float(exp[i]))

    def guards(self, name):
        """None if everything outside the view is untouched and the view holds no NaN"""
        v = self.view()
        if bool(v.isnan().any()):
            return "%s: %d elements were not written" % (name, int(v.isnan().sum()))
        return self.complaint(name + " (outside the view)", v)


def out_bf(n, width=None):
    return Buf(1, n, n, BF) if width is None else Buf(n, width, width, BF)


def in_buf(a, dtype=BF):
    a = np.asarray(a, dtype=np.float64)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    return Buf(a.shape[0], a.shape[1], a.shape[1], dtype, a, NAN)


def vec(a_or_n, dtype=F32):
    """input vector from an array; output vector (NaN inside sentinels) from a length"""
    if isinstance(a_or_n, int):
        return Buf(1, a_or_n, a_or_n, dtype)
    return in_buf(a_or_n, dtype)


class seed_offset:
    """install a device word with mi_dropout_seed_offset, always uninstall it"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        if self.value is not None:
            v = self.value if self.value < 1 << 63 else self.value - (1 << 64)
            self.word = torch.tensor([v], dtype=torch.int64, device=DEV)
            L.check(L.lib().mi_dropout_seed_offset(self.word.data_ptr()), "seed_offset")
        return self

    def __exit__(self, *a):
        L.check(L.lib().mi_dropout_seed_offset(None), "seed_offset(NULL)")
        torch.cuda.synchronize()


def f(p):
    return float(np.float32(p))


# ------------------------------------------------------------------------------------------------------------- dropout
def run_dropout(n, p, seed, with_res, offset=None, x=None, res=None):
    x = R.bf16_pool(n, 3) if x is None else x
    res = (R.bf16_pool(n, 4) if res is None else res) if with_res else None
    xb, rb, ob = in_buf(x), (in_buf(res) if with_res else None), out_bf(n)
    if with_res:
        L.check(L.lib().mi_dropout_add_bf16(xb.ptr, rb.ptr, ob.ptr, n, f(p), C.c_uint64(seed), sp()), "dropout_add")
    else:
        L.check(L.lib().mi_dropout_bf16(xb.ptr, ob.ptr, n, f(p), C.c_uint64(seed), sp()), "dropout")
    torch.cuda.synchronize()
    SEEN["dropout_kernel" + ("+res" if with_res else "")] += 1
    ref = R.dropout_ref(x, res, p, seed, offset)
    return [s for s in [ob.complaint("dropout%s n %d p %g seed %x offset %r" % ("_add" if with_res else "", n, p, seed, offset), ref)] if s]


@pytest.mark.parametrize("n", R.DROP_NS)
def test_dropout_is_the_host_model_bit_for_bit(n):
    """mi_dropout_bf16 / mi_dropout_add_bf16 at p in {0.5, 0.1, 2^-33 (the thr = 1 floor), 0}: the keep bits of the integer
    model, kept values bf16(fp32(x) * fp32(1 / (1 - p))), the residual form's second rounding; the last n makes the
    grid-stride loop run (its mask must continue the index sequence).  At the small sizes a crafted seed makes element 5
    draw exactly the threshold (kept: `>=`), and at p = 2^-33 another makes it draw the word 0: the floor's threshold of 1
    drops exactly that element, a threshold of 0 would keep it (R.SEED and the first crafted seed drop nothing there)."""
    x, res = R.bf16_pool(n, 3), R.bf16_pool(n, 4)
    bad = []
    idx = np.arange(n, dtype=np.uint64)
    for p in R.DROP_PS:
        seeds = [R.SEED]
        if n <= 8 * 257 and p > 0:
            seeds.append(R.seed_with_word(5, R.drop_threshold(p)))
            assert bool(R.keep_mask(seeds[-1], None, np.array([5], dtype=np.uint64), p)[0])
        if n <= 8 * 257 and p == R.FLOOR_P:
            seeds.append(R.seed_with_word(5, 0))
            assert np.flatnonzero(~R.keep_mask(seeds[-1], None, idx, p)).tolist() == [5] and x[5] != 0
            assert R.keep_mask(seeds[-1], None, idx, p, "thr_floor_missing").all()
        for seed in seeds:
            for with_res in (False, True):
                bad += run_dropout(n, p, seed, with_res, None, x, res)
    assert bad == [], bad


MHA_MASK_SHAPE = (2, 3, 5, 7)


def run_mha_mask(ps=(0.5, 0.1), seed=R.SEED):
    B, H, Lq, Lk = MHA_MASK_SHAPE
    n = B * H * Lq * Lk
    bad = []
    for p in ps:
        ob = Buf(1, n, n, torch.uint8, 255, 77)
        L.check(L.lib().mi_mha_dropout_mask(ob.ptr, B, H, Lq, Lk, f(p), C.c_uint64(seed), sp()), "mha_dropout_mask")
        torch.cuda.synchronize()
        SEEN["mha_mask_kernel"] += 1
        keep = R.keep_mask(seed, None, np.arange(n, dtype=np.uint64), p)
        s = ob.complaint("mha mask p %g" % p, keep.astype(np.float64))
        bad += [s] if s else []
    return bad


def test_mha_dropout_mask_is_the_host_model():
    """the entry tests/mha_ref.py takes its keep bits from: uint8 [B][H][Lq][Lk], element i draws index i"""
    assert run_mha_mask() == []


# ----------------------------------------------------------------------------------------------------------- LayerNorm
def check_stats(o, mean, rstd, worst):
    bad = []
    s = mean.complaint("mean", o.mean)
    bad += [s] if s else []
    s = rstd.guards("rstd")
    bad += [s] if s else []
    d = float(R.ulps32(rstd.np().reshape(-1), o.rstd).max())
    worst[0] = max(worst[0], d)
    if not d <= R.RSTD_ULPS:
        bad.append("rstd: %g ulps from float64 (cap %d)" % (d, R.RSTD_ULPS))
    return bad


def run_ln_fwd(o, worst):
    R.assert_fwd_conditions(o)
    x, g, b = in_buf(o.x), vec(o.gamma), vec(o.beta)
    y, mean, rstd = out_bf(o.T, o.E), vec(o.T), vec(o.T)
    L.check(L.lib().mi_layernorm_fwd(x.ptr, g.ptr, b.ptr, y.ptr, mean.ptr, rstd.ptr, o.T, o.E, o.eps, sp()), "ln_fwd")
    torch.cuda.synchronize()
    SEEN["layernorm_fwd_kernel<plain>"] += 1
    s = y.complaint("y", R.bf16_rne(o.y))
    return ["T %d E %d family %d: %s" % (o.T, o.E, o.family, m) for m in ([s] if s else []) + check_stats(o, mean, rstd, worst)]


def run_ln_fused_fwd(o, worst, offset=None):
    R.assert_fused_conditions(o)
    x, res, g, b = in_buf(o.xin), in_buf(o.res), vec(o.gamma), vec(o.beta)
    so, y, mean, rstd = out_bf(o.T, o.E), out_bf(o.T, o.E), vec(o.T), vec(o.T)
    L.check(L.lib().mi_dropout_add_layernorm_fwd(x.ptr, res.ptr, so.ptr, g.ptr, b.ptr, y.ptr, mean.ptr, rstd.ptr, o.T, o.E, o.eps,
                                                 f(o.p), C.c_uint64(o.seed), sp()), "dropout_add_ln_fwd")
    torch.cuda.synchronize()
    SEEN["layernorm_fwd_kernel<fused>"] += 1
    bad = [s for s in (so.complaint("sum_out", o.t), y.complaint("y", R.bf16_rne(o.y))) if s] + check_stats(o, mean, rstd, worst)
    return ["fused T %d E %d family %d p %g offset %r: %s" % (o.T, o.E, o.family, o.p, offset, m) for m in bad]


@pytest.mark.parametrize("E", R.FWD_ES)
def test_layernorm_fwd_exact(E):
    """every E the forward takes, T in {1, 3, 4, 5, 37} (four rows per block: ragged last blocks), both families: y and mean
    bit for bit, rstd within RSTD_ULPS of float64"""
    bad, worst = [], [0.0]
    for T in R.FWD_TS:
        for fam in (0, 1):
            bad += run_ln_fwd(R.fwd_exact_case(T, E, fam, 1000 * fam + 10 * E + T), worst)
    print("layernorm_fwd E %d: worst rstd distance %g ulps (cap RSTD_ULPS = %d)" % (E, worst[0], R.RSTD_ULPS))
    assert bad == [], bad[:8]


@pytest.mark.parametrize("E", R.FWD_ES)
def test_dropout_add_layernorm_fwd_exact(E):
    """the fused forward at p in {0.5, 0.1}: keep bits from the host model (index row * E + lane + 64 j = the element's linear
    index), res = t - d so that sum_out = t; sum_out, y, mean bit for bit, rstd within RSTD_ULPS"""
    bad, worst = [], [0.0]
    for T in (1, 5, 37):
        for k, p in enumerate((0.5, 0.1)):
            bad += run_ln_fused_fwd(R.fused_fwd_case(T, E, (T + k) % 2, p, R.SEED + 10 * E + T), worst)
    print("dropout_add_layernorm_fwd E %d: worst rstd distance %g ulps (cap RSTD_ULPS = %d)" % (E, worst[0], R.RSTD_ULPS))
    assert bad == [], bad[:8]


def run_ln_bwd(o, p=None, offset=None):
    """p None: mi_layernorm_bwd; else mi_layernorm_bwd_dropout"""
    R.assert_bwd_conditions(o)
    T, E = o.T, o.E
    rpb = R.bwd_rows_per_block(T)
    nblk = -(-T // rpb)
    x, dy, g, mean, rstd = in_buf(o.x), in_buf(o.dy), vec(o.gamma), vec(o.mean), vec(o.rstd)
    dx, dg, db = out_bf(T, E), vec(E), vec(E)
    nws = -(-T // 16) * E * 2
    ws = Buf(1, nws, nws, F32)
    dd = None
    if p is None:
        rc = L.lib().mi_layernorm_bwd(x.ptr, dy.ptr, g.ptr, mean.ptr, rstd.ptr, dx.ptr, dg.ptr, db.ptr, ws.ptr, T, E, sp())
    else:
        dd = out_bf(T, E)
        rc = L.lib().mi_layernorm_bwd_dropout(x.ptr, dy.ptr, g.ptr, mean.ptr, rstd.ptr, dx.ptr, dd.ptr, dg.ptr, db.ptr, ws.ptr, T, E,
                                              f(p), C.c_uint64(o.seed), sp())
    L.check(rc, "ln_bwd")
    torch.cuda.synchronize()
    SEEN["layernorm_bwd_kernel<%d>%s" % (E // 64, "" if p is None else "+dx_drop")] += 1
    SEEN["layernorm_bwd_params_kernel"] += 1
    dxr = R.bf16_rne(o.dx)
    bad = [dx.complaint("dx", dxr), dg.complaint("dgamma", o.dgamma), db.complaint("dbeta", o.dbeta)]
    if dd is not None:
        idx = np.arange(T * E, dtype=np.uint64).reshape(T, E)
        bad.append(dd.complaint("dx_drop", R.dropped(dxr, R.keep_mask(o.seed, offset, idx, p), p)))
    w = ws.view().reshape(-1)
    used = nblk * E * 2
    if bool(w[:used].isnan().any()):
        bad.append("ws: %d of the %d partial words were not written" % (int(w[:used].isnan().sum()), used))
    if not bool(w[used:].isnan().all()):
        bad.append("ws: words past [nblk = %d][E][2] were written" % nblk)
    bad.append(ws.complaint("ws (outside)", ws.view()))
    return ["bwd T %d E %d p %r offset %r: %s" % (T, E, p, offset, m) for m in bad if m]


@pytest.mark.parametrize("E,T", R.bwd_cases())
def test_layernorm_bwd_exact(E, T):
    """every PER with and without dx_drop; block counts 1, 8, 9, 25, 32, 33, 40 (both loops of the parameter kernel and
    their boundaries), last blocks of 1, 15 and 16 rows, and 8193 rows at E = 64 (20 rows per block): dx (rounded once),
    dgamma, dbeta bit for bit against float64; dx_drop the host model's mask on the bf16 dx; the NaN-filled workspace
    written up to [nblk][E][2] and not beyond"""
    if T in R.BWD_TS:
        assert (-(-T // 16), T - (-(-T // 16) - 1) * 16) == R.BWD_TS[T]
    else:
        assert R.bwd_rows_per_block(T) > 16
    o = R.bwd_exact_case(T, E, 7 * E + T)
    bad = run_ln_bwd(o) + run_ln_bwd(o, 0.5) + run_ln_bwd(o, 0.1)
    assert bad == [], bad[:8]


def test_layernorm_bwd_refuses_e_192_which_the_forward_takes():
    E, T = 192, 5
    z = torch.zeros(T * E, dtype=BF, device=DEV)
    outs = [out_bf(T, E), vec(E), vec(E), Buf(1, 2 * E, 2 * E, F32)]
    st = torch.ones(T, dtype=F32, device=DEV)
    gm = torch.ones(E, dtype=F32, device=DEV)
    rc = L.lib().mi_layernorm_bwd(z.data_ptr(), z.data_ptr(), gm.data_ptr(), st.data_ptr(), st.data_ptr(), outs[0].ptr, outs[1].ptr,
                                  outs[2].ptr, outs[3].ptr, T, E, sp())
    torch.cuda.synchronize()
    assert rc == R.MI_EINVAL and b"192" in L.lib().mi_last_error()
    for b in outs:
        assert b.complaint("refused launch", torch.full((b.nrows, b.width), NAN, dtype=F64)) is None
    assert run_ln_fwd(R.fwd_exact_case(5, 192, 0, 5), [0.0]) == []


REAL_CASES = [(37, 64, True), (143, 256, True), (100, 1024, True), (64, 512, True), (33, 128, True), (5, 192, False), (37, 960, False)]


@pytest.mark.parametrize("T,E,bwd", REAL_CASES)
def test_layernorm_real_statistics_within_derived_bounds(T, E, bwd):
    """Gaussian rows (offset 0.5, scale 2), eps 1e-5: y, mean, rstd, dx, dgamma, dbeta within the elementwise bounds of
    rows_ref.real_*_bounds (bf16 half-ulp of the reference plus fp32 terms proportional to the chain lengths).  The
    backward gets the float64 statistics rounded to fp32, not the device's."""
    o = R.real_case(T, E, T + E)
    (yr, mr, rr), (by, bm, br) = R.real_fwd_bounds(o)
    x, g, b = in_buf(o.x), vec(o.gamma), vec(o.beta)
    y, mean, rstd = out_bf(T, E), vec(T), vec(T)
    L.check(L.lib().mi_layernorm_fwd(x.ptr, g.ptr, b.ptr, y.ptr, mean.ptr, rstd.ptr, T, E, f(o.eps), sp()), "ln_fwd")
    torch.cuda.synchronize()
    rat = dict(y=R.ratio(y.np(), yr, by), mean=R.ratio(mean.np().reshape(-1), mr, bm), rstd=R.ratio(rstd.np().reshape(-1), rr, br))
    bad = [s for s in (y.guards("y"), mean.guards("mean"), rstd.guards("rstd")) if s]
    if bwd:
        m32, r32 = R.f32(mr), R.f32(rr)
        (dxr, dgr, dbr), (bdx, bdg, bdb) = R.real_bwd_bounds(o, m32, r32)
        dy, mi, ri = in_buf(o.dy), vec(m32), vec(r32)
        dx, dg, db = out_bf(T, E), vec(E), vec(E)
        nws = -(-T // 16) * E * 2
        ws = Buf(1, nws, nws, F32)
        L.check(L.lib().mi_layernorm_bwd(x.ptr, dy.ptr, g.ptr, mi.ptr, ri.ptr, dx.ptr, dg.ptr, db.ptr, ws.ptr, T, E, sp()), "ln_bwd")
        torch.cuda.synchronize()
        rat.update(dx=R.ratio(dx.np(), dxr, bdx), dgamma=R.ratio(dg.np().reshape(-1), dgr, bdg), dbeta=R.ratio(db.np().reshape(-1), dbr, bdb))
        bad += [s for s in (dx.guards("dx"), dg.guards("dgamma"), db.guards("dbeta")) if s]
    print("layernorm real statistics T %d E %d: worst |device - float64| / bound: %s" % (
        T, E, ", ".join("%s %.3f" % kv for kv in rat.items())))
    assert bad == [] and all(v <= 1.0 for v in rat.values()), (bad, rat)


@pytest.mark.parametrize("offset", R.OFFSETS)
def test_seed_offset_enters_before_the_key_and_wraps(offset):
    """a device word installed with mi_dropout_seed_offset (0, 7, 2^64 - 1): the four kernels that add it equal the model at
    seed + offset mod 2^64; mi_mha_dropout_mask ignores it"""
    bad, worst = [], [0.0]
    with seed_offset(offset):
        n = 8 * 257
        for with_res in (False, True):
            bad += run_dropout(n, 0.5, R.SEED, with_res, offset)
        o = R.fused_fwd_case(5, 128, 0, 0.5, R.SEED + 1, offset)
        bad += run_ln_fused_fwd(o, worst, offset)
        bad += run_ln_bwd(R.bwd_exact_case(143, 128, 9), 0.5, offset)
        bad += run_mha_mask()
    if offset:                                         # the word is uninstalled: the same launch is the model without it again
        bad += run_dropout(8 * 257, 0.5, R.SEED, False, None)
    assert bad == [], bad[:8]


def test_threshold_floor_drops_the_one_element_that_draws_word_zero():
    """p = 2^-33 gives (unsigned)(p 2^32) = 0, which drop_threshold raises to 1: the only word below it is 0.  The library
    forms the threshold in three places (the dropout entries, drop_threshold() of the two fused LayerNorm forms, the
    attention parameters behind mi_mha_dropout_mask); in each a seed crafted so that ONE chosen element draws the word 0
    must drop exactly that element.  Asserted on the host for every case: the expected mask has that one zero, the element's
    value is not 0, and the same launch with a threshold of 0 (mutant thr_floor_missing) would keep everything."""
    p, bad, worst = R.FLOOR_P, [], [0.0]

    def only_drop(seed, n, k):
        idx = np.arange(n, dtype=np.uint64)
        assert np.flatnonzero(~R.keep_mask(seed, None, idx, p)).tolist() == [k]
        assert R.keep_mask(seed, None, idx, p, "thr_floor_missing").all()

    n, k = 8 * 257, 2051                               # in the second block of dropout_kernel
    x = R.bf16_pool(n, 3)
    seed = R.seed_with_word(k, 0)
    only_drop(seed, n, k)
    assert x[k] != 0
    for with_res in (False, True):
        bad += run_dropout(n, p, seed, with_res, None, x)
    T, E, k = 5, 128, 3 * 128 + 77                     # the fused forward: row 3, lane 13 + 64 * 1
    seed = R.seed_with_word(k, 0)
    only_drop(seed, T * E, k)
    o = R.fused_fwd_case(T, E, 0, p, seed)
    assert np.flatnonzero(o.d == 0).tolist() == [k] and o.xin.reshape(-1)[k] != 0
    bad += run_ln_fused_fwd(o, worst)
    o = R.bwd_exact_case(33, 128, 9)                   # the backward: three blocks, PER = 2, a row of the second
    dxr = R.bf16_rne(o.dx).reshape(-1)
    k = int(np.flatnonzero(dxr[17 * 128:] != 0)[0]) + 17 * 128
    o.seed = R.seed_with_word(k, 0)
    only_drop(o.seed, 33 * 128, k)
    bad += run_ln_bwd(o, p)
    n, k = int(np.prod(MHA_MASK_SHAPE)), 101
    seed = R.seed_with_word(k, 0)
    only_drop(seed, n, k)
    bad += run_mha_mask((p,), seed)
    assert bad == [], bad[:8]


# ---------------------------------------------------------------------------------------------------------- mi_ew_bf16
def run_ew(op, a, b, ref=None, bound=None):
    """-> complaints, worst bound ratio"""
    n = a.size
    ab, bb, ob = in_buf(a), (in_buf(b) if b is not None else None), out_bf(n)
    L.check(L.lib().mi_ew_bf16(ab.ptr, bb.ptr if bb else None, ob.ptr, n, op, sp()), "ew_bf16 op %d" % op)
    torch.cuda.synchronize()
    SEEN["ew_kernel<op%d>" % op] += 1
    if bound is None:
        s = ob.complaint("ew op %d n %d" % (op, n), R.ew_exact(op, a, b) if ref is None else ref)
        return ([s] if s else []), 0.0
    s = ob.guards("ew op %d n %d" % (op, n))
    return ([s] if s else []), R.ratio(ob.np().reshape(-1), ref, bound)


def ew_operands(op, n):
    a, b = R.ew_edge_operands(n, 20 + op)
    if op == 2 and n >= 8:                             # y = -0, NaN, a subnormal: dx = 0, 0, dy
        b = b.copy()
        b[1], b[2], b[3] = -0.0, NAN, 2.0 ** -133
        a = a.copy()
        a[1:4] = 3.0
    if op in (3, 5, 6):                                # keep the arguments of the exponential where the bound is meaningful
        b = np.clip(b, -128, 128)
        a = np.clip(a, -128, 128)
    if op == 4:
        b = np.clip(np.abs(b), 0, 1)
        a = np.clip(a, -128, 128)
    return a, (None if op in R.EW_UNARY else b)


@pytest.mark.parametrize("n", R.EW_NS)
def test_ew_sizes_all_ops(n):
    """every op at n in {8, 8 * 255, 8 * 257, above 8 * 256 * 2048 (the grid-stride loop)} with guarded outputs: ops 0, 1, 2, 7
    bit for bit on operands with +-0, subnormals, the largest finite bf16 and sums that overflow; ops 3 .. 6 within their
    derived bounds"""
    bad, rat = [], {}
    for op in range(8):
        a, b = ew_operands(op, n)
        if op in (0, 1, 2, 7):
            bad += run_ew(op, a, b)[0]
        else:
            ref, bound = R.ew_bound(op, a, b)
            c, rat[op] = run_ew(op, a, b, ref, bound)
            bad += c
    print("mi_ew_bf16 n %d: worst |device - float64| / bound: %s" % (n, ", ".join("op %d %.3f" % kv for kv in rat.items())))
    assert bad == [] and all(v <= 1.0 for v in rat.values()), (bad[:6], rat)


def test_ew_relu_bwd_keys_on_y_greater_than_zero():
    a = np.full(8, 3.0)
    b = np.array([-0.0, NAN, 0.0, 2.0 ** -133, -2.0 ** -133, 1.0, -1.0, R.BF16_MAX])
    exp = np.array([0.0, 0.0, 0.0, 3.0, 0.0, 3.0, 0.0, 3.0])
    assert np.array_equal(R.ew_exact(2, a, b), exp)
    assert run_ew(2, a, b, exp)[0] == []


@pytest.mark.parametrize("op", [3, 5])
def test_ew_sigmoid_and_swish_over_every_finite_bf16(op):
    """all 65 280 finite bf16 arguments against float64 within half a bf16 ulp plus the derived fp32 error of
    1 / (1 + __expf(-x)) (x / (1 + __expf(-x)))"""
    a = R.all_finite_bf16()
    ref, bound = R.ew_bound(op, a)
    bad, r = run_ew(op, a, None, ref, bound)
    print("mi_ew_bf16 op %d over every finite bf16: worst |device - float64| / bound %.3f" % (op, r))
    assert bad == [] and r <= 1.0, (bad, r)


@pytest.mark.parametrize("op", [4, 6])
def test_ew_sigmoid_and_swish_backward_on_a_grid(op):
    a, b = R.ew_grid(op)
    ref, bound = R.ew_bound(op, a, b)
    bad, r = run_ew(op, a, b, ref, bound)
    print("mi_ew_bf16 op %d on %d grid points: worst |device - float64| / bound %.3f" % (op, a.size, r))
    assert bad == [] and r <= 1.0, (bad, r)


def test_ew_argument_checks_write_nothing():
    n = 16
    a, b, o = in_buf(np.ones(n + 8)), in_buf(np.ones(n + 8)), out_bf(n + 8)
    lib = L.lib()
    calls = [("n % 8", (a.ptr, b.ptr, o.ptr, 12, 0)), ("missing b", (a.ptr, None, o.ptr, n, 0)), ("missing b op 7", (a.ptr, None, o.ptr, n, 7)),
             ("op 8", (a.ptr, b.ptr, o.ptr, n, 8)), ("op -1", (a.ptr, b.ptr, o.ptr, n, -1)), ("misaligned a", (a.ptr + 2, b.ptr, o.ptr, n, 0)),
             ("misaligned b", (a.ptr, b.ptr + 2, o.ptr, n, 0)), ("misaligned out", (a.ptr, b.ptr, o.ptr + 2, n, 0)), ("n 0", (a.ptr, b.ptr, o.ptr, 0, 0))]
    for name, args in calls:
        assert lib.mi_ew_bf16(*args, sp()) == R.MI_EINVAL, name
    torch.cuda.synchronize()
    assert o.complaint("refused", torch.full((1, n + 8), NAN, dtype=F64)) is None


# ------------------------------------------------------------------------------------------------------ mi_sigmoid_f32
def run_sigmoid_fwd(x):
    n = x.size
    xb, yb = in_buf(x, F32), vec(n)
    L.check(L.lib().mi_sigmoid_f32(xb.ptr, None, yb.ptr, None, n, sp()), "sigmoid_f32")
    torch.cuda.synchronize()
    SEEN["sigmoid_f32_kernel<fwd>"] += 1
    s = yb.guards("sigmoid_f32 y")
    return ([s] if s else []), float(R.ulps32(yb.np().reshape(-1), R.sigmoid_ref(x)).max())


def run_sigmoid_bwd(n, seed):
    y, dy, ref = R.sigmoid_bwd_case(n, seed)
    yb, db, ob = Buf(1, n, n, F32, T_(y), SENT), in_buf(dy, F32), vec(n)
    L.check(L.lib().mi_sigmoid_f32(None, db.ptr, yb.ptr, ob.ptr, n, sp()), "sigmoid_f32 bwd")
    torch.cuda.synchronize()
    SEEN["sigmoid_f32_kernel<bwd>"] += 1
    return [s for s in (ob.complaint("sigmoid_f32 dx n %d" % n, ref), yb.complaint("y (an input of the backward)", y)) if s]


@pytest.mark.parametrize("n", R.SIG_NS)
def test_sigmoid_f32_sizes(n):
    """forward within SIGMOID_F32_ULPS fp32 ulps of float64, backward exact on dyadic y and dy; the last n makes the
    grid-stride loop run"""
    args = R.sigmoid_f32_args()
    x = np.resize(args, n)
    bad, d = run_sigmoid_fwd(x)
    if n == R.SIG_NS[-1]:
        bad2, d2 = run_sigmoid_fwd(args)
        bad, d = bad + bad2, max(d, d2)
    print("mi_sigmoid_f32 n %d: worst distance from float64 %.3f fp32 ulps (cap SIGMOID_F32_ULPS = %.3f)" % (n, d, R.SIGMOID_F32_ULPS))
    bad += run_sigmoid_bwd(n, n)
    assert bad == [] and d <= R.SIGMOID_F32_ULPS, (bad, d)


def test_sigmoid_f32_argument_rule():
    """forward (x, y) xor backward (dy, y, dx; the header lets x ride along, ignored): everything else is refused and
    writes nothing"""
    n = 8
    x, dy, y, dx = in_buf(np.zeros(n), F32), in_buf(np.zeros(n), F32), vec(n), vec(n)
    lib = L.lib()
    for name, args in [("x and dy, no dx", (x.ptr, dy.ptr, y.ptr, None)), ("x and dx", (x.ptr, None, y.ptr, dx.ptr)), ("dy without dx", (None, dy.ptr, y.ptr, None)),
                       ("dx without dy", (None, None, y.ptr, dx.ptr)), ("nothing", (None, None, y.ptr, None)), ("no y", (x.ptr, None, None, None))]:
        assert lib.mi_sigmoid_f32(*args, n, sp()) == R.MI_EINVAL, name
    assert lib.mi_sigmoid_f32(x.ptr, None, y.ptr, None, 0, sp()) == R.MI_EINVAL
    torch.cuda.synchronize()
    for b in (y, dx):
        assert b.complaint("refused", torch.full((1, n), NAN, dtype=F64)) is None


# --------------------------------------------------------------------------------------------------------- column sums
COL_ENTRIES = {"wide": "mi_colsum_bf16_wide", "wide_sq": "mi_colsumsq_bf16_wide", "narrow": "mi_colsum_bf16"}


class ColInput:
    """[npix][ld] bf16 with the values in the first C channels and NaN in the pad channels, NaN guards around"""

    def __init__(self, npix, C, ld, seed=0):
        self.npix, self.C, self.ld = npix, C, ld
        self.vals = R.col_values(npix, C, seed, DEV)
        self.flat = torch.full((npix * ld + 2 * GUARD,), NAN, dtype=BF, device=DEV)
        self.flat[GUARD:GUARD + npix * ld].view(npix, ld)[:, :C] = self.vals.to(BF)
        self.ptr = self.flat.data_ptr() + GUARD * 2


def col_launch(kind, xin, out, ws, acc):
    assert "MI_COLSUM_TWO_STAGE" not in os.environ      # else the label below would name a kernel that did not run
    fn = getattr(L.lib(), COL_ENTRIES[kind])
    L.check(fn(xin.ptr, xin.ld, xin.npix, xin.C, out.ptr, acc, ws.ptr, sp()), COL_ENTRIES[kind])
    SEEN[R.col_path(xin.C, kind == "narrow") + ("<sq>" if kind == "wide_sq" else "")] += 1


def col_kinds(C):
    return ("wide", "wide_sq") + (("narrow",) if C <= 128 else ())


def run_colsum(xin, kinds=None):
    C, bad = xin.C, []
    out0 = torch.arange(C, device=DEV, dtype=F64) % 7 - 3
    nws = int(L.lib().mi_colsum_wide_ws_bytes(C)) // 4
    assert nws == 128 * R.col_cp(C)
    for kind in kinds or col_kinds(C):
        sq = kind == "wide_sq"
        R.assert_col_conditions(xin.vals, sq, out0)
        for acc in (0, 1):
            out = Buf(1, C, C, F32, out0 if acc else NAN)
            ws = Buf(1, nws, nws, F32)
            col_launch(kind, xin, out, ws, acc)
            torch.cuda.synchronize()
            s = out.complaint("%s C %d npix %d ld %d accumulate %d" % (kind, C, xin.npix, xin.ld, acc), R.col_ref(xin.vals, sq, out0 if acc else None))
            bad += [s] if s else []
            s = ws.complaint("workspace past mi_colsum_wide_ws_bytes (%s C %d npix %d)" % (kind, C, xin.npix), ws.view())
            bad += [s] if s else []
    return bad


@pytest.mark.parametrize("C", R.COL_CS)
@pytest.mark.parametrize("npix", R.COL_NPIX)
def test_colsum_exact(npix, C):
    """mi_colsum_bf16_wide, mi_colsumsq_bf16_wide and (C <= 128) mi_colsum_bf16 on small integers, no tolerance: ldx = CP and
    ldx > CP (NaN in every pad channel: C = 60 reads its four), accumulate 0 and 1, out and the workspace guarded.  C = 4096
    is the last fused size (64 chunks), C = 4104 takes the two-stage path; npix = 128 * 256 + 1 hits the block cap."""
    bad = []
    for ld in (R.col_cp(C), R.col_cp(C) + 24):
        bad += run_colsum(ColInput(npix, C, ld, seed=C + npix))
    assert bad == [], bad[:6]


def test_colsum_back_to_back_launches_with_different_block_counts():
    """no synchronisation between launches of 2, 128, 1, 9 and 128 blocks on one stream: the chunk counters of the one-launch
    form must have returned to zero each time"""
    C = 2048
    nws = int(L.lib().mi_colsum_wide_ws_bytes(C)) // 4
    ws = Buf(1, nws, nws, F32)
    jobs = []
    for i, npix in enumerate((257, 128 * 256 + 1, 1, 9 * 256, 200 * 256)):
        xin = ColInput(npix, C, C + 8 * (i % 2), seed=i)
        jobs.append((xin, Buf(1, C, C, F32), "wide_sq" if i % 2 else "wide"))
    torch.cuda.synchronize()
    for xin, out, kind in jobs:
        col_launch(kind, xin, out, ws, 0)
    torch.cuda.synchronize()
    bad = [out.complaint("launch of %d pixels" % xin.npix, R.col_ref(xin.vals, kind == "wide_sq")) for xin, out, kind in jobs]
    assert [s for s in bad if s] == [] and ws.complaint("ws", ws.view()) is None, bad


# ------------------------------------------------------------------------------------------------------------ coverage
def test_every_instantiation_is_launched():
    """the counted table: in this process the exact cases launch the plain and the fused forward, PER 1 .. 16 with and
    without dx_drop, the parameter kernel, both dropout forms, the mask entry, each ew op, both directions of the fp32
    sigmoid, and every column-sum path"""
    SEEN.clear()
    bad, worst = [], [0.0]
    bad += run_ln_fwd(R.fwd_exact_case(5, 192, 0, 1), worst)
    bad += run_ln_fused_fwd(R.fused_fwd_case(5, 64, 1, 0.1, 2), worst)
    for E in R.BWD_ES:
        o = R.bwd_exact_case(33, E, E)
        bad += run_ln_bwd(o) + run_ln_bwd(o, 0.5)
    bad += run_dropout(64, 0.5, R.SEED, False) + run_dropout(64, 0.5, R.SEED, True) + run_mha_mask()
    for op in (0, 1, 2, 7):
        a, b = ew_operands(op, 264)
        bad += run_ew(op, a, b)[0]
    for op in (3, 4, 5, 6):
        a, b = ew_operands(op, 264)
        ref, bound = R.ew_bound(op, a, b)
        c, r = run_ew(op, a, b, ref, bound)
        bad += c + ([] if r <= 1 else ["op %d ratio %g" % (op, r)])
    bad += run_sigmoid_fwd(R.sigmoid_f32_args()[:300])[0] + run_sigmoid_bwd(300, 1)
    for Cc in (60, 4104):
        bad += run_colsum(ColInput(257, Cc, R.col_cp(Cc) + 8))
    assert bad == [], bad[:10]
    for k in R.REQUIRED:
        print("%-40s %d" % (k, SEEN.get(k, 0)))
    assert set(SEEN) <= set(R.REQUIRED), set(SEEN) - set(R.REQUIRED)
    missing = [k for k in R.REQUIRED if SEEN.get(k, 0) == 0]
    assert missing == [] and len(R.REQUIRED) == 31, missing
