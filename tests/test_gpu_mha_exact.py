"""GPU (-m gpu): the attention core csrc/mha.hip - forward, delta, dQ, dK/dV and the dropout template of
each - against the plain float64 reference of tests/mha_ref.py with NO tolerance, through the C ABI (mi_mha_fwd_dropout_ld /
mi_mha_bwd_dropout_ld; the tests own scale, H, the row strides and the o_f32 / lse pointers), on every route and block shape.

The method (tests/mha_ref.py): three operand families on which the softmax weights are dyadic - uniform scores over 2^k live
keys, a one-hot gather with +-1 codes at scale 64, uniform scores with dropout at p = 1/2 - so that every value a kernel
rounds to bf16 is representable, every fp32 sum is exact in any order, and O, o_f32, delta, dq, dk, dv of ANY correct
configuration equal the float64 reference rounded once, bit for bit; lse (a log2 and a product round) to mha_ref.LSE_ULPS = 2
fp32 ulps.  The conditions are asserted on the reference of every case before anything is launched.  Every key of a row weighs
the same (uniform) or exactly one does (gather), and with dropout every keep bit of every (b, h, query, key) carries 1/8 of an
output: one dropped, doubled or leaked key, a keep bit from the neighbouring element, an unwritten row changes an output bit.
Padded keys hold V = 100 so that a leak shows.

The dropout cases run with no dropout seed offset installed (the default outside captured graphs): mi_mha_dropout_mask, whose
keep bits the reference applies, does not add the offset.

Hygiene of every launch (Job): o, o_f32, lse, delta, dq, dk, dv live in buffers of sentinel words - guards before and after
the view and, with ldq / ldk > E, the columns outside [0, E) of every dq / dk row - that must survive; the views are pre-filled
with NaN and every element must have been written; the input buffers hold NaN outside their views.

Coverage is counted: the version-2 block shape (mha2_waves: 4 .. 12 waves of 16 rows, from L, B x H and the CU count) is
mirrored in Python (mha_ref.mirror_waves) and the sweep must give every wave count to each of the three version-2 kernels in
both template forms."""
import collections
import types

import pytest
import torch

import mha_ref as R
from yolov7_d2_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -1536.0                 # sentinel (exact in bf16, fp32 and fp64)
GUARD = 64                     # guard elements around every buffer (128 bytes of bf16: the 16-byte alignments hold)
NAN = float("nan")


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def case_table(n):
    return R.exact_cases(n)


class Buf:
    """rows x width elements at row stride ld inside a flat buffer with GUARD elements before and after: `fill` in the view,
    `other` everywhere else"""

    def __init__(self, nrows, width, ld, dtype, fill=NAN, other=SENT, flat=None, col0=0):
        self.nrows, self.width, self.ld, self.col0 = nrows, width, ld, col0
        self.flat = torch.full((nrows * ld + 2 * GUARD,), other, dtype=dtype, device=DEV) if flat is None else flat
        self.idx = (GUARD + col0 + torch.arange(nrows, device=DEV)[:, None] * ld + torch.arange(width, device=DEV)[None, :])
        if fill is not None:
            self.flat[self.idx] = fill if not torch.is_tensor(fill) else fill.reshape(nrows, width).to(DEV, dtype)

    @property
    def ptr(self):
        return self.flat.data_ptr() + (GUARD + self.col0) * self.flat.element_size()

    def view(self):
        return self.flat[self.idx]

    def expected(self, value, base=None):
        """the whole buffer as it must look: `value` in the view, the rest as it was"""
        e = torch.full_like(self.flat, SENT) if base is None else base
        e[self.idx] = value.reshape(self.nrows, self.width).to(e.dtype)
        return e


class Job:
    """one case on the device: operands in NaN-surrounded buffers, outputs in guarded NaN-filled buffers, the launches, and
    the comparison of every WHOLE output buffer with what the float64 reference says it must hold"""

    def __init__(self, c, ops, forward_only=False):
        self.c, self.fwd = c, forward_only
        B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
        E = H * R.D
        self.E = E
        self.ldq, self.ldk = R.strides(c)
        bfl = torch.bfloat16
        v = ops.v_fwd if forward_only else ops.v
        if c.ld == "packed":                      # q and k are the two halves of ONE [T, 2E] buffer, and so are dq and dk
            assert Lq == Lk
            self.q = Buf(Lq * B, E, 2 * E, bfl, ops.q, NAN)
            self.k = Buf(Lk * B, E, 2 * E, bfl, ops.k, NAN, flat=self.q.flat, col0=E)
            self.dq = Buf(Lq * B, E, 2 * E, bfl)
            self.dk = Buf(Lk * B, E, 2 * E, bfl, flat=self.dq.flat, col0=E)
        else:
            self.q = Buf(Lq * B, E, self.ldq, bfl, ops.q, NAN)
            self.k = Buf(Lk * B, E, self.ldk, bfl, ops.k, NAN)
            self.dq = Buf(Lq * B, E, self.ldq, bfl)
            self.dk = Buf(Lk * B, E, self.ldk, bfl)
        self.v = Buf(Lk * B, E, E, bfl, v, NAN)
        self.do = Buf(Lq * B, E, E, bfl, ops.dout, NAN)
        self.mask = None if ops.mask is None else ops.mask.to(DEV, torch.uint8).contiguous()
        self.o = Buf(Lq * B, E, E, bfl)
        self.o32 = Buf(Lq * B, E, E, torch.float32) if c.o32 else None
        self.lse = None if (forward_only and c.lse_null) else Buf(B * H, Lq, Lq, torch.float32)
        self.delta = Buf(B * H, Lq, Lq, torch.float32)
        self.dv = Buf(Lk * B, E, E, bfl)
        self.p = 0.5 if c.family == "dropout" else 0.0
        self.seed = 0x9E3779B97F4A7C15 ^ (c.seed * 2654435761) if self.p else 0
        self.keep = None
        if self.p:
            self.keep = torch.empty(B, H, Lq, Lk, dtype=torch.uint8, device=DEV)
            L.check(L.lib().mi_mha_dropout_mask(self.keep.data_ptr(), B, H, Lq, Lk, self.p, self.seed, L.stream_ptr()), "mask")
        self.waves = (R.mirror_waves(Lq, B * H, ncu()), R.mirror_waves(Lk, B * H, ncu()))

    def launch(self):
        c = self.c
        ptr = lambda b: None if b is None else b.ptr
        mk = None if self.mask is None else self.mask.data_ptr()
        lib = L.lib()
        L.check(lib.mi_mha_fwd_dropout_ld(self.q.ptr, self.ldq, self.k.ptr, self.ldk, self.v.ptr, mk, self.o.ptr, ptr(self.o32),
                                          ptr(self.lse), c.B, c.H, c.Lq, c.Lk, self.E, c.scale, self.p, self.seed, L.stream_ptr()),
                "mi_mha_fwd_dropout_ld")
        if not self.fwd:
            L.check(lib.mi_mha_bwd_dropout_ld(self.q.ptr, self.ldq, self.k.ptr, self.ldk, self.v.ptr, mk, self.o.ptr, ptr(self.o32),
                                              self.lse.ptr, self.do.ptr, self.delta.ptr, self.dq.ptr, self.dk.ptr, self.dv.ptr,
                                              c.B, c.H, c.Lq, c.Lk, self.E, c.scale, self.p, self.seed, L.stream_ptr()),
                    "mi_mha_bwd_dropout_ld")
        torch.cuda.synchronize()

    def result(self):
        """the views as [L][B][E] / [B][H][Lq] tensors (what mha_ref.exact_mismatches compares)"""
        c = self.c
        sh = lambda b, n: None if b is None else b.view().reshape(n, c.B, self.E)
        st = lambda b: None if b is None else b.view().reshape(c.B, c.H, c.Lq)
        return types.SimpleNamespace(O=sh(self.o, c.Lq), O32=sh(self.o32, c.Lq), lse=st(self.lse), delta=st(self.delta),
                                     dq=sh(self.dq, c.Lq), dk=sh(self.dk, c.Lk), dv=sh(self.dv, c.Lk))

    def check(self, ref):
        """names of the output buffers that are not, element for element and sentinel for sentinel, what they must be"""
        bad = []

        def whole(name, buf, value):
            if buf is not None and not torch.equal(buf.flat, buf.expected(value)):
                got, exp = buf.flat, buf.expected(value)
                n = int((~((got == exp) | (got.isnan() & exp.isnan()))).sum())
                bad.append(f"{name}: {n} elements differ ({int(got.isnan().sum())} NaN left)")
        whole("o", self.o, ref.O)
        whole("o_f32", self.o32, ref.O32)
        if self.lse is not None:
            lv = self.lse.view().reshape(ref.lse.shape)
            n = R.lse_mismatch(lv, ref.lse)
            if n:
                bad.append(f"lse: {n} rows beyond {R.LSE_ULPS} ulps")
            if not torch.equal(self.lse.flat, self.lse.expected(lv)):          # the guards
                bad.append("lse: guard touched")
        if not self.fwd:
            whole("delta", self.delta, ref.delta)
            if self.c.ld == "packed":
                exp = self.dk.expected(ref.dk, base=self.dq.expected(ref.dq))
                if not torch.equal(self.dq.flat, exp):
                    bad.append("dq / dk (packed): %d elements differ" % int((self.dq.flat != exp).sum()))
            else:
                whole("dq", self.dq, ref.dq)
                whole("dk", self.dk, ref.dk)
            whole("dv", self.dv, ref.dv)
        else:                                       # a forward launch writes nothing else
            for name, buf in (("delta", self.delta), ("dq", self.dq), ("dk", self.dk), ("dv", self.dv)):
                if not bool(buf.view().isnan().all()):
                    bad.append(name + ": written by a forward launch")
        return bad


def run_case(c, seen=None, want_result=False):
    """both launches of a case - the forward-only one (v_fwd; lse = NULL if the case says so) and forward + backward - each
    against the float64 reference computed on the device, the conditions of the method asserted first.  Returns the list of
    complaints; `seen` collects (kernel, dropout form) -> wave counts of the version-2 launcher's choice."""
    ops = R.make_operands(c)
    bad = []
    for fwd in (True, False):
        job = Job(c, ops, forward_only=fwd)
        ref = R.reference_of(c, ops, job.keep, forward_only=fwd, device=DEV)
        R.assert_exact_conditions(c, ops, ref, forward_only=fwd)
        job.launch()
        bad += [f"{c.name} ({'forward' if fwd else 'forward + backward'}): {b}" for b in job.check(ref)]
        if seen is not None:
            drop = job.p > 0
            seen[("fwd2", drop)].add(job.waves[0])
            if not fwd:
                seen[("dq2", drop)].add(job.waves[0])
                seen[("dkv2", drop)].add(job.waves[1])
    return bad


def test_wave_mirror_by_the_grid_arithmetic():
    """mha_ref.mirror_waves restates mha2_waves; what can be held to the launcher without reading its mind is its grid
    arithmetic: 4 .. 12 waves (a block of at most 768 threads, the kernels' launch bound), blocks x waves cover every 16-row
    group with no empty block, the grid is one round of blocks on the device unless a clamp applies, and never more waves
    than groups above 4"""
    n = ncu()
    for BH in (1, 3, 16, 64, 160, n + 32):
        for Lx in list(range(1, 70)) + [127, 128, 129, 257, 300, 763, 1050]:
            w = R.mirror_waves(Lx, BH, n)
            gq = -(-Lx // 16)
            blocks = -(-gq // w)
            assert 4 <= w <= 12 and w * 64 <= 768
            assert blocks * w >= gq > (blocks - 1) * w
            assert w <= max(gq, 4)
            raw = -(-gq * BH // n)
            if 4 <= raw <= 12 and raw <= gq:
                assert w == raw and blocks * BH <= n + BH       # one round of blocks (rounded up to whole blocks per head)


@pytest.mark.parametrize("family", ["uniform", "gather", "dropout"])
def test_exact_on_every_block_shape(family):
    """nine cases at B x H = 5 x 32 whose Lq and Lk (none a multiple of 16, ragged last blocks, three key chunks, scattered /
    leading / whole-chunk masks, a fully masked image in every second one, q or k zero in turn, all four stride forms, with
    and without o_f32) give the forward and dQ kernels (by Lq) and dK/dV (by Lk) every wave count 4 .. 12 - counted"""
    sweep, _ = case_table(ncu())
    seen = collections.defaultdict(set)
    bad = []
    for c in sweep[family]:
        bad += run_case(c, seen)
    assert bad == [], bad[:20]
    drop = family == "dropout"
    for kern in ("fwd2", "dq2", "dkv2"):
        assert seen[(kern, drop)] == set(range(4, 13)), (kern, drop, sorted(seen[(kern, drop)]))


@pytest.mark.parametrize("family", ["uniform", "gather", "dropout"])
def test_exact_on_small_shapes_and_parameter_variants(family):
    """L = 1; Lk < 32; Lk just above 128 and 256; the nwv > gq clamp (B x H above the CU count); H in {1, 3, 8, 32}; B in
    {1, 2, 5, ...}; no mask; a fully masked image; the packed q / k buffer and the wider strides; delta from the bf16 O
    (o_f32 = NULL); lse = NULL in a forward-only launch"""
    _, extras = case_table(ncu())
    bad = []
    for c in extras:
        if c.family == family:
            bad += run_case(c)
    assert bad == [], bad[:20]


@pytest.mark.parametrize("family", ["uniform", "gather", "dropout"])
def test_mutants_fail_exactly_where_the_norm_passes(family):
    """standing mutation evidence, on the reference side only (mha_ref.mutants / check_mutants): a reference with one key
    dropped from one query row, the mask boundary moved by one key for one wave, one row's keep bits shifted by one element,
    one head's dv row of the ragged last group zeroed, or one lse off by 2^-6 is REJECTED by the exact comparison with the
    device's (correct) result, and ACCEPTED by the Frobenius criterion of tests/test_gpu_detr.py at the same shape"""
    c = [m for m in R.mutation_cases() if m.name == "mut-" + family][0]
    mutants_on_device(c)


def mutants_on_device(c):
    ops = R.make_operands(c)
    keep = {}

    def result_of(fwd):
        job = Job(c, ops, forward_only=fwd)
        keep[0] = job.keep
        job.launch()
        return job.result()
    if c.family == "dropout":                       # the keep bits are the device's own: one export serves reference and mutants
        keep[0] = Job(c, ops).keep
    R.check_mutants(c, ops, None if keep.get(0) is None else keep[0].cpu(), result_of, device=DEV)


def test_refusals_leave_the_outputs_untouched():
    """mha_check and the stride / dropout requirements: each refusal returns an error with its documented message and
    launches nothing (the NaN-filled outputs stay NaN).  Only refusals whose launch would stay inside the buffers were the
    check missing: E != 32 H with buffers sized for the larger reading, a row stride that is no multiple of 8 or below E in
    buffers of the wider stride, drop_p = 1"""
    c = R.Case("refusal", "uniform", 2, 3, 40, 48, None, "q", 0.25, True, "wide", False, 5)
    ops = R.make_operands(c)
    big = c._replace(H=4)                           # buffers for E = 128
    opsb = R.make_operands(big)
    lib = L.lib()

    def attempt(job, what, msg, **kw):
        a = dict(ldq=job.ldq, ldk=job.ldk, H=c.H, E=job.E, p=0.0)
        a.update(kw)
        mk = None
        rcs = [lib.mi_mha_fwd_dropout_ld(job.q.ptr, a["ldq"], job.k.ptr, a["ldk"], job.v.ptr, mk, job.o.ptr, job.o32.ptr, job.lse.ptr,
                                         c.B, a["H"], c.Lq, c.Lk, a["E"], c.scale, a["p"], 1, L.stream_ptr())]
        err = [lib.mi_last_error().decode()]
        rcs.append(lib.mi_mha_bwd_dropout_ld(job.q.ptr, a["ldq"], job.k.ptr, a["ldk"], job.v.ptr, mk, job.o.ptr, job.o32.ptr,
                                             job.lse.ptr, job.do.ptr, job.delta.ptr, job.dq.ptr, job.dk.ptr, job.dv.ptr,
                                             c.B, a["H"], c.Lq, c.Lk, a["E"], c.scale, a["p"], 1, L.stream_ptr()))
        err.append(lib.mi_last_error().decode())
        torch.cuda.synchronize()
        assert all(rc < 0 for rc in rcs), (what, rcs)
        assert all(msg in e for e in err), (what, err)
        for b in (job.o, job.o32, job.lse, job.delta, job.dq, job.dk, job.dv):
            assert bool(b.view().isnan().all()) and bool((b.flat[:GUARD] == SENT).all()) and bool((b.flat[-GUARD:] == SENT).all()), what

    jb = Job(big, opsb)                             # E = 128 buffers, called with H = 3: E != 32 H
    attempt(jb, "E != 32 H", "mha: E 128 must be H*32 (H 3)", H=3, E=128)
    j = Job(c, ops)                                 # ldq = E + 8, ldk = E + 24
    attempt(j, "ldq % 8", "row strides ldq 100 / ldk 120", ldq=c.H * R.D + 4)
    attempt(j, "ldk < E", "row strides ldq 104 / ldk 88", ldk=c.H * R.D - 8)
    attempt(j, "drop_p = 1", "mha: dropout p 1.0", p=1.0)
    attempt(j, "drop_p < 0", "mha: dropout p -0.5", p=-0.5)


@pytest.mark.parametrize("nc", R.numerics_cases(), ids=lambda c: c.name)
def test_numerics_within_derived_bounds(nc):
    """the arithmetic the exact families cannot reach - the scale fold, the exp2 / lse conversions, the lazy maximum, delta -
    on random bf16 data at scale 1/sqrt(32): every element of O, o_f32, lse, delta, dq, dk, dv within the first-order worst-case
    bound mha_ref.error_bounds derives from the float64 reference's own intermediates (constants 2^-8 and 2^-24, nothing
    fitted; the derivation is that function's docstring), with the hygiene of every launch.  The ratios and the median of
    bound / |value| are printed (the latter is judged in tests/test_mha_ref.py::test_bounds_are_not_vacuous)."""
    ops = R.make_numerics_operands(nc)
    c = R.Case(nc.name, "numerics", nc.B, nc.H, nc.Lq, nc.Lk, None, "", R.NSCALE, nc.o32, "wide" if nc.seed % 2 else "E", False, nc.seed)
    d = lambda t: None if t is None else t.to(DEV)
    ref = R.attention_reference(d(ops.q), d(ops.k), d(ops.v), d(ops.dout), d(ops.mask), R.NSCALE, nc.H)
    bounds = R.error_bounds(ref, d(ops.q), d(ops.k), d(ops.v), d(ops.dout), R.NSCALE, nc.H, nc.o32)
    job = Job(c, ops)
    job.launch()
    for name, b in (("o", job.o), ("o_f32", job.o32), ("lse", job.lse), ("delta", job.delta), ("dq", job.dq), ("dk", job.dk), ("dv", job.dv)):
        if b is not None:
            assert torch.equal(b.flat, b.expected(b.view())) and not bool(b.view().isnan().any()), (name, "sentinel touched or NaN left")
    rat = R.bound_ratios(job.result(), ref, bounds)
    print(nc.name, {k: "%.2f (median bound/|value| %.1e)" % v for k, v in rat.items()})
    assert all(v[0] <= 1.0 for v in rat.values()), rat
