"""GPU (-m gpu): the BatchNorm(train) + SiLU (+ residual) family csrc/bn_act.hip - the three streaming kernels, the one-launch
backward that keeps registers and LDS across a grid-wide barrier, the
grouped forms of all four and mi_bn_eval_affine - against the plain float64 reference of tests/bn_ref.py with NO tolerance,
through the C ABI by ctypes, on every pass and launch form.

The method (tests/bn_ref.py): operand families on which every fp32 / fp64 operation of the kernels is exact - dyadic
statistics with invstd in {1, 2, 4} for the forward, small integers on a 2^-(k+2) grid for the backward, and SiLU saturated to
sigmoid = 1 or 0 for the ACT = 1 instantiations - so the device must equal the float64 reference, rounded once to bf16 where a
kernel stores bf16, bit for bit, whatever the fma contraction, summation order, block count, slot count or atomic arrival
order.  The conditions are asserted on the reference of every case before anything is launched; the premise of the
saturated family is checked on the device first (test_premise_*).

Hygiene of every launch: every output lives in a buffer of sentinel words - guards before and after the view and, with a
leading dimension above C, the pad channels [C, ld) of every row - that must survive; outputs are pre-filled with NaN before
EVERY launch and every element must have been written; input buffers hold NaN outside their views; the accumulator slots
>= nslots and the pad channels [C, CA) of every slot hold NaN (the forward and apply must not read them, reduce and fused
must not write them); dres starts as NaN when it is overwritten and as integers when it accumulates; the leading dimensions
are pairwise different in at least one case per entry point.

What the exact families cannot reach - the sigmoid itself, real statistics - is held to derived bounds: an exhaustive sweep
of SiLU and SiLU' over every finite bf16 argument, and Gaussian data with elementwise bounds (bn_ref.numerics_*), each bound
first checked against an fp32 emulation on the host.  The launched instantiations are counted and the table must be
complete."""
import collections
import ctypes as C
import math
import types

import pytest
import torch

import bn_ref as R
from yolov7_d2_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -1536.0                 # sentinel (exact in bf16, fp32, fp64 and the integer types)
GUARD = 64                     # guard elements around every buffer (>= 64 bytes: every alignment the ABI asks for holds)
NAN = float("nan")
F64 = torch.float64
BF, F32 = torch.bfloat16, torch.float32
SEEN = collections.Counter()   # instantiation -> launches by an exact family in this process


def sp():
    return L.stream_ptr()


class Buf:
    """rows x width elements at row stride ld inside a flat buffer with GUARD elements before and after: `fill` in the view,
    `other` everywhere else (SENT for outputs, NaN for inputs)"""

    def __init__(self, nrows, width, ld, dtype, fill=NAN, other=SENT):
        self.nrows, self.width, self.ld, self.other = nrows, width, ld, other
        self.flat = torch.full(((nrows - 1) * ld + width + (ld - width) + 2 * GUARD,), other, dtype=dtype, device=DEV)
        self.idx = GUARD + torch.arange(nrows, device=DEV)[:, None] * ld + torch.arange(width, device=DEV)[None, :]
        self.set(fill)

    def set(self, fill):
        if torch.is_tensor(fill):
            fill = fill.reshape(self.nrows, self.width).to(DEV).to(self.flat.dtype)
        self.flat[self.idx] = fill

    @property
    def ptr(self):
        return self.flat.data_ptr() + GUARD * self.flat.element_size()

    def view(self):
        return self.flat[self.idx].to(F64)

    def from_view(self):
        """the buffer from the view's first element on, as a kernel indexing from ptr sees it"""
        return self.flat[GUARD:].to(F64)

    def complaint(self, name, value):
        """None if the WHOLE buffer is `value` (float64 tensor of the view's shape, NaN = NaN) in the view and untouched
        elsewhere"""
        exp = torch.full(self.flat.shape, self.other, dtype=F64, device=DEV)
        exp[self.idx] = value.reshape(self.nrows, self.width).to(DEV).to(F64)
        got = self.flat.to(F64)
        bad = ~((got == exp) | (got.isnan() & exp.isnan()))
        if not bool(bad.any()):
            return None
        inside = torch.zeros_like(bad)
        inside[self.idx] = True
        i = int(torch.nonzero(bad)[0])
        return "%s: %d elements differ (%d outside the view, %d NaN in the view), first at flat %d: got %r, expected %r" % (
            name, int(bad.sum()), int((bad & ~inside).sum()), int(self.flat[self.idx].to(F64).isnan().sum()), i - GUARD,
            float(got[i]), float(exp[i]))


def vec(value, C, dtype=F32, other=NAN):
    """a per-channel input vector (NaN around it) or, with value = NAN, a per-channel output (sentinels around it)"""
    return Buf(1, C, C, dtype, value, other)


def ptr(b):
    return None if b is None else b.ptr


def dev(o):
    """the tensors of an operand namespace moved to the device"""
    for k, v in vars(o).items():
        if torch.is_tensor(v):
            setattr(o, k, v.to(DEV))
    return o


# ------------------------------------------------------------------------------------------------------------- forward
class FwdJob:
    """one forward case on the device"""

    def __init__(self, c, o):
        self.c, self.o = c, o
        Cc, n = c.C, c.npix
        self.ldy, self.ldres, self.lda = R.fwd_lds(c)
        self.y = Buf(n, Cc, self.ldy, BF, o.y, NAN)
        self.res = Buf(n, Cc, self.ldres, BF, o.res, NAN) if o.res is not None else None
        self.a = Buf(n, Cc, self.lda, BF)
        self.acc = self.gamma = self.beta = self.mean = self.invstd = self.rmean = self.rvar = self.nbt = None
        if c.train:
            CA = R.acc_c(Cc)
            self.acc = Buf(R.SLOTS, CA * 2, CA * 2, F64, o.acc.reshape(R.SLOTS, CA * 2), NAN)
            self.gamma, self.beta = vec(o.gamma, Cc), vec(o.beta, Cc)
            self.scale, self.shift, self.mean, self.invstd = (vec(NAN, Cc, other=SENT) for _ in range(4))
            if c.running != "none":
                self.rmean, self.rvar = vec(o.rmean0, Cc, other=SENT), vec(o.rvar0, Cc, other=SENT)
                if c.running == "both":
                    self.nbt = Buf(1, 1, 1, torch.int64, o.nbt0, int(SENT))
        else:                                           # eval mode: scale / shift are inputs, everything else NULL
            self.scale, self.shift = vec(o.scale, Cc, other=SENT), vec(o.shift, Cc, other=SENT)

    def outputs(self):
        return [b for b in ((self.a, self.scale, self.shift, self.mean, self.invstd) if self.c.train else (self.a,)) if b is not None]

    def refill(self):
        for b in self.outputs():
            b.set(NAN)

    def args(self):
        c = self.c
        return (self.y.ptr, self.ldy, ptr(self.acc), c.nslots, self.o.count, ptr(self.gamma), ptr(self.beta), R.EPS, R.MOMENTUM,
                ptr(self.rmean), ptr(self.rvar), ptr(self.nbt), self.scale.ptr, self.shift.ptr, ptr(self.mean), ptr(self.invstd),
                ptr(self.res), self.ldres if self.res is not None else 0, self.a.ptr, self.lda, c.npix, c.C, 1 if c.act else 0, sp())

    def job(self, j):
        """fill a mi_bn_job for the grouped form"""
        c = self.c
        j.y, j.res, j.a, j.acc = self.y.ptr, ptr(self.res), self.a.ptr, ptr(self.acc)
        j.gamma, j.beta, j.rmean, j.rvar, j.nbt = ptr(self.gamma), ptr(self.beta), ptr(self.rmean), ptr(self.rvar), ptr(self.nbt)
        j.scale, j.shift, j.mean, j.invstd = self.scale.ptr, self.shift.ptr, ptr(self.mean), ptr(self.invstd)
        j.npix, j.count, j.ldy, j.ldres, j.lda = c.npix, self.o.count, self.ldy, self.ldres if self.res is not None else 0, self.lda
        j.C, j.nslots, j.act, j.eps, j.momentum = c.C, c.nslots, 1 if c.act else 0, R.EPS, R.MOMENTUM

    def launch(self):
        L.check(L.lib().mi_bn_act_fwd(*self.args()), "mi_bn_act_fwd")
        torch.cuda.synchronize()
        SEEN[R.kernel_name("bn_act_fwd", self.c.act)] += 1

    def check(self, r, i=0):
        """complaints after launch number i (0-based) against the reference r of fwd_reference"""
        c, bad = self.c, []
        add = lambda s: bad.append(s) if s else None
        add(self.a.complaint("a", r.a))
        add(self.scale.complaint("scale", r.scale))
        add(self.shift.complaint("shift", r.shift))
        if c.train:
            add(self.mean.complaint("mean", r.mean))
            add(self.invstd.complaint("invstd", r.invstd))
            add(self.acc.complaint("acc (an input)", self.o.acc))
            if self.rmean is not None:
                add(self.rmean.complaint("running_mean after launch %d" % (i + 1), r.rmean[i]))
                rv = self.rvar.view().reshape(-1)
                if not bool(((rv - r.rvar[i]).abs() <= r.rvar_tol[i]).all()):
                    bad.append("running_var after launch %d: off by %.3g (bound %.3g)" % (
                        i + 1, float((rv - r.rvar[i]).abs().max()), float(r.rvar_tol[i].max())))
                add(self.rvar.complaint("running_var guards", rv))
            if self.nbt is not None:
                add(self.nbt.complaint("num_batches_tracked", torch.tensor([float(r.nbt[i])])))
        return ["%s: %s" % (c.name, b) for b in bad]


def run_fwd_case(c, launches=3):
    o = R.make_fwd_operands(c)
    r0 = R.fwd_reference(c, o, launches)
    R.assert_fwd_conditions(c, o, r0)
    o = dev(o)
    r = R.fwd_reference(c, o, launches)                 # the same reference, on the device
    job = FwdJob(c, o)
    bad = []
    for i in range(launches):
        job.refill()
        job.launch()
        bad += job.check(r, i)
    return bad


# ------------------------------------------------------------------------------------------------------------ backward
class BwdJob:
    """one backward case on the device: reduce + apply, or the one-launch form"""

    def __init__(self, c, o):
        self.c, self.o = c, o
        Cc, n = c.C, c.npix
        self.ldda, self.ldy, self.lddy, self.lddres = R.bwd_lds(c)
        self.da, self.y = Buf(n, Cc, self.ldda, BF, o.da, NAN), Buf(n, Cc, self.ldy, BF, o.y, NAN)
        self.scale, self.shift, self.mean, self.invstd, self.gamma = (vec(t, Cc) for t in (o.scale, o.shift, o.mean, o.invstd, o.gamma))
        self.CA, self.n = R.acc_c(Cc), R.norm_slots(c.nslots)
        self.acc0 = torch.full((R.SLOTS, self.CA, 2), NAN, dtype=F64)
        self.acc0[:self.n, :Cc] = 0.0
        self.dacc = Buf(R.SLOTS, self.CA * 2, self.CA * 2, F64, self.acc0.reshape(R.SLOTS, -1), SENT)
        self.dy = Buf(n, Cc, self.lddy, BF)
        self.dres = Buf(n, Cc, self.lddres, BF) if c.dres else None
        self.dgamma, self.dbeta = (None, None) if c.nodg else (vec(NAN, Cc, other=SENT), vec(NAN, Cc, other=SENT))
        self.bar = Buf(1, R.BAR_WORDS, R.BAR_WORDS, torch.int32, 0, int(SENT))
        self.nbs = []

    def refill(self):
        self.dacc.set(self.acc0.reshape(R.SLOTS, -1))
        self.dy.set(NAN)
        if self.dres is not None:
            self.dres.set(self.o.dres0 if self.c.dres == 2 else NAN)
        for b in (self.dgamma, self.dbeta):
            if b is not None:
                b.set(NAN)

    def head(self):
        return (self.da.ptr, self.ldda, self.y.ptr, self.ldy, self.scale.ptr, self.shift.ptr, self.mean.ptr, self.invstd.ptr)

    def tail(self):
        c = self.c
        return (ptr(self.dgamma), ptr(self.dbeta), self.dy.ptr, self.lddy, ptr(self.dres), self.lddres if self.dres is not None else 0,
                int(c.dres == 2), c.npix, c.C, 1 if c.act else 0)

    def job(self, j):
        c = self.c
        j.da, j.y, j.dy, j.dres, j.acc = self.da.ptr, self.y.ptr, self.dy.ptr, ptr(self.dres), self.dacc.ptr
        j.scale, j.shift, j.mean, j.invstd, j.gamma = self.scale.ptr, self.shift.ptr, self.mean.ptr, self.invstd.ptr, self.gamma.ptr
        j.dgamma, j.dbeta, j.bar = ptr(self.dgamma), ptr(self.dbeta), self.bar.ptr
        j.npix, j.count, j.ldda, j.ldy, j.lddy = c.npix, self.o.count, self.ldda, self.ldy, self.lddy
        j.lddres, j.dres_accum = self.lddres if self.dres is not None else 0, int(c.dres == 2)
        j.C, j.nslots, j.nblk, j.act = c.C, c.nslots, c.nblk, 1 if c.act else 0

    def two_pass(self):
        c, lib = self.c, L.lib()
        L.check(lib.mi_bn_act_bwd_reduce(*self.head(), self.dacc.ptr, c.nslots, c.nblk, c.npix, c.C, 1 if c.act else 0, sp()), "reduce")
        torch.cuda.synchronize()
        SEEN[R.kernel_name("bn_bwd_reduce", c.act)] += 1
        mid = self.check_sums("reduce", folded=False)
        for b in (self.dy, self.dres if c.dres == 1 else None, self.dgamma, self.dbeta):      # reduce writes nothing else
            if b is not None and not bool(b.view().isnan().all()):
                mid.append("%s: written by the reduce launch" % c.name)
        L.check(lib.mi_bn_act_bwd_apply(*self.head(), self.gamma.ptr, self.dacc.ptr, c.nslots, self.o.count, *self.tail(), sp()), "apply")
        torch.cuda.synchronize()
        SEEN[R.kernel_name("bn_bwd_apply", c.act)] += 1
        return mid

    def fused(self):
        c = self.c
        L.check(L.lib().mi_bn_act_bwd_fused(*self.head(), self.gamma.ptr, self.dacc.ptr, c.nslots, self.o.count, *self.tail(),
                                            self.bar.ptr, sp()), "fused")
        torch.cuda.synchronize()
        SEEN[R.kernel_name("bn_bwd_fused", c.act)] += 1

    def check_sums(self, what, folded):
        """the accumulators: NaN pattern and guards intact, and the live slots hold the channel sums - exactly (every partial
        sum is exact): their sum over the slots, or slot 0 alone once the last block of a fused launch has folded them"""
        r, Cc = self.r, self.c.C
        got = self.dacc.view().reshape(R.SLOTS, self.CA, 2)
        bad = []
        pattern = got.isnan() == self.acc0.to(DEV).isnan()
        if not bool(pattern.all()):
            bad.append("%s: %s wrote outside its slots / channels (%d accumulator words)" % (self.c.name, what, int((~pattern).sum())))
        if self.dacc.complaint("g", self.dacc.view()) is not None:
            bad.append("%s: %s touched the accumulator guards" % (self.c.name, what))
        tot = got[0, :Cc] if folded else got[:self.n, :Cc].sum(0)
        if not (torch.equal(tot[:, 0], r.s1) and torch.equal(tot[:, 1], r.s2)):
            bad.append("%s: %s: channel sums differ in %d channels" % (
                self.c.name, what, int(((tot[:, 0] != r.s1) | (tot[:, 1] != r.s2)).sum())))
        return bad

    def check(self, what):
        c, r, bad = self.c, self.r, []
        add = lambda s: bad.append(s) if s else None
        add(self.dy.complaint("dy", r.dy))
        if self.dres is not None:
            add(self.dres.complaint("dres", r.dres))
        if self.dgamma is not None:
            add(self.dgamma.complaint("dgamma", r.dgamma))
            add(self.dbeta.complaint("dbeta", r.dbeta))
        return ["%s (%s): %s" % (c.name, what, b) for b in bad]

    def check_barrier(self, nbs):
        exp = R.barrier_expected(nbs).to(F64)
        s = self.bar.complaint("barrier words after %d launches of %s blocks" % (len(nbs), nbs[-1]), exp)
        return ["%s: %s" % (self.c.name, s)] if s else []


def effective_capacity(cap):
    """install the resident-block budget (0 = the device's) and return the one in effect; never more than the device's"""
    lib = L.lib()
    hw = lib.mi_bn_fused_set_capacity(0)
    assert cap <= hw, "the case asks for more resident blocks than the device has"
    return lib.mi_bn_fused_set_capacity(cap)


def make_bwd_job(c):
    o = R.make_bwd_operands(c)
    R.assert_bwd_conditions(c, o, R.bwd_reference(c, o))
    o = dev(o)
    job = BwdJob(c, o)
    job.r = R.bwd_reference(c, o)
    return job


def run_two_pass_case(c):
    job = make_bwd_job(c)
    job.refill()
    bad = job.two_pass()
    return bad + job.check("reduce + apply")


def run_fused_case(c, stats=None):
    """three launches on one barrier record, everything refilled and checked every time"""
    job = make_bwd_job(c)
    bad = []
    try:
        cap = effective_capacity(c.cap)
        nb = R.fused_blocks(c.npix, c.C, cap)
        assert nb <= cap
        if stats is not None:
            stats["nb"].add(nb)
            stats["items"] |= R.nmine_set(c.npix, c.C, nb)
        for i in range(3):
            job.refill()
            job.fused()
            bad += job.check("fused, launch %d, %d blocks" % (i + 1, nb))
            bad += job.check_sums("fused", folded=True)
            bad += job.check_barrier([nb] * (i + 1))
    finally:
        L.lib().mi_bn_fused_set_capacity(0)
    return bad


# --------------------------------------------------------------------------------------------------------------- groups
def plan_group(kind, jobs, act):
    """mi_bn_group_plan into a host table, the table copied into a guarded device buffer; -> (meta, table Buf, starts)"""
    lib = L.lib()
    n = len(jobs)
    arr = (L.mi_bn_job * n)()
    for j, job in zip(arr, jobs):
        job.job(j)
    meta = L.mi_bn_group()
    L.check(lib.mi_bn_group_plan(kind, arr, n, None, 0, C.byref(meta)), "plan (size)")
    host = (C.c_uint8 * meta.table_bytes)()
    L.check(lib.mi_bn_group_plan(kind, arr, n, host, meta.table_bytes, C.byref(meta)), "plan")
    assert meta.kind == kind and meta.njobs == n and meta.act == (1 if act else 0)
    tab = Buf(1, meta.table_bytes, meta.table_bytes, torch.uint8, torch.frombuffer(host, dtype=torch.uint8).clone(), 0xA5)
    starts = list((C.c_int32 * (n + 1)).from_buffer(host, meta.starts_off))
    assert starts[0] == 0 and starts[-1] == meta.nblocks and all(b > a for a, b in zip(starts, starts[1:])), starts
    return meta, tab, starts


def run_group(meta, tab, stem, act):
    L.check(L.lib().mi_bn_group_run(C.byref(meta), tab.ptr, sp()), "mi_bn_group_run")
    torch.cuda.synchronize()
    SEEN[R.kernel_name(stem, act, group=True)] += 1
    assert tab.complaint("table", tab.view()) is None


def run_group_case(g):
    bad = []
    if g.kind == 0:
        jobs, refs = [], []
        for c in g.jobs:
            o = R.make_fwd_operands(c)
            R.assert_fwd_conditions(c, o, R.fwd_reference(c, o, 1))
            o = dev(o)
            jobs.append(FwdJob(c, o))
            refs.append(R.fwd_reference(c, o, 1))
        meta, tab, starts = plan_group(0, jobs, g.act)
        assert [b - a for a, b in zip(starts, starts[1:])] == [R.ew_blocks(c.npix * c.C // 8) for c in g.jobs]
        run_group(meta, tab, "bn_act_fwd", g.act)
        for job, r in zip(jobs, refs):
            bad += job.check(r, 0)
        return bad
    jobs = [make_bwd_job(c) for c in g.jobs]
    for job in jobs:
        job.refill()
    if g.kind == 12:
        meta, tab, starts = plan_group(1, jobs, g.act)
        assert [b - a for a, b in zip(starts, starts[1:])] == [c.nblk for c in g.jobs]
        run_group(meta, tab, "bn_bwd_reduce", g.act)
        for job in jobs:
            bad += job.check_sums("grouped reduce", folded=False)
        meta, tab, starts = plan_group(2, jobs, g.act)
        run_group(meta, tab, "bn_bwd_apply", g.act)
        for job in jobs:
            bad += job.check("grouped apply")
        return bad
    # kind 3: a small capacity, so that the jobs SHARE it (want > cap): a third of what they would take, at least n + 1
    try:
        hw = effective_capacity(0)
        want = sum(R.fused_blocks(c.npix, c.C, hw) for c in g.jobs)
        cap = effective_capacity(max(g.n + 1, want // 3))
        want = sum(R.fused_blocks(c.npix, c.C, cap) for c in g.jobs)
        assert want > cap or g.n == 1, (want, cap)
        meta, tab, starts = plan_group(3, jobs, g.act)
        nbs = [b - a for a, b in zip(starts, starts[1:])]
        assert meta.nblocks <= cap and all(nb >= 1 for nb in nbs), (nbs, cap)
        for i in range(2):
            for job in jobs:
                job.refill()
            run_group(meta, tab, "bn_bwd_fused", g.act)
            for job, nb in zip(jobs, nbs):
                bad += job.check("grouped fused, launch %d, %d blocks" % (i + 1, nb))
                bad += job.check_sums("grouped fused", folded=True)
                bad += job.check_barrier([nb] * (i + 1))
    finally:
        L.lib().mi_bn_fused_set_capacity(0)
    return bad


# ---------------------------------------------------------------------------------------------------------------- tests
def eval_forward(y_bf16, scale, shift, act):
    """the forward kernel in eval mode (NULL statistics pointers) over the values of y_bf16, laid out as pixels of 8 channels
    that share one scale and shift: -> a, as float64"""
    n = y_bf16.numel() // 8
    y = Buf(n, 8, 8, BF, y_bf16.reshape(n, 8), NAN)
    a = Buf(n, 8, 8, BF)
    sc, sh = vec(torch.full((8,), scale, dtype=F64), 8), vec(torch.full((8,), shift, dtype=F64), 8)
    L.check(L.lib().mi_bn_act_fwd(y.ptr, 8, None, 0, 0, None, None, R.EPS, R.MOMENTUM, None, None, None, sc.ptr, sh.ptr, None, None,
                                  None, 0, a.ptr, 8, n, 8, act, sp()), "mi_bn_act_fwd (eval)")
    torch.cuda.synchronize()
    assert a.complaint("guards", a.view()) is None
    return a.view().reshape(-1)


def test_reference_rounding_is_the_same_on_the_device():
    """the float64 references are computed on the device: bn_ref.bf16_rne there must be what tests/test_bn_ref.py pins on the
    host (powers of two built from bits, not from a library function), on random values, every midpoint and the subnormals"""
    g = torch.Generator().manual_seed(9)
    pos = R.all_finite_bf16().to(F64)
    pos = pos[pos > 0].sort().values
    x = torch.cat([torch.randn(100000, generator=g, dtype=F64) * torch.exp2(torch.randint(-140, 127, (100000,), generator=g).to(F64)),
                   (pos[:-1] + pos[1:]) / 2, -pos, torch.randint(-4096, 4096, (100000,), generator=g).to(F64) / 32])
    assert torch.equal(R.bf16_rne(x.to(DEV)).cpu(), R.bf16_rne(x))
    assert torch.equal(R.bf16_half_ulp(x.to(DEV)).cpu(), R.bf16_half_ulp(x))


def test_premise_saturated_sigmoid_is_exact_on_the_device():
    """the premise of the saturated family, through the forward kernel in eval mode (scale 1, shift 0, SiLU): for every bf16
    z >= 32 the result is z itself (sigmoidf_ = rcp(1) = 1), for every finite bf16 z <= -100 it is zero (exp overflows to
    +inf, rcp(inf) = 0).  If this does not hold the family is void - it is the reference that must not bend."""
    allv = R.all_finite_bf16()
    z = allv[(allv.float() >= 32) | (allv.float() <= -100)]
    z = torch.cat([z, torch.zeros((-z.numel()) % 8, dtype=BF) + 64])
    a = eval_forward(z, 1.0, 0.0, 1).cpu()
    zf = z.to(F64)
    exp = torch.where(zf >= 32, zf, torch.zeros_like(zf))
    wrong = int((a != exp).sum())
    assert wrong == 0, "%d of %d saturated arguments are not exact on the device" % (wrong, z.numel())


@pytest.mark.parametrize("c", R.fwd_cases(), ids=lambda c: c.name)
def test_forward_exact(c):
    """mi_bn_act_fwd, three successive launches: train and eval mode, act 0 / saturated SiLU, with and without res, C8 = 1,
    3, 5, 12, 33, 160, 256, npix 1 / 5 / 777 / 4096, nslots 1 / 3 / 16 and 0 / 17 (= 16), NULL running pointers or NULL nbt,
    NULL gamma .. invstd in eval mode: a, scale, shift, mean, invstd, the running mean and nbt exactly; the running variance
    exactly after the first launch and within bn_ref.rvar_tolerance after the second and third"""
    bad = run_fwd_case(c)
    assert bad == [], bad[:10]


def test_forward_exact_beyond_the_block_cap():
    """4100 x 2048: 1 049 600 items on the 1024-block cap - the 4-deep loop makes a second, partial trip"""
    bad = run_fwd_case(R.fwd_cap_case(), launches=1)
    assert bad == [], bad[:10]


def one_job_group(kind, c):
    return types.SimpleNamespace(kind=kind, n=1, act=c.act, jobs=[c])


def test_forward_exact_beyond_the_block_cap_grouped():
    """the same case as a one-job group of kind 0: the grouped body makes the second trip too"""
    bad = run_group_case(one_job_group(0, R.fwd_cap_case()))
    assert bad == [], bad[:10]


@pytest.mark.parametrize("c", R.bwd_cap_cases(), ids=lambda c: c.name)
def test_backward_two_pass_exact_beyond_the_block_cap(c):
    """2100 x 2048: 537 600 items on the 1024-block cap - a thread of the 2-deep apply loop takes a third item (a second,
    partial trip); the 1024 reduce blocks (one pixel lane each) take 2 or 3 pixels"""
    bad = run_two_pass_case(c)
    assert bad == [], bad[:10]


@pytest.mark.parametrize("c", R.bwd_cap_cases(), ids=lambda c: c.name)
def test_backward_two_pass_exact_beyond_the_block_cap_grouped(c):
    """the same cases as a one-job group of kind 12 (reduce, then apply on its sums)"""
    bad = run_group_case(one_job_group(12, c))
    assert bad == [], bad[:10]


@pytest.mark.parametrize("c", R.bwd_cases(), ids=lambda c: c.name)
def test_backward_two_pass_exact(c):
    """mi_bn_act_bwd_reduce + mi_bn_act_bwd_apply: the forward's shapes, nblk 1 / 3 / more blocks than pixel lanes of work /
    1024, dres absent / overwritten / accumulated, dgamma and dbeta NULL: the accumulators after reduce (their sum over the
    live slots, the NaN pattern of the others), then dy, dres, dgamma, dbeta exactly"""
    bad = run_two_pass_case(c)
    assert bad == [], bad[:10]


@pytest.mark.parametrize("c", R.bwd_cases() + R.fused_capacity_cases(), ids=lambda c: c.name)
def test_backward_fused_exact(c):
    """mi_bn_act_bwd_fused, three launches on one barrier record: the same cases, and the capacity cases that pin the grid
    at 1, 2, 15, 16, 17, 33 blocks with 13 .. 20 items per thread; after every launch the outputs exactly, the folded totals
    in slot 0, and the barrier words: flag, top arrivals and every arrival counter 0, the generation of every used group
    equal to the number of launches, every other word still 0"""
    bad = run_fused_case(c)
    assert bad == [], bad[:10]


def test_fused_capacity_cases_reach_the_grids_and_item_counts():
    """what mi_bn_fused_set_capacity returns for the capacity cases is what they ask for (the device holds more), so the
    launcher's grid is the pinned one: nb in {1, 2, 15, 16, 17, 33}, items per thread 0, 1, 13 .. 20"""
    stats = dict(nb=set(), items=set())
    try:
        for c in R.fused_capacity_cases():
            cap = effective_capacity(c.cap)
            assert cap == c.cap
            nb = R.fused_blocks(c.npix, c.C, cap)
            stats["nb"].add(nb)
            stats["items"] |= R.nmine_set(c.npix, c.C, nb)
    finally:
        assert L.lib().mi_bn_fused_set_capacity(0) >= 33
    assert stats["nb"] == {1, 2, 15, 16, 17, 33} and stats["items"] >= {0, 1, 13, 14, 15, 16, 17, 19}, stats


@pytest.mark.parametrize("g", R.group_cases(), ids=lambda g: "kind%s-n%d-%s" % (g.kind, g.n, g.act))
def test_group_exact(g):
    """mi_bn_group_plan + mi_bn_group_run, kinds 0 - 3 (12 = reduce, then apply on its sums) with 1, 3, 8 jobs of different
    C, npix, ld and nslots, the table in a guarded device buffer: every job exact.  Kind 3 runs under a small capacity, so
    that the jobs share it: nblocks <= capacity, every job at least one block, the barrier words of every job"""
    bad = run_group_case(g)
    assert bad == [], bad[:10]


def test_eval_affine_within_derived_bound_and_exact_on_powers_of_four():
    """mi_bn_eval_affine against the float64 reference: random running statistics within bn_ref.eval_affine_bounds (derived
    there from correctly rounded fp32 sqrt and divide, hipcc's default for the file: 3.5 u |scale|, 4.5 u |rm scale| +
    u |shift|); and where the host's fp32 rv + eps is an exact power of four and gamma, rm, beta are short dyadics every
    operation is exact: equality"""
    lib = L.lib()
    for Cc in (8, 200, 2048):
        g = torch.Generator().manual_seed(Cc)
        for exact in (False, True):
            if exact:
                p4 = 4.0 ** torch.randint(-3, 3, (Cc,), generator=g).float()
                rv = p4 - torch.tensor(R.EPS, dtype=F32)
                keep = (rv + torch.tensor(R.EPS, dtype=F32)) == p4            # the host's fp32 emulation of rv + eps
                assert int(keep.sum()) > Cc // 4
                gamma = torch.randint(1, 13, (Cc,), generator=g).float() / 4
                beta = torch.randint(-16, 17, (Cc,), generator=g).float() / 8
                rm = torch.randint(-8, 9, (Cc,), generator=g).float() / 4
            else:
                keep = None
                rv = torch.rand(Cc, generator=g) * 4 + 1e-4
                gamma, beta, rm = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g), torch.randn(Cc, generator=g) * 3
            ins = [vec(t.to(F64), Cc) for t in (gamma, beta, rm, rv)]
            sc, sh = vec(NAN, Cc, other=SENT), vec(NAN, Cc, other=SENT)
            L.check(lib.mi_bn_eval_affine(*(b.ptr for b in ins), R.EPS, Cc, sc.ptr, sh.ptr, sp()), "mi_bn_eval_affine")
            torch.cuda.synchronize()
            assert sc.complaint("g", sc.view()) is None and sh.complaint("g", sh.view()) is None
            gs, gh = sc.view().reshape(-1).cpu(), sh.view().reshape(-1).cpu()
            d = lambda t: t.to(F64)
            if exact:
                inv = 1.0 / torch.sqrt(d(p4))
                es, eh = d(gamma) * inv, d(beta) - d(rm) * d(gamma) * inv
                assert torch.equal(gs[keep], es[keep]) and torch.equal(gh[keep], eh[keep])
            rs, rh = R.eval_affine(d(gamma), d(beta), d(rm), d(rv), R.EPS)
            bs, bh = R.eval_affine_bounds(d(gamma), d(beta), d(rm), d(rv), R.EPS)
            if exact:                                 # (the reference adds (double)(float)eps to the fp32 rv: not a power of four)
                bs, bh = bs + R.U32 * rs.abs(), bh + R.U32 * (d(rm) * rs).abs()
            print("C %d exact %d: scale %.2f, shift %.2f of the bound" % (Cc, exact, float(((gs - rs).abs() / bs).max()),
                                                                           float(((gh - rh).abs() / bh.clamp_min(1e-300)).max())))
            assert bool(((gs - rs).abs() <= bs).all()) and bool(((gh - rh).abs() <= bh).all())


def refused(rc, call):
    msg = L.lib().mi_last_error().decode()
    assert rc < 0 and call in msg, (call, rc, msg)


def test_refusals_leave_the_outputs_untouched():
    """every refusal returns < 0, mi_last_error names the call, and no output buffer is touched.  All buffers are valid and
    large enough for the nearest legal shape (C = 24, ld up to 48 for rows of 48 elements), so a refusal that failed to
    refuse could not leave them: null pointers; C % 8 != 0; C > 2048 (refused before anything is read); ld % 8 != 0; a
    misaligned y / a / res (forward) or da / y / dy / dres (reduce, apply, fused, group plan); count <= 0 in train mode;
    group jobs that disagree on act; more fused jobs than capacity; a run with nblocks > capacity; the 4 GB bound of the
    fused form, through mi_bn_group_plan kind 3, which launches nothing"""
    lib = L.lib()
    fc = R.FwdCase("refuse-f", 24, 40, 16, 8, 0, True, True, (48, 48, 48), "both", 41)
    fo = R.make_fwd_operands(fc)
    fj = FwdJob(fc, dev(fo))
    fj.refill()
    bc = R.BwdCase("refuse-b", 24, 40, 16, 4, 0, 2, (48, 48, 48, 48), 2, 0, False, 42)
    bj = BwdJob(bc, dev(R.make_bwd_operands(bc)))
    bj.refill()
    outs = fj.outputs() + [fj.rmean, fj.rvar, fj.nbt, bj.dacc, bj.dy, bj.dres, bj.dgamma, bj.dbeta, bj.bar]
    before = [b.flat.clone() for b in outs]

    def untouched(what):
        torch.cuda.synchronize()
        for b, f in zip(outs, before):
            assert torch.equal(b.flat.view(torch.uint8), f.view(torch.uint8)), what

    def fwd(what, **kw):
        names = ("y ldy acc nslots count gamma beta eps momentum rmean rvar nbt scale shift mean invstd res ldres a lda npix C act s").split()
        a = dict(zip(names, fj.args()))
        a.update(kw)
        refused(lib.mi_bn_act_fwd(*[a[n] for n in names]), "bn_act_fwd")
        untouched("fwd: " + what)
    fwd("null y", y=None)
    fwd("null a", a=None)
    fwd("null scale", scale=None)
    fwd("train mode without gamma", gamma=None)
    fwd("train mode without invstd", invstd=None)
    fwd("count 0", count=0)
    fwd("count < 0", count=-5)
    fwd("C % 8", C=20)
    fwd("C > 2048", C=2056)
    fwd("C 0", C=0)
    fwd("ldy % 8", ldy=44)
    fwd("lda % 8", lda=44)
    fwd("ldres % 8", ldres=44)
    fwd("misaligned y", y=fj.y.ptr + 2)
    fwd("misaligned a", a=fj.a.ptr + 8)
    fwd("misaligned res", res=fj.res.ptr + 4)

    rn = "da ldda y ldy scale shift mean invstd dacc nslots nblk npix C act s".split()
    an = "da ldda y ldy scale shift mean invstd gamma dacc nslots count dgamma dbeta dy lddy dres lddres accum npix C act".split()
    base_r = dict(zip(rn, bj.head() + (bj.dacc.ptr, bc.nslots, bc.nblk, bc.npix, bc.C, 0, sp())))
    base_a = dict(zip(an, bj.head() + (bj.gamma.ptr, bj.dacc.ptr, bc.nslots, bj.o.count) + bj.tail()))

    def red(what, **kw):
        a = dict(base_r)
        a.update(kw)
        refused(lib.mi_bn_act_bwd_reduce(*[a[n] for n in rn]), "bn_bwd_reduce")
        untouched("reduce: " + what)

    def app(what, **kw):
        a = dict(base_a)
        a.update(kw)
        refused(lib.mi_bn_act_bwd_apply(*[a[n] for n in an], sp()), "bn_bwd_apply")
        untouched("apply: " + what)
        refused(lib.mi_bn_act_bwd_fused(*[a[n] for n in an], bj.bar.ptr, sp()), "bn_bwd_fused")
        untouched("fused: " + what)
    red("null da", da=None)
    red("null dacc", dacc=None)
    red("C % 8", C=20)
    red("C > 2048", C=2056)
    red("ldda % 8", ldda=44)
    red("ldy % 8", ldy=44)
    red("nblk 0", nblk=0)
    red("misaligned da", da=bj.da.ptr + 2)
    red("misaligned y", y=bj.y.ptr + 8)
    app("null da", da=None)
    app("null gamma", gamma=None)
    app("null dy", dy=None)
    app("count 0", count=0)
    app("C % 8", C=20)
    app("C > 2048", C=2056)
    app("ldda % 8", ldda=44)
    app("lddy % 8", lddy=44)
    app("lddres % 8", lddres=44)
    app("misaligned da", da=bj.da.ptr + 2)
    app("misaligned y", y=bj.y.ptr + 4)
    app("misaligned dy", dy=bj.dy.ptr + 8)
    app("misaligned dres", dres=bj.dres.ptr + 2)
    a = dict(base_a)
    refused(lib.mi_bn_act_bwd_fused(*[a[n] for n in an], None, sp()), "bn_bwd_fused")
    untouched("fused: null barrier words")

    # the group plan (host side) and run
    meta = L.mi_bn_group()

    def plan(kind, what, n=2, call="bn_group_plan", **kw):
        arr = (L.mi_bn_job * n)()
        for j in arr:
            (fj if kind == 0 else bj).job(j)
        for k, v in kw.items():
            setattr(arr[n - 1], k, v)
        refused(lib.mi_bn_group_plan(kind, arr, n, None, 0, C.byref(meta)), call)
        untouched("plan kind %d: %s" % (kind, what))
    plan(0, "act differs", act=1)
    plan(0, "C % 8", C=20)
    plan(0, "C > 2048", C=2056)
    plan(0, "null y", y=None)
    plan(0, "ldy % 8", ldy=44)
    plan(0, "misaligned a", a=fj.a.ptr + 2)
    plan(0, "train mode, count 0", count=0)
    for kind in (1, 2, 3):
        plan(kind, "act differs", act=1)
        plan(kind, "null da", da=None)
        plan(kind, "ldda % 8", ldda=44)
        plan(kind, "ldy % 8", ldy=44)
        plan(kind, "misaligned da", da=bj.da.ptr + 2)
        plan(kind, "misaligned y", y=bj.y.ptr + 8)
    for kind in (2, 3):
        plan(kind, "lddy % 8", lddy=44)
        plan(kind, "lddres % 8", lddres=44)
        plan(kind, "misaligned dy", dy=bj.dy.ptr + 4)
        plan(kind, "misaligned dres", dres=bj.dres.ptr + 2)
        plan(kind, "count 0", count=0)
    plan(1, "nblk 0", nblk=0)
    plan(3, "null barrier words", bar=None)
    plan(3, "beyond 4 GB", npix=(1 << 32) // (48 * 2), ldy=48)          # npix * ld * 2 >= 2^32 - 4096; nothing is launched
    plan(0, "nine jobs", n=1 + 8)
    try:
        assert effective_capacity(2) == 2
        plan(3, "more fused jobs than capacity", n=3)
        assert lib.mi_bn_fused_set_capacity(0) >= 8
        meta, tab, _ = plan_group(3, [bj], 0)             # a real table of one job (one block) ...
        meta.nblocks = 3                                  # ... in a plan made for a larger budget than the one in effect at the
        assert effective_capacity(2) == 2                 # run (blocks beyond the job's own would find no pixel of theirs)
        refused(lib.mi_bn_group_run(C.byref(meta), tab.ptr, sp()), "bn_group_run")
        untouched("run with nblocks > capacity")
        refused(lib.mi_bn_group_run(C.byref(meta), None, sp()), "bn_group_run")
    finally:
        lib.mi_bn_fused_set_capacity(0)


def test_activation_sweep_over_every_bf16_value():
    """SiLU and SiLU' over every finite bf16 argument in one launch each: the eval-mode forward with scale 1, shift 0 (z = y
    exactly), and the apply kernel with gamma = invstd = 1, mean 0, zero sums, da = 1 (dy = act'(y) exactly as computed).
    Against RNE-bf16 of the float64 function the device may be off by half a bf16 ulp of the reference (the store) plus the
    fp32 evaluation error of sigmoidf_ (bn_ref.silu_bound / silu_grad_bound: ((2 |z| + 2)(1 - s) + 3) 2^-24 relative on
    the sigmoid, from 1-ulp v_exp_f32 and v_rcp_f32 and the rounding of each fp32 operation) plus the absolute floor 2^-100
    for the flush-to-zero of rcp.  The number of elements that differ from RNE(reference) at all is printed."""
    allv = R.all_finite_bf16()
    z = allv.to(F64)
    a = eval_forward(allv, 1.0, 0.0, 1).cpu()
    n = allv.numel() // 8
    scale, shift, mean, invstd, gamma = (vec(torch.full((8,), v, dtype=F64), 8) for v in (1.0, 0.0, 0.0, 1.0, 1.0))
    da, y, dy = Buf(n, 8, 8, BF, torch.ones(n, 8), NAN), Buf(n, 8, 8, BF, allv.reshape(n, 8), NAN), Buf(n, 8, 8, BF)
    dacc = Buf(R.SLOTS, 64, 64, F64, 0.0, NAN)
    L.check(L.lib().mi_bn_act_bwd_apply(da.ptr, 8, y.ptr, 8, scale.ptr, shift.ptr, mean.ptr, invstd.ptr, gamma.ptr,
                                        dacc.ptr, 16, 1 << 20, None, None, dy.ptr, 8, None, 0, 0, n, 8, 1, sp()), "apply")
    torch.cuda.synchronize()
    assert dy.complaint("guards", dy.view()) is None
    g = dy.view().reshape(-1).cpu()
    s = torch.sigmoid(z)
    for name, got, ref, bound in (("silu", a, z * s, R.silu_bound(z)), ("silu'", g, s * (1 + z * (1 - s)), R.silu_grad_bound(z))):
        assert not bool(got.isnan().any()), name
        lim = R.store_bound(ref, bound)
        err = (got - ref).abs()
        differ = int((got != R.bf16_rne(ref)).sum())
        print("%s: %d of %d elements differ from RNE(reference); largest error / bound %.3f" % (
            name, differ, z.numel(), float((err / lim).max())))
        assert bool((err <= lim).all()), (name, int((err > lim).sum()), float(z[(err > lim)][0]))


@pytest.mark.parametrize("nc", R.numerics_cases(), ids=lambda c: c.name)
def test_random_data_within_derived_bounds(nc):
    """Gaussian y and da, real statistics, SiLU, C = 80 / 264 / 24: the train-mode forward (statistics, running statistics,
    a), reduce + apply and the one-launch backward, every output elementwise inside the bounds bn_ref.numerics_* derives
    (rounding points, fp32 chains of known length, the sigmoid term); the float64 reference is fed the same bf16 inputs and
    the device's own fp32 scale / shift / mean / invstd; dgamma and dbeta per channel.  The fp32 emulation must stay inside
    the same bounds on the host first."""
    o = R.make_numerics_operands(nc)
    fc = R.FwdCase(nc.name, nc.C, nc.npix, nc.nslots, 0, 1, nc.res, True, (nc.C + 8, nc.C + 16, nc.C), "both", nc.seed)
    o.nbt0 = 3
    fj = FwdJob(fc, dev(types.SimpleNamespace(**vars(o))))
    fj.launch()
    p = R.fwd_prologue(o.acc, nc.nslots, o.count, o.gamma, o.beta, R.EPS, R.MOMENTUM, o.rmean0, o.rvar0)
    sb = R.stats_bounds(p, o.gamma, o.beta, R.MOMENTUM, o.rmean0, o.rvar0)
    st = {}
    for name, b in (("scale", fj.scale), ("shift", fj.shift), ("mean", fj.mean), ("invstd", fj.invstd), ("rmean", fj.rmean), ("rvar", fj.rvar)):
        assert b.complaint(name, b.view()) is None and not bool(b.view().isnan().any()), name
        st[name] = b.view().reshape(-1).cpu()
        err = (st[name] - getattr(p, name)).abs()
        assert bool((err <= getattr(sb, name)).all()), (name, float((err / getattr(sb, name)).max()))
    assert int(fj.nbt.view()) == 4
    sc, sh, mu, is_ = st["scale"], st["shift"], st["mean"], st["invstd"]
    gam = R.f32(o.gamma)
    _, PL, _ = R.tpb(nc.C)
    ref, bound = {}, {}
    ref["a"], bound["a"] = R.numerics_fwd(o, sc, sh)
    emu = R.emulate_numerics_fp32(o, sc, sh, mu, is_, gam, nc.dres)
    assert fj.a.complaint("a", fj.a.view()) is None
    got = {"a": fj.a.view().cpu()}
    bc = R.BwdCase(nc.name, nc.C, nc.npix, nc.nslots, 0, 1, nc.dres, (nc.C + 24, nc.C + 8, nc.C, nc.C + 16 if nc.dres else 0), nc.nblk,
                   0, False, nc.seed)
    bo = dev(types.SimpleNamespace(da=o.da, y=o.y, scale=sc, shift=sh, mean=mu, invstd=is_, gamma=gam, dres0=o.dres0, count=o.count))
    results = []
    for form in ("two-pass", "fused"):
        bj = BwdJob(bc, bo)
        bj.refill()
        if form == "two-pass":
            nb = nc.nblk
            L.check(L.lib().mi_bn_act_bwd_reduce(*bj.head(), bj.dacc.ptr, bc.nslots, nb, bc.npix, bc.C, 1, sp()), "reduce")
            L.check(L.lib().mi_bn_act_bwd_apply(*bj.head(), bj.gamma.ptr, bj.dacc.ptr, bc.nslots, o.count, *bj.tail(), sp()), "apply")
        else:
            nb = R.fused_blocks(bc.npix, bc.C, L.lib().mi_bn_fused_set_capacity(0))
            L.check(L.lib().mi_bn_act_bwd_fused(*bj.head(), bj.gamma.ptr, bj.dacc.ptr, bc.nslots, o.count, *bj.tail(), bj.bar.ptr, sp()), "fused")
        torch.cuda.synchronize()
        for name, b in (("dy", bj.dy), ("dres", bj.dres), ("dgamma", bj.dgamma), ("dbeta", bj.dbeta)):
            if b is not None:
                assert b.complaint(name, b.view()) is None and not bool(b.view().isnan().any()), (form, name)
        if form == "fused":
            assert bj.check_barrier([nb]) == []
        r, bd = R.numerics_bwd(o, sc, sh, mu, is_, gam, R.chain_length(nc.npix, nc.C, nb), nc.dres)
        g = dict(dy=bj.dy.view().cpu(), dgamma=bj.dgamma.view().reshape(-1).cpu(), dbeta=bj.dbeta.view().reshape(-1).cpu())
        if bj.dres is not None:
            g["dres"] = bj.dres.view().cpu()
        results.append((form, r, bd, g))
    r1, b1 = R.numerics_bwd(o, sc, sh, mu, is_, gam, R.chain_length(nc.npix, nc.C, 1), nc.dres)
    for k in list(r1) + ["a"]:                            # the emulation first (sums in one chain: the bound of one block)
        rr, bb = (ref[k], bound[k]) if k == "a" else (r1[k], b1[k])
        assert bool(((emu[k] - rr).abs() <= bb).all()), ("emulation", k)
    results.append(("forward", ref, bound, got))
    for form, r, bd, g in results:
        for k in g:
            err = (g[k] - r[k]).abs()
            ratio = float((err / bd[k].clamp_min(1e-300)).max()) if bool((bd[k] > 0).any()) else float(err.max())
            print("%s %s %s: error / bound %.3f" % (nc.name, form, k, ratio))
            assert bool((err <= bd[k]).all()), (form, k, int((err > bd[k]).sum()))


def test_mutants_fail_exactly_where_the_old_criteria_pass():
    """standing mutation evidence (bn_ref.fwd_mutants / bwd_mutants): the device's result equals the reference, and a
    reference with one pixel left out of a channel's sums, the neighbouring channel group's scale / shift for the last thread
    group, item R of a thread skipped in phase 2, ldy used for da, dres overwritten where it should accumulate, slot nslots
    read, or the biased variance in the running update is REJECTED by the exact comparison with that result under this
    file's hygiene and ACCEPTED by the older criteria (2e-2 norm-relative; one ulp / 2 % for the fused dy; 2e-3 for the
    running statistics) under theirs"""
    mutants_on_device()


def mutants_on_device():
    c = R.fwd_mutation_case()
    o = R.make_fwd_operands(c)
    R.assert_fwd_conditions(c, o, R.fwd_reference(c, o, 1))
    o = dev(o)
    r = R.fwd_reference(c, o, 1)
    job = FwdJob(c, o)
    job.launch()
    assert job.check(r, 0) == []
    got = dict(a=job.a.view(), scale=job.scale.view().reshape(-1), shift=job.shift.view().reshape(-1), mean=job.mean.view().reshape(-1),
               invstd=job.invstd.view().reshape(-1), rmean=job.rmean.view().reshape(-1), rvar=job.rvar.view().reshape(-1))
    ref = R.fwd_outputs(r)
    assert all(R.same(got[k], ref[k]) for k in ref)
    muts = R.fwd_mutants(c, o, r)
    assert len(muts) == 3
    for name, (exact, old) in muts.items():
        assert not all(R.same(got[k], exact[k]) for k in ref), name
        assert R.old_criteria_accept(ref, old), name
    c = R.bwd_mutation_case()
    job = make_bwd_job(c)
    try:
        cap = effective_capacity(c.cap)
        nb = R.fused_blocks(c.npix, c.C, cap)
        job.refill()
        job.fused()
    finally:
        L.lib().mi_bn_fused_set_capacity(0)
    assert job.check("fused") == []
    got = dict(dy=job.dy.view(), dgamma=job.dgamma.view().reshape(-1), dbeta=job.dbeta.view().reshape(-1), dres=job.dres.view())
    ref = R.bwd_outputs(job.r)
    muts = R.bwd_mutants(c, job.o, job.r, nb, 14, job.da.from_view())
    assert len(muts) == 4
    for name, (exact, old) in muts.items():
        assert not all(R.same(got[k], exact[k]) for k in ref), name
        assert R.old_criteria_accept(ref, old), name




# ------------------------------------------------------------------------------------------------------------- coverage
def test_every_instantiation_is_launched_by_an_exact_family():
    """the counted table: in this process the exact families launch every entry of bn_ref.instantiations() - the six
    streaming kernels, the two forms of the one-launch backward, and the grouped forms of all eight: 16"""
    SEEN.clear()
    bad = []
    for c in R.fwd_cases()[:4]:
        bad += run_fwd_case(c, launches=1)
    for c in R.bwd_cases()[:4]:
        bad += run_two_pass_case(c) + run_fused_case(c)
    for g in R.group_cases()[:6]:
        bad += run_group_case(g)
    assert bad == [], bad[:10]
    table = R.instantiations()
    for k in sorted(table):
        print("%-40s %d" % (k, SEEN.get(k, 0)))
    assert len(table) == 16 and set(SEEN) <= set(table), set(SEEN) - set(table)
    missing = [k for k in table if SEEN.get(k, 0) == 0]
    assert missing == [], missing
