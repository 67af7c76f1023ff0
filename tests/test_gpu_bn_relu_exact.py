"""GPU (-m gpu): the BatchNorm + ReLU kernels of csrc/bn_relu.hip - mi_bn_stats, mi_bn_relu_fwd (one norm, one norm + plain
residual, two norms; with and without the ReLU; train and eval mode) and mi_bn_relu_bwd_reduce / _apply (the same forms, dres
overwritten and accumulated) - against the plain float64 restatement of tests/bn_relu_ref.py with NO tolerance, through the
C ABI by ctypes.

The method is that of tests/test_gpu_bn_exact.py: operand families on which every fp32 / fp64 operation of the kernels is
exact (tests/bn_ref.py: dyadic statistics with invstd in {1, 2, 4} for the forward, small integers on a 2^-(k+2) grid for the
backward; the ReLU and its mask are exact on any operand), so the device must equal the float64 reference - rounded once to
bf16 where a kernel stores bf16 - bit for bit, whatever the fma contraction, summation order, block count, slot count or
atomic arrival order.  The conditions are asserted on the reference of every case before anything is launched.

Hygiene of every launch: every output lives in a buffer of sentinel words - guards before and after the view and, with a
leading dimension above C, the pad channels [C, ld) of every row - that must survive; outputs are pre-filled with NaN before
every launch and every element must have been written; input buffers hold NaN outside their views; the accumulator slots
>= nslots and the pad channels [C, CA) of every slot hold NaN (forward and apply must not read them, stats and reduce must not
write them); dres starts as NaN when it is overwritten (reduce must have written all of it, apply must leave it) and as integers
when it accumulates; one shape per width runs with
pairwise different leading dimensions above C.  C in {8, 24, 56, 152, 368} (C8 = 1 and RegNetX-200MF's 3, 7, 19, 46: 256, 255,
252, 247 and 230 working threads), npix = count in {64, 1024}, nslots in {1, 16}.  The running mean of three launches is exact,
the running variance follows bn_ref.running_var_fp32 / rvar_tolerance."""
import ctypes as C

import pytest
import torch

import bn_ref as B
import bn_relu_ref as R
from yolov7_d2_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -1536.0                 # sentinel (exact in bf16, fp32, fp64 and the integer types)
GUARD = 64                     # guard elements around every buffer
NAN = float("nan")
F64, BF, F32 = torch.float64, torch.bfloat16, torch.float32
SHAPES = R.shapes()


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

    def complaint(self, name, value):
        """None if the WHOLE buffer is `value` (NaN = NaN) in the view and untouched elsewhere"""
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


def vec(value, Cc, dtype=F32, other=NAN):
    """a per-channel input vector (NaN around it) or, with value = NAN, a per-channel output (sentinels around it)"""
    return Buf(1, Cc, Cc, dtype, value, other)


def acc_buf(s, live):
    """accumulators [SLOTS][CA][2]: `live` ([nslots][C][2] or a scalar) in the slots < nslots and channels < C, NaN elsewhere"""
    CA, n = B.acc_c(s.C), B.norm_slots(s.nslots)
    t = torch.full((B.SLOTS, CA, 2), NAN, dtype=F64)
    t[:n, :s.C] = live
    return Buf(B.SLOTS, CA * 2, CA * 2, F64, t.reshape(B.SLOTS, CA * 2), NAN), t


def slot_total(buf, s):
    """the live part of an accumulator buffer summed in slot order -> [C][2]; the rest must still be NaN"""
    CA, n = B.acc_c(s.C), B.norm_slots(s.nslots)
    v = buf.view().reshape(B.SLOTS, CA, 2)
    assert bool(v[n:].isnan().all()) and bool(v[:, s.C:].isnan().all()), "an unused slot / pad channel of the accumulators was written"
    return B.slot_sums(v[:, :s.C], n)


# ------------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("s", SHAPES + [R.Shape(56, 1024, 3)], ids=R.shape_id)
def test_stats_exact_on_a_channel_slice(s):
    x = R.stats_case(s, 1)
    wide = s.C + 24                                            # the map is channels [8, 8 + C) of a wider one
    full = torch.randint(-64, 65, (s.npix, wide), generator=torch.Generator().manual_seed(5)).to(F64)
    full[:, 8:8 + s.C] = x
    m = Buf(s.npix, wide, wide, BF, full, NAN)
    acc, _ = acc_buf(s, 0.0)
    L.check(L.lib().mi_bn_stats(m.ptr + 16, wide, s.npix, s.C, acc.ptr, s.nslots, sp()), "mi_bn_stats")
    torch.cuda.synchronize()
    s1, s2 = R.stats(x)
    got = slot_total(acc, s)
    assert torch.equal(got[:, 0].cpu(), s1) and torch.equal(got[:, 1].cpu(), s2)
    assert acc.complaint("acc guards", acc.view()) is None
    assert m.complaint("x (an input)", full) is None


# ---------------------------------------------------------------------------------------------------------------- forward
class FwdNorm:
    """the buffers of one norm operand of a forward case"""

    def __init__(self, s, c, o, ldy):
        Cc = s.C
        self.train = c.train
        self.y = Buf(s.npix, Cc, ldy, BF, o.y, NAN)
        self.ldy = ldy
        self.acc = self.gamma = self.beta = self.mean = self.invstd = self.rmean = self.rvar = self.nbt = None
        if c.train:
            CA = B.acc_c(Cc)
            self.acc = Buf(B.SLOTS, CA * 2, CA * 2, F64, o.acc.reshape(B.SLOTS, CA * 2), NAN)
            self.gamma, self.beta = vec(o.gamma, Cc), vec(o.beta, Cc)
            self.scale, self.shift, self.mean, self.invstd = (vec(NAN, Cc, other=SENT) for _ in range(4))
            self.rmean, self.rvar = vec(o.rmean0, Cc, other=SENT), vec(o.rvar0, Cc, other=SENT)
            self.nbt = Buf(1, 1, 1, torch.int64, o.nbt0, int(SENT))
        else:
            self.scale, self.shift = vec(o.scale, Cc, other=SENT), vec(o.shift, Cc, other=SENT)
        self.o = o

    def fill(self, n, s, count):
        p = lambda b: None if b is None else b.ptr
        n.y, n.ldy, n.acc, n.nslots, n.count = self.y.ptr, self.ldy, p(self.acc), s.nslots, count
        n.gamma, n.beta, n.eps, n.momentum = p(self.gamma), p(self.beta), R.EPS, R.MOMENTUM
        n.running_mean, n.running_var, n.num_batches_tracked = p(self.rmean), p(self.rvar), p(self.nbt)
        n.scale, n.shift, n.mean, n.invstd = self.scale.ptr, self.shift.ptr, p(self.mean), p(self.invstd)

    def refill(self):
        if self.train:
            for b in (self.scale, self.shift, self.mean, self.invstd):
                b.set(NAN)

    def check(self, r, i, tag):
        bad = []
        add = lambda m: bad.append(m) if m else None
        add(self.scale.complaint(tag + "scale", r.scale))
        add(self.shift.complaint(tag + "shift", r.shift))
        add(self.y.complaint(tag + "y (an input)", self.o.y))
        if self.train:
            add(self.mean.complaint(tag + "mean", r.mean))
            add(self.invstd.complaint(tag + "invstd", r.invstd))
            add(self.acc.complaint(tag + "acc (an input)", self.o.acc))
            add(self.rmean.complaint(tag + "running_mean after launch %d" % (i + 1), r.rmean[i]))
            rv = self.rvar.view().reshape(-1)
            if not bool(((rv.cpu() - r.rvar[i]).abs() <= r.rvar_tol[i]).all()):
                bad.append(tag + "running_var after launch %d: off by %.3g (bound %.3g)" % (
                    i + 1, float((rv.cpu() - r.rvar[i]).abs().max()), float(r.rvar_tol[i].max())))
            add(self.rvar.complaint(tag + "running_var guards", rv))
            add(self.nbt.complaint(tag + "num_batches_tracked", torch.tensor([float(r.nbt[i])])))
        return bad


def run_fwd(s, form, relu, train, seed):
    k = R.fwd_case(s, form, relu, train, seed)
    ld = R.lds(s, 4, R.different_lds(s))                       # y1, y2 / res, a
    ops = [FwdNorm(s, k.c[j], k.o[j], ld[j]) for j in range(len(k.o))]
    res = Buf(s.npix, s.C, ld[1], BF, k.res, NAN) if form == "res" else None
    a = Buf(s.npix, s.C, ld[2], BF)
    d = L.mi_bn_relu_desc()
    ops[0].fill(d.n1, s, k.o[0].count)
    if form == "two":
        ops[1].fill(d.n2, s, k.o[1].count)
    if res is not None:
        d.res, d.ldres = res.ptr, ld[1]
    d.a, d.lda, d.npix, d.C, d.relu = a.ptr, ld[2], s.npix, s.C, relu
    bad = []
    for i in range(3 if train else 1):
        a.set(NAN)
        for op in ops:
            op.refill()
        L.check(L.lib().mi_bn_relu_fwd(C.byref(d), sp()), "mi_bn_relu_fwd")
        torch.cuda.synchronize()
        m = a.complaint("a", k.a)
        if m:
            bad.append(m)
        for j, op in enumerate(ops):
            bad += op.check(k.r[j], i, "n%d." % (j + 1))
        if res is not None and res.complaint("res (an input)", k.res):
            bad.append("res was written")
    return ["%s %s relu %d train %d: %s" % (R.shape_id(s), form, relu, train, b) for b in bad]


@pytest.mark.parametrize("s", SHAPES, ids=R.shape_id)
def test_forward_exact(s):
    seed = SHAPES.index(s)
    bad = []
    for form in R.FORMS:
        for relu in (0, 1):
            for train in (True, False):
                bad += run_fwd(s, form, relu, train, seed)
    assert not bad, "\n".join(bad[:20])


# --------------------------------------------------------------------------------------------------------------- backward
def run_bwd(s, form, relu, mode, seed):
    k = R.bwd_case(s, form, relu, mode, seed)
    ld = R.lds(s, 8, R.different_lds(s))                       # da, a, y1, y2, dy1, dy2, dres
    da = Buf(s.npix, s.C, ld[0], BF, k.da, NAN)
    a = Buf(s.npix, s.C, ld[1], BF, k.a, NAN) if relu else None     # relu == 0: a is not read and may be NULL
    d = L.mi_bn_relu_desc()
    ops = []
    for j, o in enumerate(k.o):
        n = d.n1 if j == 0 else d.n2
        t = dict(y=Buf(s.npix, s.C, ld[2 + j], BF, o.y, NAN), mean=vec(o.mean, s.C), invstd=vec(o.invstd, s.C),
                 gamma=vec(o.gamma, s.C), dy=Buf(s.npix, s.C, ld[4 + j], BF), dgamma=vec(NAN, s.C, other=SENT),
                 dbeta=vec(NAN, s.C, other=SENT), o=o)
        t["dacc"], _ = acc_buf(s, 0.0)
        n.y, n.ldy, n.mean, n.invstd, n.gamma = t["y"].ptr, ld[2 + j], t["mean"].ptr, t["invstd"].ptr, t["gamma"].ptr
        n.dacc, n.nslots, n.count = t["dacc"].ptr, s.nslots, k.count
        n.dy, n.lddy, n.dgamma, n.dbeta = t["dy"].ptr, ld[4 + j], t["dgamma"].ptr, t["dbeta"].ptr
        ops.append(t)
    dres = None
    if mode:
        dres = Buf(s.npix, s.C, ld[6], BF, k.dres0 if mode == 2 else NAN)
        d.dres, d.lddres, d.accumulate = dres.ptr, ld[6], int(mode == 2)
    d.da, d.ldda, d.npix, d.C, d.relu = da.ptr, ld[0], s.npix, s.C, relu
    if a is not None:
        d.a, d.lda = a.ptr, ld[1]
    bad = []
    add = lambda m: bad.append(m) if m else None
    L.check(L.lib().mi_bn_relu_bwd_reduce(C.byref(d), sp()), "mi_bn_relu_bwd_reduce")
    torch.cuda.synchronize()
    for j, t in enumerate(ops):
        got = slot_total(t["dacc"], s).cpu()
        if not (torch.equal(got[:, 0], k.r[j].s1) and torch.equal(got[:, 1], k.r[j].s2)):
            bad.append("n%d: the reduce sums differ" % (j + 1))
        add(t["dacc"].complaint("n%d.dacc guards" % (j + 1), t["dacc"].view()))
        add(t["dy"].complaint("n%d.dy after reduce (must be untouched)" % (j + 1), torch.full((s.npix, s.C), NAN, dtype=F64)))
    if dres is not None:    # overwritten: reduce stores dz there for apply (the header's exception); accumulated: untouched so far
        add(dres.complaint("dres after reduce", k.dres0 if mode == 2 else k.dres))
    L.check(L.lib().mi_bn_relu_bwd_apply(C.byref(d), sp()), "mi_bn_relu_bwd_apply")
    torch.cuda.synchronize()
    for j, t in enumerate(ops):
        tag = "n%d." % (j + 1)
        add(t["dy"].complaint(tag + "dy", k.r[j].dy))
        add(t["dgamma"].complaint(tag + "dgamma", k.r[j].dgamma))
        add(t["dbeta"].complaint(tag + "dbeta", k.r[j].dbeta))
        add(t["y"].complaint(tag + "y (an input)", t["o"].y))
    if dres is not None:
        add(dres.complaint("dres", k.dres))
    add(da.complaint("da (an input)", k.da))
    if a is not None:
        add(a.complaint("a (an input)", k.a))
    return ["%s %s relu %d dres %d: %s" % (R.shape_id(s), form, relu, mode, b) for b in bad]


@pytest.mark.parametrize("s", SHAPES, ids=R.shape_id)
def test_backward_exact(s):
    seed = SHAPES.index(s)
    bad = []
    for form, mode in (("one", 0), ("two", 0), ("res", 1), ("res", 2)):
        for relu in (0, 1):
            bad += run_bwd(s, form, relu, mode, seed)
    assert not bad, "\n".join(bad[:20])


def test_refusals_leave_the_output_untouched():
    """an argument error returns before anything is launched: the output keeps its NaN fill"""
    s = R.Shape(24, 64, 1)
    k = R.fwd_case(s, "one", 1, False, 0)
    op = FwdNorm(s, k.c[0], k.o[0], 24)
    a = Buf(s.npix, s.C, 24, BF)
    d = L.mi_bn_relu_desc()
    op.fill(d.n1, s, 0)
    d.a, d.lda, d.npix, d.C, d.relu = a.ptr, 24, s.npix, s.C, 1
    lib = L.lib()
    for field, value, word in (("C", 20, b"C 20"), ("lda", 28, b"multiple of 8"), ("a", a.ptr + 2, b"aligned"), ("res", a.ptr, None)):
        old = getattr(d, field)
        setattr(d, field, value)
        if field == "res":
            d.n2.y, d.n2.ldy, d.n2.scale, d.n2.shift = op.y.ptr, 24, op.scale.ptr, op.shift.ptr
            word = b"both"
        assert lib.mi_bn_relu_fwd(C.byref(d), sp()) == -1 and word in lib.mi_last_error(), (field, lib.mi_last_error())
        setattr(d, field, old)
        d.n2.y = None
    torch.cuda.synchronize()
    assert a.complaint("a", torch.full((s.npix, s.C), NAN, dtype=F64)) is None
    L.check(lib.mi_bn_relu_fwd(C.byref(d), sp()), "mi_bn_relu_fwd")
    torch.cuda.synchronize()
    assert a.complaint("a", k.a) is None
