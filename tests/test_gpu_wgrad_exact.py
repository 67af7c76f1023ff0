"""GPU (-m gpu): the convolution weight-gradient kernels (csrc/conv_wgrad.hip) against the plain float64 reference of
tests/wgrad_ref.py with NO tolerance, through the C ABI (mi_conv2d_wgrad_plan / mi_conv2d_wgrad / mi_conv2d_wgrad_group_plan /
_run), in every tile configuration of MI_WG_ALL and every launch form: single, one grid per configuration, the mixed grid
of the 1x1 layers.

The method: the bf16 operands hold small integers (wgrad_ref.make_operands), so every product is exact in fp32 and every
partial sum is an integer below 2^24 whatever the order of summation: the result does not depend on the split-K layout, the
LDS ring depth or the block order, and any correct configuration equals the reference BIT FOR BIT (torch.equal).  One dropped
halo pixel, one mis-clipped ragged-tile row, one wrong tap, channel or split fails - the norm-relative tolerances of the other
weight-gradient tests hide such an error at about 1 / sqrt(pixels).  test_premise_* checks the premise on the device,
test_a_transposed_tap_table_does_not_pass is the standing evidence that a one-tap error cannot pass.

Hygiene of every launch (Job / run_single / run_group): the gradient sits between sentinel guard words that must stay
untouched; it is pre-filled with NaN unless it accumulates, so every element must be written; the split-K workspace is exactly
the planned size plus a guard, all 0xFF bytes (NaN as fp32): the guard must stay intact and a stale partial must never be read
as a sum; the operand buffers are NaN outside the descriptor's views."""
import collections
import ctypes as C
import functools

import pytest
import torch

import wgrad_ref as R
from yolov7_d2_amd import _lib as L
from yolov7_d2_amd.modeling.resnet import _STEM_TAPS
from yolov7_d2_amd.modeling.transformer import _factor

pytestmark = pytest.mark.gpu
DEV = "cuda"
MI_EINVAL = -1                 # include/mi355_det.h
SENT = -1234.5                 # guard words around a gradient
GW_GUARD, WS_GUARD = 64, 256   # floats / bytes

# MI_WG_ALL of csrc/conv_wgrad.hip, written out: (NT, MI, NJ, WCO, WCI, TP) - 28 instantiations
WG_ALL = ({(9, 4, 1, 1, 4, tp) for tp in (64, 128)} | {(9, 2, 1, 2, 2, tp) for tp in (64, 128)} |
          {(9, 1, 1, 2, 2, tp) for tp in (64, 128)} | {(9, 1, 1, 2, 1, tp) for tp in (64, 128)} |
          {(16, 1, 1, 2, 1, tp) for tp in (64, 128)} |
          {(1, mi, nj, 2, 2, tp) for mi in (1, 2, 4) for nj in (1, 2, 4) for tp in (64, 128)})
assert len(WG_ALL) == 28

Spec = collections.namedtuple("Spec", "taps stride N H W oH oW Cin Cout CinPad CoutPad ldx x_off ldy dy_off seed")


def _rup(a, b):
    return (a + b - 1) // b * b


def spec(k, stride, Cin, Cout, N, H, W, CinPad=None, CoutPad=None, wide=False, seed=0):
    """k = 1 / 3: a k x k convolution with padding k // 2; k = 16: the ResNet stem's 4 x 4 table over the space-to-depth image.
    wide: both operands are the UPPER channel slice of a buffer twice as wide (the lower half is NaN)."""
    if k == 16:
        taps, (oH, oW) = tuple((a, b) for a, b, _ in _STEM_TAPS), (H, W)
    else:
        taps, (oH, oW) = tuple(R.square_taps(k)), R.conv_out(H, W, k, stride)
    CinPad = CinPad or _rup(Cin, 32 if k == 1 else 16)
    CoutPad = CoutPad or _rup(Cout, 32)
    m = 2 if wide else 1
    return Spec(taps, stride, N, H, W, oH, oW, Cin, Cout, CinPad, CoutPad, m * CinPad, (m - 1) * CinPad, m * CoutPad,
                (m - 1) * CoutPad, seed)


@functools.lru_cache(maxsize=None)
def _ops(s):
    """operands on the device and the references, once per Spec (shared by every launch of it; never modified)"""
    xb, dyb, x, dy = R.make_operands(s.N, s.H, s.W, s.oH, s.oW, s.Cin, s.Cout, s.CinPad, s.CoutPad, s.seed, s.ldx, s.x_off,
                                     s.ldy, s.dy_off)
    ref = R.wgrad_reference(x, dy, list(s.taps), s.stride, s.Cin, s.Cout)
    return dict(xd=xb.to(DEV), dyd=dyb.to(DEV), x=x, dy=dy, ref=ref, bref=R.bias_reference(dy, s.Cout))


def _f32_exact(t64):
    t32 = t64.to(torch.float32)
    assert torch.equal(t32.double(), t64), "the expected value is not exact in fp32: the case breaks the method's premise"
    return t32


class Job:
    """one descriptor with its gradient buffers and its expected result"""

    def __init__(self, s, TH=0, TW=0, splitk=0, cfg_tp=0, cfg_ns=0, accumulate=0, scaled=False, gbias=False, gw=None, taps=None,
                 ops=None):
        self.s, self.o = s, (ops or _ops(s))
        self.kw = dict(TH=TH, TW=TW, splitk=splitk, cfg_tp=cfg_tp, cfg_ns=cfg_ns, accumulate=accumulate)
        self.taps = tuple(taps) if taps else s.taps            # the table handed to the kernel
        self.shape = (s.Cout, s.Cin, len(s.taps))
        n = s.Cout * s.Cin * len(s.taps)
        g = torch.Generator().manual_seed(1000 + s.seed)
        self.buf = None
        if gw is None:                                         # (else: a slice of a tensor the test owns and checks)
            self.buf = torch.full((n + 2 * GW_GUARD,), SENT, device=DEV)
            gw = self.buf[GW_GUARD:GW_GUARD + n]
        self.gw = gw
        self.g0 = None
        if accumulate:
            self.g0 = torch.randint(-50, 51, self.shape, generator=g).double()
            self.gw.copy_(self.g0.float().reshape(-1))
        else:
            self.gw.fill_(float("nan"))
        self.rs = self.rsd = None
        if scaled:                                             # signed powers of two: the scaled sums stay exact
            self.rs = (2.0 ** torch.randint(-3, 4, (s.Cout,), generator=g).double()) * (torch.randint(0, 2, (s.Cout,), generator=g) * 2 - 1)
            self.rsd = self.rs.float().to(DEV)
        self.gbbuf = None
        if gbias:
            self.gbbuf = torch.full((s.Cout + 2 * GW_GUARD,), SENT, device=DEV)
            self.gbbuf[GW_GUARD:GW_GUARD + s.Cout] = float("nan")

    def fill(self, d):
        s = self.s
        d.x, d.dy, d.gw = self.o["xd"].data_ptr() + 2 * s.x_off, self.o["dyd"].data_ptr() + 2 * s.dy_off, self.gw.data_ptr()
        d.ldx, d.ldy = s.ldx, s.ldy
        d.N, d.H, d.W, d.outH, d.outW, d.stride = s.N, s.H, s.W, s.oH, s.oW, s.stride
        d.Cin, d.Cout, d.CinPad, d.CoutPad, d.ntaps = s.Cin, s.Cout, s.CinPad, s.CoutPad, len(self.taps)
        for t, (a, b) in enumerate(self.taps):
            d.tap_dy[t], d.tap_dx[t] = a, b
        for k, v in self.kw.items():
            setattr(d, k, v)
        d.row_scale = self.rsd.data_ptr() if self.rsd is not None else None
        d.gbias = self.gbbuf.data_ptr() + 4 * GW_GUARD if self.gbbuf is not None else None
        return d

    def expected(self, runs=1, ref=None):
        e = self.o["ref"] if ref is None else ref
        if self.rs is not None:
            e = e * self.rs[:, None, None]
        if self.g0 is not None:
            e = self.g0 + runs * e
        return _f32_exact(e)

    def problems(self, label, runs=1, ref=None):
        """what is wrong with the buffers after `runs` launches (an empty list: nothing)"""
        bad = []
        if self.buf is not None:
            h = self.buf.cpu()
            if not (torch.all(h[:GW_GUARD] == SENT) and torch.all(h[-GW_GUARD:] == SENT)):
                bad.append((label, "guard words around gw were written"))
            got = h[GW_GUARD:-GW_GUARD]
        else:
            got = self.gw.cpu()
        got, exp = got.view(self.shape), self.expected(runs, ref)
        if not torch.equal(got, exp):
            ne = got != exp
            taps = sorted(set(torch.nonzero(ne)[:, 2].tolist()))
            bad.append((label, "gw: %d of %d elements differ (%d NaN), max |diff| %g, taps %s" % (
                int(ne.sum()), ne.numel(), int(got.isnan().sum()), float((got - exp).nan_to_num(0.0).abs().max()), taps)))
        if self.gbbuf is not None:
            h = self.gbbuf.cpu()
            if not (torch.all(h[:GW_GUARD] == SENT) and torch.all(h[-GW_GUARD:] == SENT)):
                bad.append((label, "guard words around gbias were written"))
            if not torch.equal(h[GW_GUARD:-GW_GUARD], _f32_exact(self.o["bref"])):
                bad.append((label, "gbias differs: max |diff| %g" % float((h[GW_GUARD:-GW_GUARD] - self.o["bref"].float()).abs().max())))
        return bad


def plan_bytes(job, **over):
    d = job.fill(L.mi_wgrad_desc())
    for k, v in over.items():
        setattr(d, k, v)
    need = int(L.lib().mi_conv2d_wgrad_plan(C.byref(d)))
    assert need > 0, (need, L.lib().mi_last_error())
    return need


def split_count(s, **kw):
    """the split-K count the launcher takes for these descriptor fields: workspace bytes over the bytes of one split"""
    j = Job(s, **kw)
    return plan_bytes(j) // plan_bytes(j, splitk=1)


def ntiles_of(s, **kw):
    kw = dict(kw, splitk=1 << 20)        # (clamped to one pixel tile per split)
    return split_count(s, **kw)


def run_single(job, label, runs=1):
    """mi_conv2d_wgrad on an exactly sized, 0xFF-filled workspace; returns the list of problems"""
    lib = L.lib()
    d = job.fill(L.mi_wgrad_desc())
    need = int(lib.mi_conv2d_wgrad_plan(C.byref(d)))
    assert need > 0, (label, need, lib.mi_last_error())
    ws = torch.full((need + WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    d.ws, d.ws_bytes = ws.data_ptr(), need
    for _ in range(runs):
        L.check(lib.mi_conv2d_wgrad(C.byref(d), L.stream_ptr()), "mi_conv2d_wgrad %s" % (label,))
    torch.cuda.synchronize()
    bad = job.problems(label, runs)
    if not bool((ws[need:] == 0xFF).all()):
        bad.append((label, "the guard behind the workspace was written"))
    return bad


def run_group(jobs, labels, runs=1):
    """mi_conv2d_wgrad_group_plan / _run (MI_WG_MULTI is read from the environment per plan); returns (problems, meta)"""
    lib = L.lib()
    descs = (L.mi_wgrad_desc * len(jobs))()
    for d, j in zip(descs, jobs):
        j.fill(d)
    meta = L.mi_wgrad_group()
    L.check(lib.mi_conv2d_wgrad_group_plan(descs, len(jobs), None, None, 0, C.byref(meta)), "group plan (sizes)")
    need = int(meta.ws_bytes)
    ws = torch.full((need + WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    host = (C.c_char * int(meta.table_bytes))()
    L.check(lib.mi_conv2d_wgrad_group_plan(descs, len(jobs), ws.data_ptr(), host, meta.table_bytes, C.byref(meta)), "group plan")
    assert int(meta.ws_bytes) == need
    table = torch.frombuffer(bytearray(bytes(host)[:int(meta.table_bytes)]), dtype=torch.uint8).to(DEV)
    bad = []
    for r in range(runs):
        L.check(lib.mi_conv2d_wgrad_group_run(C.byref(meta), table.data_ptr(), L.stream_ptr()), "group run")
        torch.cuda.synchronize()
        for j, lab in zip(jobs, labels):
            bad += j.problems((lab, "run %d" % r), r + 1)
    if not bool((ws[need:] == 0xFF).all()):
        bad.append(("group", "the guard behind the workspace was written"))
    return bad, meta


def group_cfgs(meta):
    return [tuple(meta.g[i].cfg) for i in range(meta.ngroups)]


# ------------------------------------------------------------------------------------------------------- (a) the premise
def test_premise_mfma_sums_of_integers_are_exact():
    """fp32 accumulation of exactly representable values in the matrix cores: small integers (the operands of this file) and
    integers up to 255 (16-bit products, sums up to 2^21) equal the integer product exactly"""
    g = torch.Generator().manual_seed(0)
    for name, (m, k, n) in (("mi_probe_mfma32", (32, 16, 32)), ("mi_probe_mfma16", (16, 32, 16))):
        for amax, bmax in ((R.DY_MAX, R.X_MAX), (255, 255)):
            a = torch.randint(-amax, amax + 1, (m, k), generator=g)
            b = torch.randint(-bmax, bmax + 1, (k, n), generator=g)
            d = torch.full((m, n), float("nan"), device=DEV)
            ad, bd = a.to(DEV, torch.bfloat16), b.to(DEV, torch.bfloat16)
            assert torch.equal(ad.cpu().long(), a) and torch.equal(bd.cpu().long(), b)       # exact in bf16
            L.check(getattr(L.lib(), name)(ad.data_ptr(), bd.data_ptr(), d.data_ptr(), L.stream_ptr()), name)
            torch.cuda.synchronize()
            assert torch.equal(d.cpu().double(), (a @ b).double()), (name, amax)


# --------------------------------------------------------------------------------------------- (b) every instantiation
CLASSES_3X3 = [(64, 64, 1), (32, 64, 1), (32, 64, 2), (64, 64, 2), (32, 32, 1), (32, 96, 2), (16, 32, 1), (16, 32, 2)]   # (CinPad, CoutPad, stride)


@functools.lru_cache(maxsize=None)
def matrix_b():
    """one case per channel class of wg_pick_cfg; each runs at cfg_tp 64 and 128.  Ragged maps, real channel counts below the
    pads where the class allows it."""
    out = []
    for i, (ci, co, st) in enumerate(CLASSES_3X3):
        out.append(("3x3 pads (%d, %d) stride %d" % (ci, co, st), spec(3, st, ci - 3, co - 5, 2, 19, 23, seed=10 + i)))
    out.append(("16-tap stem", spec(16, 1, 12, 64, 2, 15, 18, seed=30)))
    for i, co in enumerate((32, 64, 128)):
        for k, ci in enumerate((32, 64, 128)):
            out.append(("1x1 pads (%d, %d)" % (ci, co), spec(1, 1, ci - 1, co - 2, 2, 19, 23, seed=40 + 3 * i + k)))
    out.append(("1x1 96 -> 192", spec(1, 1, 96, 192, 2, 19, 23, seed=50)))
    out.append(("1x1 512 -> 256", spec(1, 1, 512, 256, 1, 20, 20, seed=51)))
    out.append(("1x1 256 -> 512", spec(1, 1, 256, 512, 1, 20, 20, seed=52)))
    return out


def matrix_b_jobs(**kw):
    jobs, labels = [], []
    for name, s in matrix_b():
        for tp in (64, 128):
            jobs.append(Job(s, cfg_tp=tp, **kw))
            labels.append((name, "cfg_tp %d" % tp))
    return jobs, labels


def test_every_instantiation_single_launch(monkeypatch):
    monkeypatch.setenv("MI_WG_MULTI", "0")
    seen = set()
    for j, lab in zip(*matrix_b_jobs()):      # coverage is asserted, not assumed: the configuration the launcher picks
        meta = L.mi_wgrad_group()
        descs = (L.mi_wgrad_desc * 1)()
        j.fill(descs[0])
        L.check(L.lib().mi_conv2d_wgrad_group_plan(descs, 1, None, None, 0, C.byref(meta)), "one-job group plan")
        assert meta.ngroups == 1, lab
        seen.add(tuple(meta.g[0].cfg))
    assert seen == WG_ALL, (sorted(WG_ALL - seen), sorted(seen - WG_ALL))
    bad = []
    for j, lab in zip(*matrix_b_jobs()):
        bad += run_single(j, lab)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ (c) geometry
GEO_CLASSES = {
    "3x3s1": lambda N, H, W, seed: spec(3, 1, 29, 61, N, H, W, seed=seed),          # pads (32, 64): MI 2, 2 x 2 waves
    "3x3s2": lambda N, H, W, seed: spec(3, 2, 29, 61, N, H, W, seed=seed),
    "1x1": lambda N, H, W, seed: spec(1, 1, 61, 61, N, H, W, seed=seed),            # pads (64, 64): MI 2, NJ 2
}
# output maps (N = 3: a split's tile range crosses image boundaries): one that fits its 64- and 128-pixel tiles exactly, one
# ragged in both dimensions, one narrower than every tile candidate, single rows, and the token rows of the transformer
GEO_MAPS = [(8, 16), (13, 17), (5, 3), (1, 37), _factor(37), _factor(200)]
S2_PARITIES = [(20, 26), (20, 27), (21, 26), (21, 27)]
TILES = [(1, 64), (64, 1), (8, 8), (5, 7)]       # (5 x 7 = 35 < TP: the rows past TH * TW)


def _geo_specs(cls):
    mk = GEO_CLASSES[cls]
    if cls == "3x3s2":        # the input maps whose outputs are GEO_MAPS (even and odd inputs), then all four parities
        ins = [(2 * h - (i & 1), 2 * w - ((i >> 1) & 1)) for i, (h, w) in enumerate(GEO_MAPS)] + S2_PARITIES
    else:
        ins = GEO_MAPS
    return [mk(3, h, w, 100 + i) for i, (h, w) in enumerate(ins)]


@pytest.mark.parametrize("cls", list(GEO_CLASSES))
def test_geometry_tiles_splits_ring_and_block_order(cls):
    bad = []
    for s in _geo_specs(cls):
        nt = ntiles_of(s)
        variants = [dict(), dict(cfg_tp=128)]
        variants += [dict(TH=th, TW=tw, cfg_tp=tp) for th, tw in TILES for tp in (64, 128)]
        variants += [dict(splitk=k) for k in (1, 2, 3, 7, nt, nt + 5)]
        variants += [dict(cfg_ns=ns, splitk=k) for ns in (2, 3, 4) for k in (1, nt)]     # (nt: one tile per split < ns - 1)
        for kw in variants:
            bad += run_single(Job(s, **kw), (cls, s.H, s.W, kw))
        # the descriptor's tuning fields are honoured (seen through the workspace the plan asks for: one slab per split)
        for th, tw in TILES:
            assert ntiles_of(s, TH=th, TW=tw) == s.N * (-(-s.oH // th)) * (-(-s.oW // tw)), (cls, s.H, s.W, th, tw)
        for k in (1, 2, 3, 7, nt, nt + 5):
            assert split_count(s, splitk=k) == -(-nt // -(-nt // min(k, nt))), (cls, s.H, s.W, k)
        # the block order (wg_decode): no full group of 8 splits, one full group plus a remainder of 4, one tile per split
        for kw in (dict(), dict(splitk=3), dict(splitk=12), dict(splitk=nt, cfg_tp=128)):
            bad += run_single(Job(s, **kw), (cls, s.H, s.W, kw, "block order"))
    assert not bad, bad[:20]


def test_block_order_groups_of_eight_plus_remainder():
    """12 splits on layers of 2 x 2 (cout, cin) tiles: 8 splits in whole groups of 8 block ids, the other r = 4 dealt pair by
    pair (the remainder decode of wg_decode)"""
    bad = []
    for s in (spec(3, 1, 128, 128, 3, 16, 32, seed=200), spec(3, 2, 64, 128, 3, 32, 64, seed=201)):
        for tp, splitk in ((64, 12), (128, 12)):
            assert split_count(s, splitk=splitk, cfg_tp=tp) == 12, (s, tp)
            bad += run_single(Job(s, splitk=splitk, cfg_tp=tp), (s.stride, tp))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------- (d) views and padding
def test_channel_slice_views_and_padded_channels():
    """x and dy as the upper channel slice of buffers twice as wide (NaN below), real channel counts below the pads"""
    bad = []
    cases = [spec(3, 1, 29, 61, 3, 13, 17, wide=True, seed=300), spec(3, 2, 29, 61, 3, 21, 27, wide=True, seed=301),
             spec(1, 1, 61, 61, 3, 13, 17, wide=True, seed=302),
             spec(3, 1, 12, 85, 2, 13, 17, seed=303), spec(3, 1, 12, 85, 2, 13, 17, wide=True, seed=304),     # Cin 12 of 16, Cout 85 of 96
             spec(1, 1, 128, 85, 2, 13, 17, seed=305), spec(1, 1, 128, 85, 2, 13, 17, wide=True, seed=306),   # the prediction convs
             spec(16, 1, 12, 64, 2, 9, 11, wide=True, seed=307)]
    for s in cases:
        for kw in (dict(), dict(cfg_tp=128), dict(splitk=3, cfg_ns=3)):
            bad += run_single(Job(s, **kw), (len(s.taps), s.stride, s.Cin, s.Cout, s.ldx, kw))
    assert not bad, bad


def test_deep_stem_nine_taps_on_sixteen_padded_channels():
    """modeling/resnet_vd.py _Stem0Fn: 9 taps, stride 1, on the space-to-depth image (Cin 12 of CinPad 16, ldx 16), Cout = CoutPad"""
    bad = []
    for H, W in ((24, 20), (11, 13)):
        s = spec(3, 1, 12, 32, 2, H, W, CinPad=16, seed=310 + H)
        for kw in (dict(), dict(cfg_tp=128), dict(splitk=5)):
            bad += run_single(Job(s, **kw), ("deep stem", H, W, kw))
    assert not bad, bad


def _iam_jobs(G=4, cin=32, cout=25, CoutPad=32, N=2, H=13, W=17):
    """modeling/sparseinst.py _GroupIamFn.backward: G groups read channel slices of ONE feature map (x + g * cin, ldx = G * cin)
    and of ONE out-gradient map (dy + g * CoutPad, ldy = G * CoutPad, Cout < CoutPad) and write slices of one gradient"""
    xbuf = dybuf = None
    gwall = torch.full((G * cout * cin * 9 + 2 * GW_GUARD,), SENT, device=DEV)
    jobs = []
    for g in range(G):
        s = Spec(tuple(R.square_taps(3)), 1, N, H, W, H, W, cin, cout, cin, CoutPad, G * cin, g * cin, G * CoutPad, g * CoutPad, 320 + g)
        xbuf, dybuf, x, dy = R.make_operands(N, H, W, H, W, cin, cout, cin, CoutPad, s.seed, s.ldx, s.x_off, s.ldy, s.dy_off, xbuf, dybuf)
        jobs.append((s, x, dy))
    assert not xbuf.isnan().any() and not dybuf.isnan().any()
    xd, dyd = xbuf.to(DEV), dybuf.to(DEV)
    out = []
    for g, (s, x, dy) in enumerate(jobs):
        ops = dict(xd=xd, dyd=dyd, ref=R.wgrad_reference(x, dy, list(s.taps), 1, cin, cout), bref=R.bias_reference(dy, cout))
        n = cout * cin * 9
        out.append(Job(s, gw=gwall[GW_GUARD + g * n:GW_GUARD + (g + 1) * n], ops=ops))
    return out, gwall


def _iam_guards_ok(gwall):
    h = gwall.cpu()
    return bool(torch.all(h[:GW_GUARD] == SENT) and torch.all(h[-GW_GUARD:] == SENT))


def test_grouped_iam_convolution_layout():
    """single launches per group, then the G jobs as one grouped launch (how WgradBatch flushes them)"""
    jobs, gwall = _iam_jobs()
    bad = []
    for g, j in enumerate(jobs):
        bad += run_single(j, ("iam single", g))
    assert _iam_guards_ok(gwall)
    jobs, gwall = _iam_jobs()
    b, _ = run_group(jobs, [("iam group", g) for g in range(len(jobs))], runs=2)
    bad += b
    assert _iam_guards_ok(gwall)
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------- (e) epilogues
EPI_SPECS = [spec(3, 1, 64, 64, 3, 13, 17, seed=400), spec(3, 2, 29, 64, 3, 21, 27, seed=401), spec(1, 1, 61, 64, 3, 13, 17, seed=402),
             spec(3, 1, 12, 32, 2, 13, 17, seed=403), spec(1, 1, 128, 128, 3, 13, 17, seed=404)]


def test_accumulate_and_row_scale():
    """gw += dW onto an integer g0, launched twice; a per-Cout factor of signed powers of two; both"""
    bad = []
    for s in EPI_SPECS:
        for kw in (dict(accumulate=1), dict(scaled=True), dict(accumulate=1, scaled=True), dict(accumulate=1, scaled=True, splitk=3, cfg_tp=128)):
            runs = 2 if kw.get("accumulate") else 1
            j = Job(s, **kw)
            bad += run_single(j, (len(s.taps), s.stride, kw), runs=runs)
            if runs == 2:
                assert not torch.equal(j.expected(1), j.expected(2))
    assert not bad, bad


def test_bias_gradient_exact_and_weight_gradient_unchanged():
    """gbias (Cout = CoutPad, as the callers use it) equals the column sums of dy exactly; gw still equals its reference"""
    bad = []
    for s in EPI_SPECS:
        assert s.Cout == s.CoutPad
        for kw in (dict(), dict(cfg_tp=128), dict(splitk=3), dict(TH=5, TW=7, splitk=4), dict(scaled=True, cfg_ns=3)):
            bad += run_single(Job(s, gbias=True, **kw), ("gbias", len(s.taps), s.stride, s.Cout, kw))
    assert not bad, bad


def test_bias_gradient_with_accumulate_is_refused_before_any_launch():
    s = EPI_SPECS[0]
    j = Job(s, gbias=True, accumulate=1)
    d = j.fill(L.mi_wgrad_desc())
    need = plan_bytes(j)
    ws = torch.full((need + WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    d.ws, d.ws_bytes = ws.data_ptr(), need
    assert L.lib().mi_conv2d_wgrad(C.byref(d), L.stream_ptr()) == MI_EINVAL
    torch.cuda.synchronize()
    assert bool((ws == 0xFF).all())                                             # nothing ran: no partial was written
    assert torch.equal(j.gw.cpu().view(j.shape), j.g0.float())                  # gw still holds g0
    assert bool(j.gbbuf[GW_GUARD:-GW_GUARD].isnan().all())
    descs = (L.mi_wgrad_desc * 1)()
    j.fill(descs[0])
    meta = L.mi_wgrad_group()
    assert L.lib().mi_conv2d_wgrad_group_plan(descs, 1, None, None, 0, C.byref(meta)) == MI_EINVAL


# ------------------------------------------------------------------------------------------------------- (f) grouped forms
def _group_jobs():
    """the jobs of (b) and a subset of (c): ragged, tiny (ONE pixel tile: fewer than the group's T >= 4) and single-row
    maps, descriptor overrides, accumulate and row_scale"""
    jobs, labels = matrix_b_jobs()
    for cls in GEO_CLASSES:
        sp = _geo_specs(cls)
        for s, kw in ((sp[1], dict()), (sp[2], dict()), (sp[3], dict(cfg_tp=128)), (sp[1], dict(splitk=7, cfg_ns=4)),
                      (sp[1], dict(TH=5, TW=7, accumulate=1, scaled=True)), (sp[5], dict(splitk=1 << 20))):
            jobs.append(Job(s, **kw))
            labels.append((cls, s.H, s.W, kw))
    return jobs, labels


@pytest.mark.parametrize("multi", ["0", "3"])
def test_grouped_launch_forms(monkeypatch, multi):
    """one grid per tile configuration and the mixed grid of the 1x1 layers (MI_WG_MULTI 3), two runs of the same table:
    every result equals the reference, not merely the other form"""
    monkeypatch.setenv("MI_WG_MULTI", multi)
    jobs, labels = _group_jobs()
    assert ntiles_of(_geo_specs("1x1")[2]) == 3          # (the 5 x 3 map: one tile per image)
    bad, meta = run_group(jobs, labels, runs=2)
    cfgs = group_cfgs(meta)
    if multi == "0":
        assert set(cfgs) == WG_ALL and len(cfgs) == 28
    else:
        assert {c for c in cfgs if c[0] == 1} == {(1, 0, 0, 2, 2, 64), (1, 0, 0, 2, 2, 128)}
        assert not any(c[0] == 9 and c[1] == 0 for c in cfgs)
    assert not bad, bad[:20]


def test_group_of_one_job_and_group_with_bias_gradients(monkeypatch):
    bad = []
    for s in (EPI_SPECS[0], EPI_SPECS[2]):
        b, meta = run_group([Job(s)], [("one job", len(s.taps))], runs=2)
        assert meta.ngroups == 1
        bad += b
    for multi in ("0", "3"):
        monkeypatch.setenv("MI_WG_MULTI", multi)
        jobs = [Job(s, gbias=(i != 1), **kw) for i, (s, kw) in enumerate(zip(EPI_SPECS, (dict(), dict(), dict(cfg_tp=128), dict(splitk=3), dict(scaled=True))))]
        b, _ = run_group(jobs, [("gbias group", i, "multi " + multi) for i in range(len(jobs))], runs=2)
        bad += b
    assert not bad, bad


# --------------------------------------------------------------------------- (g) overrides on the awkward maps, epilogues
def test_overrides_on_ragged_tiny_and_single_row_maps_and_epilogues():
    """beyond matrix (b): ragged, tiny and single-row maps with tile / split / ring overrides in both pixel-tile sizes, and the
    epilogue combinations of the split-K reduction"""
    bad = []
    for cls in GEO_CLASSES:
        sp = _geo_specs(cls)
        for s in (sp[1], sp[2], sp[3]):
            nt = ntiles_of(s)
            variants = [dict(TH=th, TW=tw, cfg_tp=tp) for th, tw in TILES for tp in (64, 128)]
            variants += [dict(splitk=3), dict(splitk=nt, cfg_ns=4), dict(splitk=2, cfg_ns=3, cfg_tp=128)]
            for kw in variants:
                bad += run_single(Job(s, **kw), (cls, s.H, s.W, kw))
    for s in EPI_SPECS:
        for kw in (dict(accumulate=1, scaled=True), dict(accumulate=1, splitk=5), dict(scaled=True, cfg_tp=128), dict(gbias=True, scaled=True)):
            bad += run_single(Job(s, **kw), ("epilogue", len(s.taps), s.stride, s.Cin, kw), runs=2 if kw.get("accumulate") else 1)
    assert not bad, bad[:20]


# --------------------------------------------------------------------------------------------------- (h) the check has teeth
def test_a_transposed_tap_table_does_not_pass():
    """a 3x3 layer run with tap_dy and tap_dx swapped (the same halo: nothing is read that the true table does not read):
    the result equals the reference of the transposed table and differs from the true one in every off-diagonal tap"""
    s = spec(3, 1, 29, 61, 3, 13, 17, seed=500)
    swapped = [(b, a) for a, b in s.taps]
    o = _ops(s)
    ref_t = R.wgrad_reference(o["x"], o["dy"], swapped, 1, s.Cin, s.Cout)
    for kw in (dict(), dict(cfg_tp=128, splitk=5)):
        j = Job(s, taps=swapped, **kw)
        assert run_single_raw(j) == 0
        got = j.buf.cpu()[GW_GUARD:-GW_GUARD].view(j.shape)
        assert torch.equal(got, _f32_exact(ref_t))
        true = _f32_exact(o["ref"])
        for t, (a, b) in enumerate(s.taps):
            assert torch.equal(got[:, :, t], true[:, :, t]) == (a == b), (t, a, b)
        assert [x[1][:2] for x in j.problems("true table")] == ["gw"]            # what the other tests would report


def run_single_raw(job):
    """launch without judging the result; returns the rc"""
    d = job.fill(L.mi_wgrad_desc())
    need = plan_bytes(job)
    ws = torch.full((need + WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    d.ws, d.ws_bytes = ws.data_ptr(), need
    rc = L.lib().mi_conv2d_wgrad(C.byref(d), L.stream_ptr())
    torch.cuda.synchronize()
    return rc
