"""GPU (-m gpu): the forward / data-gradient convolution family - the tile kernel (csrc/conv_igemm*), the streaming 1x1
(csrc/conv1x1_stream*), the weight-stationary 3x3 (csrc/conv3x3_ws*) and mi_pack_conv_weight - against the plain float64
reference of tests/conv_ref.py with NO tolerance, through the C ABI (mi_conv2d / mi_conv2d_plan / mi_conv2d_route /
mi_conv2d_group_plan / _run / mi_conv1x1_stream / mi_conv3x3_ws), on every route and in every instantiation.

The method (tests/conv_ref.py): the bf16 operands hold small integers, so every product and every fp32 partial sum is an exact
integer whatever the order of k-chunks, taps, waves or tiles, and any correct configuration equals the reference BIT FOR BIT.
The conditions - bf16 outputs (and the intermediate / final sums of the accumulate and add modes) are integers of magnitude
<= 256, fp32 outputs stay below 2^24, per channel sum |v| and sum v^2 over all stored pixels stay below 2^24 - are asserted on
the float64 reference of every case (Problem) before anything is launched.  test_premise_* checks them on the device;
test_mutation_* is the standing evidence that a one-tap, one-halo-row or one-grid-row error cannot pass, at shapes where the
tolerances of the other convolution tests would pass it.

Hygiene of every launch (Problem / Job): the output view sits in a buffer of sentinel words - guards before and after it, the
channels [Cout, ldy) and the lower slice of a wider buffer - that must survive; it is pre-filled with NaN unless the launch
accumulates or visits a sub-grid (then with integers that the unvisited pixels must still hold bit for bit); the input buffer
is NaN outside the descriptor's view and zero in the pad channels [Cin, K8 * 8); the packed weight image is written by
mi_pack_conv_weight into a guarded NaN buffer and compared, pad entries included, with the reference image; the statistics
buffer is guarded and its slots beyond stats_slots must stay untouched."""
import collections
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import conv_ref as R
from yolov7_d2_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -1536.0                 # sentinel (exact in bf16, fp32 and fp64)
GUARD = 64                     # guard elements around every buffer
ALL_SLOTS = L.MI_BN_SLOTS      # slots of a statistics buffer; a launch uses the first Mode.nslots of them
COUNT = collections.Counter()  # tile-kernel launches per instantiation (the child process reports them)
REFUSED = []                   # forced configurations mi_conv2d_plan refused: (KC, BN, TPIX, TPS, lds bytes of the mirror)
F = R                          # flag names: F.ACCUM ...

# ------------------------------------------------------------------------------------------------ the instantiation sets
# conv_launch_kc of csrc/conv_igemm_kernel.h, written out: nine tile forms (pixel tile, cout tile, waves) x four k-chunks x
# the taps-per-step class (compile-time 1 / run-time > 1) x three epilogues (EPI 0 plain / statistics, 1 accumulate / BNBWD,
# 2 the aux-tensor epilogues)
FORMS4 = [(128, 32, 4), (128, 64, 4), (128, 128, 4), (64, 32, 2), (64, 64, 4), (64, 128, 4)]
FORMS8 = [(128, 64, 8), (128, 128, 8), (64, 128, 8)]
TILE_ALL = {(kc, form, tps, epi) for kc in (16, 32, 64, 128) for form in FORMS4 + FORMS8 for tps in ("1", ">1") for epi in (0, 1, 2)}
assert len(TILE_ALL) == 216
# instantiations no descriptor can reach because their LDS need exceeds 160 KB - by name, with the arithmetic.  None: the
# hungriest class, KC 128 x BN 128 with several taps per step, is reached by the two-tap parity classes of a stride-2 data
# gradient with K = 128: one k-chunk, one step -> single buffers: 2 taps x 16 x 128 x 16 B = 64 KB of weights + a 5 x 32 halo x
# 256 B = 40 KB -> 104 KB (pixel tile 4 x 32), 64 KB + 9 x 8 x 256 B = 18 KB -> 82 KB (8 x 8).  FORCED configurations beyond the
# budget - 3x3 with KC 128, BN 128, TPS 3: 2 x 96 KB of slabs - are refused by mi_conv2d_plan with "conv: LDS n too large";
# run_tile accepts a refusal only when lds_mirror gives the same n > 160 KB, and the sets below are asserted complete.
TILE_UNREACHABLE = {}
# the 4-wave forms the 8-wave rule of mi_conv2d shadows for staged launches (bf16 output, Cout % 8 == 0)
SHADOWED = {(tp, bn, 4) for (tp, bn, _) in FORMS8}
# c1s_fill of csrc/conv1x1_stream.hip, written out: (K, waves over cout, pixel tile) with a kernel (c1s_valid: whole 8 KB
# per tile and a ring of 2 - 4 tiles within 160 KB)
C1S_ALL = ({(k, wm, 128) for k in (32, 64, 128, 256) for wm in (4, 2)} | {(k, 4, 64) for k in (64, 128, 256, 512)} |
           {(k, 1, 256) for k in (32, 64, 128)})
assert len(C1S_ALL) == 15


def _rup(a, b):
    return (a + b - 1) // b * b


def lds_mirror(npixh, Kp, ntaps, kc, bn, tps, tpix):
    """lds_need of conv_fill (csrc/conv_igemm.hip): halo image (doubled with several k-chunks) + weight slabs (doubled with
    several steps), at least the staged epilogue tile"""
    xb = -(-npixh // (64 // (kc // 8))) * 1024
    wb = tps * (kc // 8) * bn * 16
    nch = Kp // kc
    nst = nch * (ntaps // tps)
    return max(xb * (2 if nch > 1 else 1) + wb * (2 if nst > 1 else 1), tpix * (bn * 2 + 16), 16 * bn * 8)


# ------------------------------------------------------------------------------------------------------------- operands
Spec = collections.namedtuple("Spec", "kind k N H W Kr Kpad Cout CoutPad xlo xhi xmax wmax seed wseed")


def spec(kind, k, N, H, W, Kr, Cout, Kpad=None, CoutPad=None, xlo=0, xhi=0, xmax=1, wmax=1, seed=0, wseed=0):
    """kind 'fwd': x is a layer's input (Kr real of Kpad readable channels), the weight image its forward image; 'dgrad': x is
    a layer's out-gradient (Kr = the layer's Cout) and the image the data-gradient image (Cout = the layer's Cin).
    xlo / xhi: channels of a wider buffer below / above the view (NaN).  Specs that agree in everything but Cout / wseed share
    ONE input buffer (several convolutions of one input); wseed tells their weights apart."""
    return Spec(kind, k, N, H, W, Kr, Kpad or _rup(Kr, 16), Cout, CoutPad or _rup(Cout, 32), xlo, xhi, xmax, wmax, seed, wseed)


@functools.lru_cache(maxsize=None)
def _input(N, H, W, Kr, Kpad, xlo, xhi, xmax, seed):
    """(buffer, float64 content of the view's real channels): integers in the real channels, ZERO in the pad channels
    [Kr, Kpad), NaN everywhere else of the buffer"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-xmax, xmax + 1, (N, H, W, Kr), generator=g).double()
    xb = torch.full((N, H, W, xlo + Kpad + xhi), float("nan"), dtype=torch.bfloat16)
    xb[..., xlo:xlo + Kpad] = 0
    xb[..., xlo:xlo + Kr] = x.to(torch.bfloat16)
    return xb.to(DEV), x.to(DEV)


class Ops:
    """the operands of one Spec on the device (shared by every launch of it; never modified): the input buffer and the weight
    image mi_pack_conv_weight made - checked against the reference image, guards and pads included"""

    def __init__(self, s):
        self.s = s
        g = torch.Generator().manual_seed(50000 + 97 * s.seed + 7 * s.wseed + s.Cout)
        KK = s.k * s.k
        wshape = (s.Cout, s.Kr, s.k, s.k) if s.kind == "fwd" else (s.Kr, s.Cout, s.k, s.k)
        self.w = torch.randint(-s.wmax, s.wmax + 1, wshape, generator=g).double()          # the OIHW master
        self.ldx = s.xlo + s.Kpad + s.xhi
        self.xbuf, self.x64 = _input(s.N, s.H, s.W, s.Kr, s.Kpad, s.xlo, s.xhi, s.xmax, s.seed)
        self.slabs = (R.fwd_slabs(self.w) if s.kind == "fwd" else R.dgrad_slabs(self.w)).to(DEV)      # w[tap][co][ci]
        n = KK * s.Kpad * s.CoutPad
        self.wbuf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.bfloat16, device=DEV)
        self.wbuf[GUARD:GUARD + n] = float("nan")
        self.pack(n)

    def pack(self, n):
        """mi_pack_conv_weight into the guarded NaN buffer; the image must equal the reference image, zero pads included"""
        s = self.s
        wm = self.w.float().to(DEV)
        wp = self.wbuf.data_ptr() + 2 * GUARD
        if s.kind == "fwd":
            rc = L.lib().mi_pack_conv_weight(wm.data_ptr(), s.Cout, s.Kr, s.k, s.k, wp, s.Kpad, s.CoutPad, None, 0, 0, L.stream_ptr())
        else:
            rc = L.lib().mi_pack_conv_weight(wm.data_ptr(), s.Kr, s.Cout, s.k, s.k, None, 0, 0, wp, s.Kpad, s.CoutPad, L.stream_ptr())
        L.check(rc, "mi_pack_conv_weight")
        torch.cuda.synchronize()
        exp = torch.full_like(self.wbuf, SENT)
        exp[GUARD:GUARD + n] = R.packed_image(self.slabs, s.Kpad // 8, s.CoutPad).reshape(-1).to(torch.bfloat16)
        assert torch.equal(self.wbuf, exp), ("mi_pack_conv_weight: image, pad entries or guards differ", s)
        self.exp_w = exp

    @property
    def xptr(self):
        return self.xbuf.data_ptr() + 2 * self.s.xlo

    @property
    def wptr(self):
        return self.wbuf.data_ptr() + 2 * GUARD


@functools.lru_cache(maxsize=None)
def ops(s):
    return Ops(s)


# ------------------------------------------------------------------------------------------------------------- problems
Mode = collections.namedtuple("Mode", "name flags bias aux stats nslots")
PLAIN = Mode("plain", 0, False, False, False, 0)
STATS = Mode("stats", 0, False, False, True, 4)
ACCUM = Mode("accum", F.ACCUM, False, False, False, 0)
BIAS = Mode("bias", 0, True, False, False, 0)
RELU = Mode("relu", F.RELU, False, False, False, 0)
BIAS_RELU = Mode("bias_relu", F.RELU, True, False, False, 0)
ADDRELU = Mode("addrelu", F.ADDRELU, True, True, False, 0)
ADDRELU_NOBIAS = Mode("addrelu_nobias", F.ADDRELU, False, True, False, 0)
RELUMASK = Mode("relumask", F.RELUMASK, False, True, False, 0)
ACCUM_RELUMASK = Mode("accum_relumask", F.ACCUM | F.RELUMASK, False, True, False, 0)
BNBWD = Mode("bnbwd", F.BNBWD, False, True, True, 4)
ACCUM_BNBWD = Mode("accum_bnbwd", F.ACCUM | F.BNBWD, False, True, True, 4)
F32 = Mode("f32_bias", F.OUT_F32, True, False, False, 0)
F32_ACCUM = Mode("f32_bias_accum", F.OUT_F32 | F.ACCUM, True, False, False, 0)
F32_STATS = Mode("f32_stats", F.OUT_F32, False, False, True, 16)
Geo = collections.namedtuple("Geo", "taps in_stride out_stride oy ox gridH gridW outH outW")
OLD_MAX = 20                   # |old| of an accumulating launch / the pre-fill of a sub-grid launch


def geo_fwd(s, stride=1):
    oH, oW = R.conv_out(s.H, s.W, s.k, stride)
    return Geo(tuple(R.square_taps(s.k)), stride, 1, 0, 0, oH, oW, oH, oW)


def geo_dgrad(s):
    return Geo(tuple(R.dgrad_taps_s1(s.k)), 1, 1, 0, 0, s.H, s.W, s.H, s.W)


def geo_s2_classes(s, H, W):
    """the four parity-class launches of the stride-2 data gradient whose out-gradient is s (the input gradient is H x W)"""
    assert (s.H, s.W) == R.conv_out(H, W, 3, 2)
    return [Geo(tuple(t), 1, 2, py, px, gh, gw, H, W) for (t, py, px, gh, gw) in R.dgrad_s2_classes(H, W)]


class YLayout:
    """where the output view lies: ylo sentinel channels below it, the view's Cout channels, sentinel channels up to ldy;
    y_nstride elements between images (0: dense); `whole`: another problem's YLayout whose buffer this view shares"""

    def __init__(self, N, outH, outW, Cout, ldy, ylo=0, y_nstride=0, img_off=0):
        self.ldy, self.ylo, self.y_nstride, self.img_off = ldy, ylo, y_nstride, img_off
        self.nstride = y_nstride or outH * outW * ldy
        self.numel = N * self.nstride + 2 * GUARD
        n = torch.arange(N, device=DEV).view(N, 1, 1, 1) * self.nstride
        p = (torch.arange(outH, device=DEV).view(1, outH, 1, 1) * outW + torch.arange(outW, device=DEV).view(1, 1, outW, 1)) * ldy
        self.idx = GUARD + img_off + n + p + ylo + torch.arange(Cout, device=DEV).view(1, 1, 1, Cout)      # [N, outH, outW, Cout]
        assert int(self.idx.max()) < self.numel - GUARD


class Problem:
    """one convolution - operands, geometry, epilogue - with its pre-filled buffers and, from the float64 reference, its expected
    buffers.  The exactness conditions of the method are asserted here, before anything is launched."""

    def __init__(self, s, geo, mode=PLAIN, ylo=0, yhi=0, y_nstride=0, img_off=0, ldy=None, old=None, seed=0, ref_taps=None,
                 ref_grid=None):
        self.s, self.geo, self.mode, self.o = s, geo, mode, ops(s)
        N, Cout = s.N, s.Cout
        f32 = bool(mode.flags & F.OUT_F32)
        self.ydt = torch.float32 if f32 else torch.bfloat16
        ldy = ldy or (ylo + (Cout if f32 else s.CoutPad) + yhi)
        self.lay = YLayout(N, geo.outH, geo.outW, Cout, ldy, ylo, y_nstride, img_off)
        g = torch.Generator().manual_seed(7000 + 13 * s.seed + seed)
        shape = (N, geo.outH, geo.outW, Cout)
        sub = (geo.gridH, geo.gridW, geo.out_stride) != (geo.outH, geo.outW, 1)
        drawn = torch.randint(-OLD_MAX, OLD_MAX + 1, shape, generator=g).double()
        if old is None:
            old = drawn.to(DEV) if ((mode.flags & F.ACCUM) or sub) else torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
        self.old = old
        self.bias = torch.randint(-9, 10, (Cout,), generator=g).double().to(DEV) if mode.bias else None
        self.aux = self.mean = self.invstd = None
        if mode.aux:
            self.aux = torch.randint(-3, 4, shape, generator=g).double().to(DEV)
        if mode.flags & F.BNBWD:
            self.mean = torch.randint(-2, 3, (Cout,), generator=g).double().to(DEV)
            self.invstd = (2.0 ** torch.randint(-2, 2, (Cout,), generator=g).double()).to(DEV)
        gh, gw = ref_grid or (geo.gridH, geo.gridW)
        self.exp, self.exp_stats = R.conv_reference(
            self.o.x64, self.o.slabs, list(ref_taps or geo.taps), old, gh, gw, geo.in_stride, geo.out_stride, geo.oy, geo.ox,
            mode.flags, self.bias, self.aux, self.aux, self.mean, self.invstd, want_stats=mode.stats)
        # ---- the conditions of the method, on the reference
        R.assert_exact(self.exp, None, f32)
        if mode.flags & F.ACCUM:                       # the rounded first term and the sum (the sum is in self.exp)
            r0, _ = R.conv_reference(self.o.x64, self.o.slabs, list(ref_taps or geo.taps), old, gh, gw, geo.in_stride, geo.out_stride,
                                     geo.oy, geo.ox, mode.flags & F.OUT_F32, self.bias)
            R.assert_exact(r0, None, f32)
        if mode.flags & F.ADDRELU:                     # bf16(r + bias) and the sum with aux, before the ReLU hides a negative one
            r0, _ = R.conv_reference(self.o.x64, self.o.slabs, list(ref_taps or geo.taps), old, gh, gw, geo.in_stride, geo.out_stride,
                                     geo.oy, geo.ox, 0, self.bias)
            R.assert_exact(r0)
            R.assert_exact(r0 + self.aux)
        if mode.stats:
            ys = slice(geo.oy, geo.oy + (gh - 1) * geo.out_stride + 1, geo.out_stride)
            xs = slice(geo.ox, geo.ox + (gw - 1) * geo.out_stride + 1, geo.out_stride)
            v = self.exp[:, ys, xs]
            if mode.flags & F.BNBWD:                   # sums of multiples of 1 / 4 (invstd >= 2^-2): exact below 2^22
                R.assert_stats_premise(v, 4.0 * (self.aux[:, ys, xs] - self.mean) * self.invstd)
                assert bool((self.exp_stats * 4 == (self.exp_stats * 4).round()).all())
            else:
                R.assert_stats_premise(v)
                R.assert_exact(torch.zeros(1), self.exp_stats)
        # ---- buffers
        self.y0 = torch.full((self.lay.numel,), SENT, dtype=self.ydt, device=DEV)
        self.y0[self.lay.idx] = old.to(self.ydt)
        self.yexp = torch.full((self.lay.numel,), SENT, dtype=self.ydt, device=DEV)
        self.yexp[self.lay.idx] = self.exp.to(self.ydt)
        self.biasd = self.bias.float() if self.bias is not None else None
        self.auxbuf = None
        if mode.aux:                                   # the view in the upper half of a NaN buffer twice as wide
            self.ldaux = 2 * _rup(Cout, 8)
            self.auxbuf = torch.full(shape[:3] + (self.ldaux,), float("nan"), dtype=torch.bfloat16, device=DEV)
            self.auxbuf[..., self.ldaux // 2:self.ldaux // 2 + Cout] = self.aux.to(torch.bfloat16)
        if mode.flags & F.BNBWD:
            self.bnp = [torch.ones(Cout, device=DEV), torch.zeros(Cout, device=DEV), self.mean.float(), self.invstd.float()]
        self.st0 = self.stexp = None
        if mode.stats:
            n = ALL_SLOTS * s.CoutPad * 2
            self.st0 = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float64, device=DEV)
            self.st0[GUARD:GUARD + mode.nslots * s.CoutPad * 2] = 0
            self.stexp = torch.zeros(s.CoutPad, 2, dtype=torch.float64, device=DEV)
            self.stexp[:Cout] = self.exp_stats


@functools.lru_cache(maxsize=None)
def problem(s, geo, mode=PLAIN, ylo=0, yhi=0):
    return Problem(s, geo, mode, ylo, yhi)


class Job:
    """one descriptor: a Problem, a forced configuration and its own copies of the output / statistics buffers"""

    def __init__(self, prob, KC=0, BN=0, TH=0, TW=0, TPS=0, taps=None, gridH=None, ybuf=None):
        self.p, self.cfg = prob, dict(KC=KC, BN=BN, TH=TH, TW=TW, TPS=TPS)
        self.taps = tuple(taps) if taps else prob.geo.taps                    # the table handed to the kernel (mutation tests)
        self.gridH = prob.geo.gridH if gridH is None else gridH
        self.ybuf = prob.y0.clone() if ybuf is None else ybuf                # (ybuf: a buffer several jobs write, owned by the test)
        self.own_y = ybuf is None
        self.stbuf = prob.st0.clone() if prob.st0 is not None else None

    def fill(self, d):
        p, s, g = self.p, self.p.s, self.p.geo
        d.x, d.w = p.o.xptr, p.o.wptr
        d.y = self.ybuf.data_ptr() + self.ybuf.element_size() * (GUARD + p.lay.img_off + p.lay.ylo)
        d.ldx, d.ldy, d.y_nstride = p.o.ldx, p.lay.ldy, p.lay.y_nstride
        d.N, d.H, d.W, d.outH, d.outW, d.gridH, d.gridW = s.N, s.H, s.W, g.outH, g.outW, self.gridH, g.gridW
        d.in_stride, d.out_stride, d.out_oy, d.out_ox = g.in_stride, g.out_stride, g.oy, g.ox
        d.K8, d.Cout, d.CoutPad, d.ntaps = s.Kpad // 8, s.Cout, s.CoutPad, len(self.taps)
        for t, (a, b, w) in enumerate(self.taps):
            d.tap_dy[t], d.tap_dx[t], d.tap_w[t] = a, b, w
        d.flags = p.mode.flags
        for k, v in self.cfg.items():
            setattr(d, k, v)
        d.bias = p.biasd.data_ptr() if p.biasd is not None else None
        if p.auxbuf is not None:
            d.bn_y, d.bn_ldy = p.auxbuf.data_ptr() + p.ldaux, p.ldaux
        if p.mode.flags & F.BNBWD:
            d.bn_scale, d.bn_shift, d.bn_mean, d.bn_invstd = [t.data_ptr() for t in p.bnp]
            d.bn_act = 0
        if self.stbuf is not None:
            d.stats_acc, d.stats_slots = self.stbuf.data_ptr() + 8 * GUARD, p.mode.nslots
        return d

    def desc(self):
        return self.fill(L.mi_conv_desc())

    def problems(self, label):
        """what is wrong with the buffers after the launch (an empty list: nothing); the first differing (n, y, x, c)"""
        p, bad = self.p, []
        if self.own_y and not torch.equal(self.ybuf, p.yexp):
            got, exp = self.ybuf[p.lay.idx], p.yexp[p.lay.idx]
            ne = ~((got == exp) | (got.isnan() & exp.isnan()))
            if bool(ne.any()):
                first = torch.nonzero(ne)[0].tolist()
                bad.append((label, "y: %d of %d elements differ (%d NaN), first at (n, y, x, c) = %s: got %s, expected %s" % (
                    int(ne.sum()), ne.numel(), int(got.isnan().sum()), first, float(got[tuple(first)]), float(exp[tuple(first)]))))
            m = torch.ones_like(self.ybuf, dtype=torch.bool)
            m[p.lay.idx] = False
            if not torch.equal(self.ybuf[m], p.yexp[m]):
                bad.append((label, "sentinel words around / beside the output view were written"))
        if self.stbuf is not None:
            n = ALL_SLOTS * p.s.CoutPad * 2
            used = p.mode.nslots * p.s.CoutPad * 2
            if not (bool((self.stbuf[:GUARD] == SENT).all()) and bool((self.stbuf[GUARD + used:] == SENT).all())):
                bad.append((label, "statistics: the guards or the slots beyond stats_slots were written"))
            got = self.stbuf[GUARD:GUARD + used].view(p.mode.nslots, p.s.CoutPad, 2).sum(0)
            if not torch.equal(got, p.stexp):
                ne = torch.nonzero(got != p.stexp)
                c, k = ne[0].tolist()
                bad.append((label, "statistics: %d of %d sums differ, first channel %d [%d]: got %r, expected %r" % (
                    len(ne), got.numel(), c, k, float(got[c, k]), float(p.stexp[c, k]))))
        return bad


def view_problems(ybuf, probs, label):
    """a buffer several jobs wrote (channel slices / parity classes of one tensor): every view and everything outside them"""
    bad = []
    m = torch.ones_like(ybuf, dtype=torch.bool)
    exp = torch.full_like(ybuf, SENT)
    for p in probs:
        m[p.lay.idx] = False
    for i, p in enumerate(probs):
        e = p.exp.to(ybuf.dtype)
        got = ybuf[p.lay.idx]
        ne = ~((got == e) | (got.isnan() & e.isnan()))
        if bool(ne.any()):
            first = torch.nonzero(ne)[0].tolist()
            bad.append((label, i, "y: %d elements differ, first at (n, y, x, c) = %s: got %s, expected %s" % (
                int(ne.sum()), first, float(got[tuple(first)]), float(e[tuple(first)]))))
    if not torch.equal(ybuf[m], exp[m]):
        bad.append((label, "sentinel words outside the views were written"))
    return bad


# ------------------------------------------------------------------------------------------------------------- launches
class env:
    """environment switches the library reads per call"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


TILE_ONLY = dict(MI_CONV_STREAM="0", MI_CONV_WS="0")


def tile_instantiation(d, ntiles):
    """the kernel mi_conv2d launches for a planned descriptor: conv_launch_kc / launch_cfg and the 8-wave rule, mirrored"""
    tpix = 64 if d.TH * d.TW <= 64 else 128
    nblocks = ntiles * (d.CoutPad // d.BN)
    w8max = int(os.environ.get("MI_CONV_W8", 1 << 40))
    w8mask = int(os.environ.get("MI_CONV_W8MASK", 7))
    cls = {(128, 64): 1, (128, 128): 2, (64, 128): 4}.get((tpix, d.BN), 0)
    staged = not (d.flags & F.OUT_F32) and d.Cout % 8 == 0
    waves = 8 if (nblocks <= w8max and (cls & w8mask) and staged) else (2 if (tpix, d.BN) == (64, 32) else 4)
    epi = 2 if d.flags & (F.RELUMASK | F.ADDRELU) else (1 if d.flags & (F.ACCUM | F.BNBWD) else 0)
    return (d.KC, (tpix, d.BN, waves), "1" if d.TPS == 1 else ">1", epi), nblocks


def run_tile(job, label, may_refuse=False):
    """mi_conv2d on the tile kernel with the job's forced configuration, which mi_conv2d_plan must echo; returns the problems.
    may_refuse: a configuration the launcher refuses is recorded (REFUSED) when the mirror of its LDS arithmetic says why -
    any other refusal is a problem"""
    lib = L.lib()
    with env(**TILE_ONLY):
        d = job.desc()
        probe = L.mi_conv_desc.from_buffer_copy(d)
        nt = lib.mi_conv2d_plan(C.byref(probe))
        if nt < 0:
            g, s = job.p.geo, job.p.s
            dys, dxs = [t[0] for t in job.taps], [t[1] for t in job.taps]
            npixh = ((d.TH - 1) * g.in_stride + max(dys) - min(dys) + 1) * ((d.TW - 1) * g.in_stride + max(dxs) - min(dxs) + 1)
            tpix = 64 if d.TH * d.TW <= 64 else 128
            need = lds_mirror(npixh, s.Kpad, len(job.taps), d.KC, d.BN, d.TPS, tpix)
            msg = lib.mi_last_error().decode()
            if may_refuse and need > 160 * 1024 and msg.startswith("conv: LDS %d too large" % need):      # the launcher's own figure
                REFUSED.append((d.KC, d.BN, tpix, d.TPS, need))
                return []
            return [(label, "mi_conv2d_plan refused the configuration (the mirror of its LDS arithmetic says %d bytes): %s" % (need, msg))]
        assert lib.mi_conv2d_route(C.byref(d)) == 0
        for k, v in job.cfg.items():
            if v:
                assert getattr(probe, k) == v, (label, "mi_conv2d_plan does not echo the forced", k, v, getattr(probe, k))
        inst, nblocks = tile_instantiation(probe, nt)
        L.check(lib.mi_conv2d(C.byref(d), L.stream_ptr()), "mi_conv2d %s" % (label,))
    COUNT[inst] += 1
    # the XCD block remap of conv_fill (default MI_CONV_XMAP=2): launches with several cout tiles or several taps whose block
    # count is a multiple of 8
    COUNT["xmap on" if (nblocks % 8 == 0 and (d.CoutPad // probe.BN > 1 or d.ntaps > 1)) else "xmap off"] += 1
    return job.problems(label)


def run_auto(job, label, route):
    """mi_conv2d with nothing forced: mi_conv2d_route names the expected family and the result equals the same reference"""
    d = job.desc()
    got = L.lib().mi_conv2d_route(C.byref(d))
    if got != route:
        return [(label, "mi_conv2d_route says %d, expected %d" % (got, route))]
    L.check(L.lib().mi_conv2d(C.byref(d), L.stream_ptr()), "mi_conv2d (routed) %s" % (label,))
    return job.problems((label, "mi_conv2d"))


def run_group(jobs, label, kc=None):
    """mi_conv2d_group_plan / _run with a device table; returns (problems, meta).  kc: the expected meta.KC (-1 streaming,
    -2 weight-stationary, None: the tile kernel)"""
    lib = L.lib()
    descs = (L.mi_conv_desc * len(jobs))()
    for d, j in zip(descs, jobs):
        j.fill(d)
    meta = L.mi_conv_group()
    L.check(lib.mi_conv2d_group_plan(descs, len(jobs), None, 0, C.byref(meta)), "group plan (sizes) %s" % (label,))
    host = (C.c_char * int(meta.table_bytes))()
    L.check(lib.mi_conv2d_group_plan(descs, len(jobs), host, meta.table_bytes, C.byref(meta)), "group plan")
    if (kc is None) != (meta.KC > 0) or (kc is not None and meta.KC != kc):
        return [(label, "the group runs on family KC = %d, expected %s" % (meta.KC, kc))], meta
    table = torch.frombuffer(bytearray(bytes(host)[:int(meta.table_bytes)]), dtype=torch.uint8).to(DEV)
    L.check(lib.mi_conv2d_group_run(C.byref(meta), table.data_ptr(), L.stream_ptr()), "group run %s" % (label,))
    torch.cuda.synchronize()
    bad = []
    for i, j in enumerate(jobs):
        bad += j.problems((label, "group job %d" % i))
    return bad, meta


def run_entry(entry, jobs, label):
    """the explicit entries mi_conv1x1_stream / mi_conv3x3_ws (they fail instead of falling back)"""
    descs = (L.mi_conv_desc * len(jobs))()
    for d, j in zip(descs, jobs):
        j.fill(d)
    L.check(getattr(L.lib(), entry)(descs, len(jobs), L.stream_ptr()), "%s %s" % (entry, label))
    bad = []
    for i, j in enumerate(jobs):
        bad += j.problems((label, entry, i))
    return bad


# -------------------------------------------------------------------------------------------------------- (8) the premise
def test_premise_integer_bf16_round_trip_and_mfma():
    """every integer of magnitude <= 256 survives bf16 on the device; 257 does not (the bound is sharp); the matrix cores sum
    integer products exactly"""
    v = torch.arange(-256, 257, dtype=torch.float64)
    d = v.to(DEV).to(torch.bfloat16)
    assert torch.equal(d.double().cpu(), v) and float(torch.tensor(257.0).to(DEV).to(torch.bfloat16)) != 257.0
    g = torch.Generator().manual_seed(0)
    a = torch.randint(-3, 4, (32, 16), generator=g)
    b = torch.randint(-3, 4, (16, 32), generator=g)
    out = torch.full((32, 32), float("nan"), device=DEV)
    ad, bd = a.to(DEV, torch.bfloat16), b.to(DEV, torch.bfloat16)
    L.check(L.lib().mi_probe_mfma32(ad.data_ptr(), bd.data_ptr(), out.data_ptr(), L.stream_ptr()), "mi_probe_mfma32")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().double(), (a @ b).double())


def test_premise_bounds_hold_for_the_stored_values():
    """the bounds a Problem asserts on its reference hold for what the kernel stored: integers within the bf16 range, and the
    fp32 partial sums of the statistics - taken here from the STORED tensor - below 2^24"""
    s = spec("fwd", 3, 2, 20, 20, 64, 64, seed=1)
    j = Job(problem(s, geo_fwd(s), STATS))
    assert run_tile(j, "premise") == []
    v = j.ybuf[j.p.lay.idx].double()
    assert bool((v == v.round()).all()) and float(v.abs().max()) <= R.BF16_INT_MAX
    assert float(v.abs().reshape(-1, 64).sum(0).max()) < R.F32_INT_MAX and float((v * v).reshape(-1, 64).sum(0).max()) < R.F32_INT_MAX
    assert torch.equal(j.p.o.xbuf[..., :64].double(), j.p.o.x64)          # the operand the device holds is the integer tensor


# ------------------------------------------------------------------------------------- (1) tile kernel, every instantiation
TILES = [(8, 16), (4, 32), (8, 8), (3, 20)]       # two 128-pixel and two 64-pixel tiles


def _s2_dgrad_spec(N, H, W, Kr, Cout, seed, **kw):
    oH, oW = R.conv_out(H, W, 3, 2)
    return spec("dgrad", 3, N, oH, oW, Kr, Cout, seed=seed, **kw)


@functools.lru_cache(maxsize=None)
def tile_matrix():
    """(name, spec, [geometries], [modes]): the smallest shapes that reach the edges - ragged tiles in both directions, odd
    stride-2 maps, four k-chunks x four cout tiles, the stem's 12 of 16 channels, block counts that are and are not multiples
    of 8 (the xmap remap on / off; counted in COUNT)"""
    out = []
    for i, (N, H, W) in enumerate(((1, 13, 17), (2, 20, 20))):
        s = spec("fwd", 3, N, H, W, 64, 64, seed=100 + i)
        out.append(("3x3 s1 64 -> 64 %dx%dx%d" % (N, H, W), s, [geo_fwd(s)], [PLAIN, STATS, ACCUM, ADDRELU]))
    for i, (N, H, W) in enumerate(((2, 22, 14), (1, 9, 7))):
        s = spec("fwd", 3, N, H, W, 32, 64, xmax=2, seed=110 + i)
        out.append(("3x3 s2 32 -> 64 %dx%dx%d" % (N, H, W), s, [geo_fwd(s, 2)], [PLAIN, STATS, ACCUM, ADDRELU]))
    s = spec("fwd", 1, 2, 8, 8, 256, 512, seed=120)
    out.append(("1x1 256 -> 512 2x8x8", s, [geo_fwd(s)], [PLAIN, STATS, ACCUM, ADDRELU]))
    s = spec("fwd", 3, 2, 11, 13, 12, 32, Kpad=16, xmax=3, wmax=2, seed=121)
    out.append(("3x3 s1 stem 12 of 16 -> 32", s, [geo_fwd(s)], [PLAIN, STATS, ACCUM, ADDRELU]))
    # data gradients: 3x3 stride 1 (128 -> 128: every cout tile with several taps per step) and the four parity classes of a
    # stride-2 layer (1, 2, 2 and 4 taps, out_stride 2: sub-grids of an odd x odd map)
    s = spec("dgrad", 3, 1, 13, 17, 128, 128, seed=122)
    out.append(("3x3 s1 dgrad 128 -> 128 1x13x17", s, [geo_dgrad(s)], [PLAIN, STATS, ACCUM, RELUMASK, BNBWD]))
    s = _s2_dgrad_spec(1, 13, 17, 128, 128, 123)
    out.append(("3x3 s2 dgrad classes 128 -> 128 1x13x17", s, geo_s2_classes(s, 13, 17), [PLAIN, STATS, ACCUM, RELUMASK]))
    # direct epilogue (fp32 / ragged Cout): the in-process way to the 4-wave forms the 8-wave rule shadows
    s = spec("fwd", 1, 2, 8, 9, 128, 80, CoutPad=128, seed=124)
    out.append(("1x1 128 -> 80 of 128 fp32", s, [geo_fwd(s)], [F32, F32_ACCUM, F32_STATS]))
    s = spec("fwd", 3, 1, 9, 11, 64, 61, CoutPad=128, seed=125)
    out.append(("3x3 64 -> 61 of 128 ragged bf16", s, [geo_fwd(s)], [BIAS, STATS, ACCUM]))
    return out


def tile_matrix_jobs(kcs, only_shadowed=False):
    for name, s, geos, modes in tile_matrix():
        for gi, geo in enumerate(geos):
            nt = len(geo.taps)
            for kc in kcs:
                if s.Kpad % kc:
                    continue
                for bn in (32, 64, 128):
                    if s.CoutPad % bn:
                        continue
                    for (th, tw) in (TILES if len(geos) == 1 else TILES[1:3]):
                        tpix = 64 if th * tw <= 64 else 128
                        if only_shadowed and (tpix, bn, 4) not in SHADOWED:
                            continue
                        for tps in [t for t in (1, 2, 3, 4, 9) if nt % t == 0]:
                            for mode in modes:
                                yield (name, gi, kc, bn, th, tw, tps, mode.name), Job(problem(s, geo, mode, 32, 0), kc, bn, th, tw, tps)


def run_tile_matrix(kcs, only_shadowed=False):
    bad = []
    for label, job in tile_matrix_jobs(kcs, only_shadowed):
        bad += run_tile(job, label, may_refuse=True)
    torch.cuda.synchronize()
    return bad


def seen_instantiations():
    return {k for k in COUNT if isinstance(k, tuple)}


@pytest.mark.parametrize("kc", [16, 32, 64, 128])
def test_tile_kernel_every_instantiation(kc):
    """every instantiation of this k-chunk that a process with the default switches launches for staged outputs - the six
    unshadowed 4-wave forms and the three 8-wave forms, both taps classes, three epilogues - and, through the direct epilogue
    (fp32 output, ragged Cout), the three shadowed 4-wave forms; test_tile_kernel_four_wave_forms_in_a_child runs those in
    every k-chunk, taps class and epilogue."""
    COUNT.clear()
    del REFUSED[:]
    bad = run_tile_matrix([kc])
    assert not bad, bad[:20]
    want = {i for i in TILE_ALL if i[0] == kc and i not in TILE_UNREACHABLE}
    here = {i for i in want if i[1] not in SHADOWED}
    seen = seen_instantiations()
    assert seen <= want and here <= seen, (sorted(here - seen), sorted(seen - want))
    assert {i[1] for i in seen if i[1] in SHADOWED} == SHADOWED          # (the direct epilogue reaches the shadowed forms)
    assert COUNT["xmap on"] > 0 and COUNT["xmap off"] > 0
    # every refusal was the LDS budget (run_tile checked the arithmetic); none of them leaves an instantiation unreached
    assert all(r[4] > 160 * 1024 for r in REFUSED)


def test_tile_kernel_four_wave_forms_in_a_child():
    """MI_CONV_W8 is read once per process: with MI_CONV_W8=0 a fresh process (tests/conv_exact_gpu_child.py) runs the matrix
    rows whose (pixel tile, cout tile) the 8-wave rule shadows - every k-chunk, taps class and epilogue of the three 4-wave
    forms, staged.  A child that ends abnormally ends the test: nothing further is started on the GPU."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_exact_gpu_child.py")
    e = {k: v for k, v in os.environ.items() if not k.startswith("MI_CONV_")}
    e["MI_CONV_W8"] = "0"
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=240, env=e)
    assert r.returncode == 0, (r.returncode, (r.stdout + r.stderr)[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["env"] == {"MI_CONV_W8": "0"} and res["bad"] == [], res["bad"][:10]
    seen = {(kc, tuple(form), tps, epi) for kc, form, tps, epi in res["seen"]}
    want = {i for i in TILE_ALL if i[1] in SHADOWED and i not in TILE_UNREACHABLE}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
    assert res["launches"] >= len(want)


def test_instantiation_sets_are_complete():
    """the two processes together: TILE_ALL minus the list of unreachable instantiations, from the matrix itself (the same
    enumeration the launches above walk, planned but not launched)"""
    seen = set()
    lib = L.lib()
    for w8 in (None, "0"):
        for label, job in tile_matrix_jobs([16, 32, 64, 128], only_shadowed=(w8 == "0")):
            with env(**(dict(TILE_ONLY, MI_CONV_W8=w8) if w8 else TILE_ONLY)):
                probe = job.desc()
                nt = lib.mi_conv2d_plan(C.byref(probe))
                if nt >= 0:
                    seen.add(tile_instantiation(probe, nt)[0])
    assert seen == TILE_ALL - set(TILE_UNREACHABLE), (sorted(TILE_ALL - seen), sorted(seen - TILE_ALL))


# ------------------------------------------------------------------------------------------- (2) epilogues, tile kernel
def test_tile_epilogues():
    """fp32 bias, ReLU, add + ReLU with and without bias, the ReLU mask, accumulate + mask - forward 1x1 / 3x3 and data-gradient
    tap orders, ragged tiles, launcher-chosen and forced configurations"""
    bad = []
    s1 = spec("fwd", 3, 2, 13, 17, 64, 64, seed=200)
    s2 = spec("fwd", 1, 2, 13, 17, 64, 128, xmax=2, seed=201)
    s3 = spec("dgrad", 3, 2, 13, 17, 64, 32, seed=202)
    for s, geo in ((s1, geo_fwd(s1)), (s2, geo_fwd(s2)), (s3, geo_dgrad(s3))):
        for mode in (BIAS, RELU, BIAS_RELU, ADDRELU, ADDRELU_NOBIAS, RELUMASK, ACCUM_RELUMASK):
            for cfg in (dict(), dict(KC=32, BN=32, TH=3, TW=20, TPS=1), dict(KC=16, BN=32, TH=8, TW=16)):
                bad += run_tile(Job(problem(s, geo, mode, 32, 0), **cfg), (s.kind, s.k, mode.name, cfg))
    assert not bad, bad[:20]


def test_tile_fp32_outputs_into_channel_offsets_of_one_tensor():
    """MI_CONV_OUT_F32 with bias at Cout 1 / 4 / 80 written into channel offsets 4 / 0 / 5 of ONE 85-wide fp32 tensor (the
    prediction maps: the direct epilogue with ragged Cout), dense and with y_nstride (the map as anchors [a0, a0 + HW) of a
    longer [B][A][85] tensor), plain and accumulating; everything beside the three views keeps its sentinel"""
    bad = []
    N, H, W = 2, 9, 11
    for nstride, img_off in ((0, 0), ((H * W + 37) * 85, 20 * 85)):
        for mode in (F32, F32_ACCUM):
            probs = []
            for i, (cout, c0) in enumerate(((4, 0), (1, 4), (80, 5))):
                s = spec("fwd", 1, N, H, W, 128, cout, seed=210 + i)
                probs.append(Problem(s, geo_fwd(s), mode, ylo=c0, ldy=85, y_nstride=nstride, img_off=img_off))
            ybuf = torch.full((probs[0].lay.numel,), SENT, dtype=torch.float32, device=DEV)
            for p in probs:
                ybuf[p.lay.idx] = p.old.float()
            for p in probs:
                for cfg in (dict(),):
                    bad += run_tile(Job(p, ybuf=ybuf, **cfg), ("f32", p.s.Cout, mode.name, nstride))
            bad += view_problems(ybuf, probs, ("f32 85-wide", mode.name, nstride))
    # the same views in forced configurations (each on its own buffer)
    s = spec("fwd", 1, N, H, W, 128, 80, seed=212)
    for cfg in (dict(KC=32, BN=32, TH=8, TW=8), dict(KC=128, BN=32, TH=4, TW=32), dict(KC=64, BN=32, TH=3, TW=20)):
        bad += run_tile(Job(Problem(s, geo_fwd(s), F32_ACCUM, ylo=5, ldy=85), **cfg), ("f32 forced", cfg))
    assert not bad, bad[:20]


def test_tile_bn_backward_sums_exact():
    """MI_CONV_BNBWD with bn_act = 0, integer bn_y / bn_mean and bn_invstd a power of two: (sum dz, sum dz * xhat) exactly - on a
    stride-1 data gradient, and on the four parity launches of a stride-2 data gradient, which together give ONE set of sums"""
    bad = []
    s = spec("dgrad", 3, 2, 13, 17, 64, 64, seed=220)
    for mode in (BNBWD, ACCUM_BNBWD):
        for cfg in (dict(), dict(KC=32, BN=32, TH=3, TW=20, TPS=3), dict(KC=64, BN=64, TH=8, TW=16, TPS=1)):
            bad += run_tile(Job(problem(s, geo_dgrad(s), mode, 32, 0), **cfg), ("bnbwd s1", mode.name, cfg))
    for (H, W) in ((13, 17), (12, 17)):
        s = _s2_dgrad_spec(2, H, W, 64, 64, 221 + H)
        geos = geo_s2_classes(s, H, W)
        whole = Problem(s, geos[0], BNBWD, ylo=32)                            # (for the layout, the aux tensors and the buffers)
        ybuf = torch.full((whole.lay.numel,), SENT, dtype=torch.bfloat16, device=DEV)
        ybuf[whole.lay.idx] = float("nan")
        stbuf = whole.st0.clone()
        exp = torch.full_like(whole.exp, float("nan"))
        total = torch.zeros_like(whole.stexp)
        jobs = []
        for geo in geos:
            p = Problem(s, geo, BNBWD, ylo=32, old=exp)
            assert torch.equal(p.aux, whole.aux) and torch.equal(p.mean, whole.mean)       # one bn_y / mean / invstd for all four
            exp = p.exp
            total[:s.Cout] += p.exp_stats
            j = Job(p, ybuf=ybuf)
            j.stbuf = stbuf
            jobs.append(j)
        with env(**TILE_ONLY):
            for j in jobs:
                L.check(L.lib().mi_conv2d(C.byref(j.desc()), L.stream_ptr()), "mi_conv2d (parity class)")
        torch.cuda.synchronize()
        assert not exp.isnan().any()
        got = ybuf[whole.lay.idx]
        if not torch.equal(got, exp.to(torch.bfloat16)):
            bad.append(("bnbwd s2 %dx%d" % (H, W), "dx differs, first at %s" % torch.nonzero(got != exp.to(torch.bfloat16))[0].tolist()))
        used = BNBWD.nslots * s.CoutPad * 2
        sums = stbuf[GUARD:GUARD + used].view(BNBWD.nslots, s.CoutPad, 2).sum(0)
        if not torch.equal(sums, total):
            bad.append(("bnbwd s2 %dx%d" % (H, W), "the sums of the four launches differ from one set of sums", sums[:4].tolist(), total[:4].tolist()))
        if not (bool((stbuf[:GUARD] == SENT).all()) and bool((stbuf[GUARD + used:] == SENT).all())):
            bad.append(("bnbwd s2", "guards / unused slots written"))
    assert not bad, bad[:20]


# ------------------------------------------------------------------------- (3) stride-2 data gradient as the plan builds it
def _plan_s2(N, H, W, Cin, Cout, accumulate):
    """a one-layer plan (3x3 stride 2) whose input is the upper channel slice of a buffer twice as wide; with `accumulate` a
    second consumer of the same input comes first in the backward pass, so the layer's four launches carry MI_CONV_ACCUM"""
    from yolov7_d2_amd.plan import PlanBuilder
    b = PlanBuilder(DEV, training=True)
    big = b.new_act(N, H, W, 2 * Cin, "xbig")
    x = big.slice(Cin, 2 * Cin)
    g = torch.Generator().manual_seed(300 + H + W)
    keep = []
    mk = lambda co: keep.append(dict(gamma=torch.ones(co, device=DEV), beta=torch.zeros(co, device=DEV), rm=torch.zeros(co, device=DEV),
                         rv=torch.ones(co, device=DEV), nbt=torch.zeros((), dtype=torch.long, device=DEV), eps=1e-3, momentum=0.03,
                         ggamma=torch.zeros(co, device=DEV), gbeta=torch.zeros(co, device=DEV))) or keep[-1]
    w = torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=g).float().to(DEV)
    wg = torch.zeros_like(w)
    keep += [w, wg]
    outs = [b.base_conv("c", x, w, mk(Cout), 3, 2, wg)]
    if accumulate:
        w2 = torch.zeros(Cout, Cin, 1, 1, device=DEV)
        wg2 = torch.zeros_like(w2)
        keep += [w2, wg2]
        outs.append(b.base_conv("late", x, w2, mk(Cout), 1, 1, wg2))
    for o in outs:
        assert b.grad_mode(o) == 0
    plan = b.finalize()
    plan._keep = keep
    return plan, w, x


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
def test_stride2_data_gradient_as_the_plan_builds_it(accumulate):
    """the four dgrad{py}{px} descriptors of a PlanBuilder plan on integer operands, as four single launches and as the plan's
    ONE grouped launch (_group_parity), the whole dx against the scatter-form reference: odd x odd, odd x even and even x odd
    maps, dx a channel slice of a wider buffer whose other half must keep its pre-fill"""
    bad = []
    for (H, W) in ((13, 17), (13, 16), (12, 17)):
        N, Cin, Cout = 2, 32, 64
        plan, w, x = _plan_s2(N, H, W, Cin, Cout, accumulate)
        plan.run("fwd")                                                   # packs the weight images (the prologue)
        torch.cuda.synchronize()
        groups = [(k, ds) for k, ds in enumerate(plan.cmd_descs["bwd"]) if isinstance(ds, list) and plan.bwd_tags[k] == "c.dgrad(4 classes)"]
        assert len(groups) == 1, plan.bwd_tags
        k, descs = groups[0]
        assert sorted((d.out_oy, d.out_ox) for d in descs) == [(0, 0), (0, 1), (1, 0), (1, 1)]
        assert all(bool(d.flags & L.MI_CONV_ACCUM) == accumulate and d.out_stride == 2 and d.ldy == 2 * Cin for d in descs)
        d0 = descs[0]
        oH, oW = R.conv_out(H, W, 3, 2)
        assert (d0.H, d0.W, d0.outH, d0.outW, d0.K8 * 8, d0.Cout) == (oH, oW, H, W, Cout, Cin)
        base = plan.arena.data_ptr()
        arena = plan.arena
        dyv = arena[d0.x - base: d0.x - base + N * oH * oW * d0.ldx * 2].view(torch.bfloat16).view(N, oH, oW, d0.ldx)
        ylo = Cin                                                         # x is the upper slice: dx starts Cin channels into the buffer
        dxv = arena[d0.y - 2 * ylo - base: d0.y - 2 * ylo - base + N * H * W * d0.ldy * 2].view(torch.bfloat16).view(N, H, W, d0.ldy)
        g = torch.Generator().manual_seed(310 + H + W)
        dy = torch.randint(-2, 3, (N, oH, oW, Cout), generator=g).double()
        ref = R.dgrad_scatter(dy, w.cpu().double(), 2, H, W)
        pre = torch.randint(-OLD_MAX, OLD_MAX + 1, (N, H, W, 2 * Cin), generator=g).double()
        exp = pre.clone()
        exp[..., ylo:] = (ref + pre[..., ylo:]) if accumulate else ref
        R.assert_exact(ref)
        R.assert_exact(exp)
        meta_ptr, table_ptr = plan.bwd_cmds[0][k].p[0], plan.bwd_cmds[0][k].p[1]

        def fill():
            dyv.fill_(float("nan"))
            dyv[..., :Cout] = dy.to(DEV, torch.bfloat16)
            dxv.copy_(pre.to(DEV, torch.bfloat16))
            if not accumulate:
                dxv[..., ylo:] = float("nan")

        for form in ("four single launches", "the plan's grouped launch"):
            fill()
            if form.startswith("four"):
                for d in descs:
                    L.check(L.lib().mi_conv2d(C.byref(d), L.stream_ptr()), "mi_conv2d %d%d" % (d.out_oy, d.out_ox))
            else:
                L.check(L.lib().mi_conv2d_group_run(C.cast(meta_ptr, C.POINTER(L.mi_conv_group)), table_ptr, L.stream_ptr()), "group run")
            torch.cuda.synchronize()
            got = dxv.double().cpu()
            if not torch.equal(got, exp):
                ne = ~((got == exp) | (got.isnan() & exp.isnan()))
                bad.append(((H, W), form, "%d elements differ, first at (n, y, x, c) = %s" % (int(ne.sum()), torch.nonzero(ne)[0].tolist())))
    assert not bad, bad[:20]


# ------------------------------------------------------------------------------------------------ (4) grouped tile launches
@pytest.mark.parametrize("mode", [PLAIN, STATS, ACCUM], ids=lambda m: m.name)
def test_grouped_tile_launch_three_maps(mode):
    """three jobs of different maps in ONE launch through a device table: the smaller two run on the configuration the largest
    forces.  3x3 (K 64 -> 64 is weight-stationary territory: the tile route is forced) and 1x1 with ragged pixel counts"""
    bad = []
    for k, Kr, Cout in ((3, 64, 64), (1, 128, 96), (3, 32, 64)):
        jobs = []
        for i, (N, H, W) in enumerate(((2, 20, 20), (2, 10, 10), (1, 5, 7))):
            s = spec("fwd", k, N, H, W, Kr, Cout, seed=400 + 10 * k + i)
            jobs.append(Job(problem(s, geo_fwd(s), mode, 32, 0)))
        with env(**TILE_ONLY):
            b, meta = run_group(jobs, ("group", k, Kr, mode.name))
        assert meta.njobs == 3 and meta.EPI == (1 if mode is ACCUM else 0)
        bad += b
    assert not bad, bad[:20]


# ----------------------------------------------------------------------------------------------------- (5) streaming 1x1
C1Case = collections.namedtuple("C1Case", "name N H W K couts xlo ylo modes form")
C1_BASIC = (PLAIN, STATS, ACCUM)
C1_EPI = (BIAS, RELU, BIAS_RELU, ADDRELU, ADDRELU_NOBIAS, RELUMASK, ACCUM_RELUMASK)      # MODE 4, 4, 4, 5, 5, 5, 6


def _c1_cases():
    out = []
    for K in (64, 128, 256):                       # WM 4 on 128-pixel tiles: enough tiles that the chip is not "small"
        out.append(C1Case("K%d WM4 t128" % K, 1, 128, 128, K, (512,), 0, 0, C1_BASIC + C1_EPI[2:], (K, 4, 128)))
    out.append(C1Case("K32 WM4 t128", 2, 16, 16, 32, (128,), 0, 0, C1_BASIC + C1_EPI, (32, 4, 128)))
    for K in (64, 128, 256, 512):
        out.append(C1Case("K%d WM4 t64" % K, 2, 16, 16, K, (128,), 0, 0, C1_BASIC + C1_EPI, (K, 4, 64)))
    for K in (32, 64, 128, 256):
        out.append(C1Case("K%d WM2 t128" % K, 2, 16, 16, K, (64,), 0, 0, C1_BASIC + C1_EPI, (K, 2, 128)))
    for K in (32, 64, 128):
        out.append(C1Case("K%d WM1 t256" % K, 2, 16, 16, K, (96,), 0, 0, C1_BASIC + C1_EPI, (K, 1, 256)))
    out.append(C1Case("two convolutions of one input", 2, 16, 16, 128, (64, 64), 0, 0, C1_BASIC + C1_EPI, (128, 4, 64)))
    out.append(C1Case("Cout 1024: two launches of 512", 2, 16, 16, 64, (1024,), 0, 0, (PLAIN, ACCUM) + C1_EPI, None))
    out.append(C1Case("ragged last tile 1x97x101", 1, 97, 101, 64, (64,), 0, 0, (PLAIN, ACCUM) + C1_EPI, (64, 2, 128)))
    out.append(C1Case("more tiles than blocks", 3, 160, 160, 64, (64,), 0, 0, C1_BASIC + C1_EPI[2:], (64, 2, 128)))
    out.append(C1Case("slice views on both sides", 2, 16, 16, 128, (128,), 128, 64, C1_BASIC + C1_EPI, (128, 4, 64)))
    return out


C1_CASES = _c1_cases()


def _c1_jobs(c, mode):
    jobs = []
    for i, co in enumerate(c.couts):
        s = spec("fwd", 1, c.N, c.H, c.W, c.K, co, Kpad=c.K, CoutPad=co, xlo=c.xlo, seed=500, wseed=i)
        jobs.append(Job(problem(s, geo_fwd(s), mode, c.ylo, 0)))
    return jobs


def _c1_form(meta):
    wm = meta.BN // 32
    return (int(meta.priv[0] & 0xFFFFFFFF), wm, 256 if wm == 1 else (64 if (wm == 4 and meta.TPIX == 1) else 128))


@pytest.mark.parametrize("c", C1_CASES, ids=lambda c: c.name.replace(" ", "_"))
def test_streaming_1x1(c):
    """every case on the explicit entry, then (7) routed: mi_conv2d for one descriptor and mi_conv2d_group_plan with nothing
    forced must take the streaming kernel (mi_conv2d_route 1 / meta.KC -1) and give the same reference"""
    bad = []
    for mode in c.modes:
        bad += run_entry("mi_conv1x1_stream", _c1_jobs(c, mode), (c.name, mode.name))
        jobs = _c1_jobs(c, mode)
        if len(jobs) == 1:
            bad += run_auto(jobs[0], (c.name, mode.name), 1)
        if c.form is not None:
            b, meta = run_group(_c1_jobs(c, mode), (c.name, mode.name), kc=-1)
            bad += b
            if not b:
                assert _c1_form(meta) == c.form, (c.name, mode.name, _c1_form(meta))
                COUNT[("c1s",) + c.form] += 1
    torch.cuda.synchronize()
    assert not bad, bad[:20]


def test_streaming_1x1_forms_complete_and_ragged_statistics_stay_on_the_tile_kernel():
    """the forms the cases above name are all of C1S_ALL (planned here, so the test stands alone); a statistics launch over a
    ragged map is not served by the streaming kernel: mi_conv2d runs the tile kernel, and exactly"""
    seen = set()
    for c in C1_CASES:
        if c.form is None:
            continue
        jobs = _c1_jobs(c, PLAIN)
        descs = (L.mi_conv_desc * len(jobs))()
        for d, j in zip(descs, jobs):
            j.fill(d)
        meta = L.mi_conv_group()
        L.check(L.lib().mi_conv2d_group_plan(descs, len(jobs), None, 0, C.byref(meta)), "group plan")
        assert meta.KC == -1 and _c1_form(meta) == c.form, (c.name, meta.KC, _c1_form(meta))
        seen.add(c.form)
    assert seen == C1S_ALL, (sorted(C1S_ALL - seen), sorted(seen - C1S_ALL))
    c = [c for c in C1_CASES if c.name.startswith("ragged")][0]
    bad = run_auto(_c1_jobs(c, STATS)[0], "ragged statistics", 0)
    torch.cuda.synchronize()
    assert not bad, bad


# -------------------------------------------------------------------------------------------- (6) weight-stationary 3x3
W3Case = collections.namedtuple("W3Case", "name kind stride K cout maps xlo ylo modes")


def _w3_cases():
    out = []
    for K in (32, 64, 128):
        for kind in ("fwd", "dgrad"):
            modes = (PLAIN, STATS, ACCUM)
            out.append(W3Case("K%d %s s1 ragged maps" % (K, kind), kind, 1, K, K, ((1, 13, 17), (2, 9, 33)), 0, 0, modes))
        out.append(W3Case("K%d fwd s2 -> %d" % (K, 2 * K), "fwd", 2, K, 2 * K, ((2, 37, 45),), 0, 0, (PLAIN, STATS)))
    out.append(W3Case("K64 fwd s2 even map", "fwd", 2, 64, 128, ((1, 18, 34),), 0, 0, (PLAIN, STATS)))
    out.append(W3Case("eight jobs", "fwd", 1, 32, 32, ((1, 13, 17), (2, 9, 33), (1, 8, 16), (1, 5, 7), (2, 20, 20), (1, 1, 40), (1, 24, 3), (1, 16, 32)),
                      0, 0, (PLAIN, STATS, ACCUM)))
    out.append(W3Case("slice views", "dgrad", 1, 64, 64, ((2, 13, 17),), 64, 32, (PLAIN, STATS, ACCUM)))
    return out


W3_CASES = _w3_cases()


def _w3_jobs(c, mode):
    jobs = []
    for i, (N, H, W) in enumerate(c.maps):
        s = spec(c.kind, 3, N, H, W, c.K, c.cout, Kpad=c.K, CoutPad=c.cout, xlo=c.xlo, seed=600 + i)
        geo = geo_fwd(s, c.stride) if c.kind == "fwd" else geo_dgrad(s)
        jobs.append(Job(problem(s, geo, mode, c.ylo, 0)))
    return jobs


@pytest.mark.parametrize("c", W3_CASES, ids=lambda c: c.name.replace(" ", "_"))
def test_weight_stationary_3x3(c):
    """every case on the explicit entry (all its maps in ONE launch), then (7) routed: mi_conv2d per descriptor and
    mi_conv2d_group_plan with nothing forced must take the weight-stationary kernel (route 2 / meta.KC -2).  Partial tiles of
    the ragged maps must stay out of the statistics: exact equality proves it"""
    bad = []
    for mode in c.modes:
        bad += run_entry("mi_conv3x3_ws", _w3_jobs(c, mode), (c.name, mode.name))
        for j in _w3_jobs(c, mode)[:2]:
            bad += run_auto(j, (c.name, mode.name), 2)
        b, meta = run_group(_w3_jobs(c, mode), (c.name, mode.name), kc=-2)
        bad += b
        assert meta.KC != -2 or meta.BN == c.K
    torch.cuda.synchronize()
    assert not bad, bad[:20]


# ------------------------------------------------------------------------------------------ (8) the check has teeth
def _mutation(job, what, old_tolerance):
    """launch a WRONG descriptor against the true reference: the launch succeeds, problems() must report the output, and the
    stated tolerance check of the older tests would have passed it"""
    with env(**TILE_ONLY):
        L.check(L.lib().mi_conv2d(C.byref(job.desc()), L.stream_ptr()), what)
    torch.cuda.synchronize()
    bad = job.problems(what)
    assert [b[1][:2] for b in bad] == ["y:"], (what, bad)
    got, exp = job.ybuf[job.p.lay.idx].double(), job.p.exp
    assert old_tolerance(got, exp), (what, "the old tolerance would have caught it too: pick a shape where it does not")
    return bad


def _allclose_2e2(got, exp):                # np.testing.assert_allclose(rtol=2e-2, atol=2e-2): tests/test_gpu_conv3x3_ws.py, test_conv_forced_configs_agree
    return bool(((got - exp).abs() <= 2e-2 + 2e-2 * exp.abs()).all())


def _relerr_2e2(got, exp):                  # the norm-relative relerr < 2e-2 of tests/test_gpu_kernels.py::test_base_conv_fwd_bwd
    return float((got - exp).norm() / exp.norm()) < 2e-2


def test_mutation_one_tap_of_one_parity_class_moved():
    """the (1, 1) class of a stride-2 data gradient with ONE of its four taps moved by one pixel: 1 / 4 of the pixels carry one
    wrong tap of 2.25 on average - tried: the norm-relative relerr < 2e-2 of test_base_conv_fwd_bwd passes it on a gradient
    whose other consumers dominate (accumulate onto a large integer gradient); torch.equal does not"""
    H, W = 21, 23
    s = _s2_dgrad_spec(1, H, W, 16, 32, 700, Kpad=16)       # (moving the tap stays inside the halo the zero padding covers)
    geo = geo_s2_classes(s, H, W)[3]
    big = (torch.randint(0, 2, (1, H, W, 32), generator=torch.Generator().manual_seed(1)).double() * 2 - 1) * 200
    p = Problem(s, geo, ACCUM, old=big.to(DEV))
    taps = list(geo.taps)
    taps[2] = (taps[2][0], taps[2][1] + 1, taps[2][2])
    _mutation(Job(p, taps=taps), "one tap of the (1, 1) class moved by one pixel", _relerr_2e2)


def test_mutation_one_halo_tap_dropped():
    """a 3x3 convolution launched with 8 of its 9 taps (the reference keeps 9), accumulating onto a gradient of +-200 - tried:
    the norm-relative relerr < 2e-2 of test_base_conv_fwd_bwd passes it (one tap of 8 channels is ~1 % of that norm);
    torch.equal does not"""
    s = spec("fwd", 3, 1, 13, 17, 8, 32, Kpad=16, seed=701)
    geo = geo_fwd(s)
    g = torch.Generator().manual_seed(2)
    old = (torch.randint(0, 2, (1, 13, 17, 32), generator=g).double() * 2 - 1).to(DEV) * 200
    _mutation(Job(Problem(s, geo, ACCUM, old=old), taps=geo.taps[:8]), "ntaps 8 of 9", _relerr_2e2)


def test_mutation_grid_short_by_one_row():
    """gridH short by one row on an accumulating launch: the last row keeps its old value - tried: assert_allclose(rtol=2e-2,
    atol=2e-2) of test_conv_forced_configs_agree passes it where the missing contribution is below the tolerance of the large
    values it would have joined (old = +-240, |result| <= 4 from 4 real channels); torch.equal does not"""
    s = spec("fwd", 1, 1, 13, 17, 4, 32, Kpad=16, seed=702)
    geo = geo_fwd(s)
    g = torch.Generator().manual_seed(3)
    old = (torch.randint(0, 2, (1, 13, 17, 32), generator=g).double() * 2 - 1).to(DEV) * 240
    p = Problem(s, geo, ACCUM, old=old)
    assert float((p.exp - old).abs().max()) <= 4.0 + 1e-9
    _mutation(Job(p, gridH=geo.gridH - 1), "gridH short by one row", _allclose_2e2)
