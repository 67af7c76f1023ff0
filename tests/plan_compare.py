"""TEST INFRASTRUCTURE: compares the device's bytes of the arena buffers a command touched with the interpreter's
(tests/plan_interp.py run on the same input bytes).  Rules per kind of output:

  exact   integers and copies (packed weight images, SPP argmax codes, SimOTA assignment), and every byte of a
          buffer that lies outside the views the command references (a neighbouring concat slice, pad channels)
  bf16    inside the views the command WRITES: elementwise |got - ref| <= ULPS * ulp_bf16(|ref|) + 2^-10 * RMS(ref), plus
          a per-channel gain check (least-squares scale of the error against the reference) that catches a channel off
          by a fraction of an ulp; every other byte (views it only reads included) exact
  f32     reductions and fp32 maps: rel-L2 <= F32_REL and |got - ref| <= F32_REL * max|ref| elementwise
  f64acc  fp64 BatchNorm slot accumulators [nslots][C][2]: the sums over the slots (the interpreter adds to slot 0)
  loss    the loss values (rtol LOSS_RTOL), foreground / gt counts exact
  skip    pure workspaces: split-K partials, barrier words, the loss's cost / IoU / partial buffers

Lives under tests/: never imported by the product."""
import torch

from yolov7_d2_amd import _lib as L
from yolov7_d2_amd.plan import Buf, TRef, _rup

# Bounds: about 4x the worst values measured on an MI355X over the cases of tests/test_gpu_plan_commands.py (bf16 outputs of
# every op < 1 ulp beyond the floor; fp32 reductions and maps at most 4.4e-6 of max|ref| - the weight-gradient group's
# split-K - and 1.2e-6 for the BatchNorm sums; loss values at most 2.7e-7 relative)
ULPS = 2.0
FLOOR = 2.0 ** -10
GAIN = 1e-3
F32_REL = 1.6e-5
LOSS_RTOL = 1e-6

SKIP_NAMES = ("scratch.wgrad_ws", "scratch.dw_wgrad_ws", "loss.bias_ws", "loss.cost", "loss.iou", "loss.partial",
              "loss.partial_l1", "loss.match")


def kind_of(buf):
    n = buf.name
    if n in SKIP_NAMES or n.endswith(".bar"):
        return "skip"
    if n.startswith("scratch.bn_acc_"):
        return "f64acc"
    if n.endswith((".wf", ".wd", ".wd_pair", ".idx")) or n in ("loss.fg", "loss.mgt", "loss.ngt", "loss.gw"):
        return "exact"
    if n == "loss.out":
        return "loss"
    if n.endswith((".scale", ".shift", ".mean", ".invstd")) or n in ("preds", "loss.miou", "loss.dpreds"):
        return "f32"
    return "bf16"


def bf16_ulp(a):
    """ulp of bf16 numbers of magnitude |a| (fp32 tensor); 0 where a == 0"""
    e = torch.frexp(a.abs())[1]
    return torch.where(a == 0, torch.zeros_like(a), torch.ldexp(torch.ones_like(a), e - 8))


class Layout:
    """what the comparator needs to know about the buffers of one plan: the bf16 views that reference each buffer (the
    bytes a command may change) and the fp64 accumulator regions (offset, nslots, channels rounded to 32)"""

    def __init__(self, cmds, acc_is_workspace=False):
        """acc_is_workspace: the one-launch BatchNorm backward (BN_BWD_FUSED) keeps its sums in its own form - what it
        leaves in the accumulators is not an output"""
        self.views = {}      # id(buf) -> set of (coff, C, ld, N, H, W): every view the commands name (locations)
        self.outs = {}       # id(buf) -> set of (coff, C, ld, N, H, W): the bf16 views they WRITE
        self.acc = {}        # id(buf) -> {byte offset: (nslots, CA)}
        self.acc_skip = acc_is_workspace
        for c in cmds:
            self._add_cmd(c)

    def _view(self, t, out=False):
        if isinstance(t, TRef):
            v = (t.coff, t.C, t.ld, t.N, t.H, t.W)
            self.views.setdefault(id(t.buf), set()).add(v)
            if out:
                self.outs.setdefault(id(t.buf), set()).add(v)

    # bf16 tensors each op stores (operand indices into c.p); CONV: its y (and an input BatchNorm's activated tensor)
    OUT_P = dict(BN_ACT_FWD=(12,), BN_BWD_APPLY=(10, 11), DWCONV_FWD=(2,), DWCONV_DGRAD=(2,), FOCUS=(1,), UPSAMPLE_FWD=(1,),
                 UPSAMPLE_BWD=(1,), SPP_FWD=(1, 2, 3), SPP_BWD=(4,), SPLIT_DPREDS=(1,))

    def _acc(self, p, nslots, C):
        if p is not None and isinstance(p.obj, Buf):
            self.acc.setdefault(id(p.obj), {})[p.off] = (max(1, int(nslots) or L.MI_BN_SLOTS), _rup(C, 32))

    def _add_cmd(self, c, writes=True):
        op = L.OPS[c.op]
        assert op in self.OUT_P or op in ("CONV", "MEMSET", "NOP", "PACK_W", "WGRAD", "BN_BWD_REDUCE", "BN_EVAL_AFFINE",
                                          "DWCONV_WGRAD", "BIAS_GRADS", "COLSUM", "LOSS_FWD", "LOSS_BWD", "DECODE"), op
        for j, q in enumerate(c.p):
            self._view(q.obj, out=writes and j in self.OUT_P.get(op, ()))
        if c.desc is not None:
            for v in c.desc.__dict__.values():
                if isinstance(v, dict):
                    for w in v.values():
                        self._view(getattr(w, "obj", None))
                else:
                    self._view(getattr(v, "obj", None))
            if getattr(c.desc, "jobs", None):
                for j in c.desc.jobs:
                    self._view(getattr(j.get("dst"), "obj", None))
        if op == "CONV":
            s = c.desc
            self._view(s.y.obj, out=True)
            if s.stats.obj is not None:
                self._acc(s.stats, s.stats_slots, s.CoutPad if not (s.flags & L.MI_CONV_BNBWD) else s.Cout)
            bn = getattr(s, "xf_bn", None)
            if bn is not None:
                self._add_cmd(bn, writes=bool(s.xf_write))     # (only the record's writer stores the activated tensor)
        elif op == "BN_ACT_FWD" and c.p[1].obj is not None:
            self._acc(c.p[1], c.i[5], c.i[3])
        elif op == "BN_BWD_REDUCE":
            self._acc(c.p[6], c.i[5], c.i[3])
        elif op == "BN_BWD_APPLY":
            self._acc(c.p[7], c.i[7], c.i[5])
        elif op == "DWCONV_FWD" and c.p[3].obj is not None:
            self._acc(c.p[3], c.i[9], c.i[5])


class Report:
    def __init__(self):
        self.fails = []          # dicts: tag, op, buf, kind, worst, nbad, first
        self.dist = {}           # op -> list of per-buffer error arrays (ulps for bf16, rel for f32)

    def fail(self, **kw):
        self.fails.append(kw)

    def note(self, op, kind, err):
        if err is not None and err.numel():
            self.dist.setdefault((op, kind), []).append(err.float().flatten())

    def summary(self):
        lines = []
        for (op, kind), errs in sorted(self.dist.items()):
            e = torch.cat(errs)
            if e.numel() > 4_000_000:
                e = e[torch.randperm(e.numel(), generator=torch.Generator().manual_seed(0))[:4_000_000]]
            unit = "ulp" if kind == "bf16" else "rel"   # (f32: elementwise / max|ref|; f32-l2: per buffer)
            lines.append(f"{op:<18s} {kind:<6s} n={e.numel():>9d}  max={float(e.max()):.3g} {unit}  "
                         f"p99.9={float(torch.quantile(e, 0.999)):.3g} {unit}")
        return "\n".join(lines)

    def __str__(self):
        return "\n".join(f"{f['tag']} [{f['op']}] {f['buf']} ({f['kind']}): worst {f['worst']:.3g}, {f['nbad']} bad, "
                         f"first at {f['first']}" for f in self.fails[:20])


def _first(buf, layout, byte_off, esize=2):
    """(n, h, w, c) of a byte offset of a bf16 activation buffer (or the element index)"""
    vs = layout.views.get(id(buf))
    if vs:
        coff, C, ld, N, H, W = sorted(vs)[0]
        e = byte_off // 2
        pix, c = divmod(e, ld)
        n, r = divmod(pix, H * W)
        return (int(n), int(r // W), int(r % W), int(c))
    return int(byte_off // esize)


def compare_buffer(buf, got, ref, layout, rep, tag="", op="", mag=None):
    """got / ref: uint8 tensors (buf.nbytes) of the device and the interpreter; mag: fp32 operand magnitudes of
    accumulated bf16 elements (Interp.mag; 0 elsewhere).  Returns True when within the rules."""
    kind = kind_of(buf)
    n = buf.nbytes
    got, ref = got[:n], ref[:n]
    if kind == "skip" or torch.equal(got, ref):
        if kind == "bf16":
            rep.note(op, kind, torch.zeros(1))
        return True
    if kind == "exact":
        bad = (got != ref).nonzero()
        rep.fail(tag=tag, op=op, buf=buf.name, kind=kind, worst=float("inf"), nbad=int(bad.numel()),
                 first=_first(buf, layout, int(bad[0]), 1))
        return False
    if kind == "loss":
        g, r = got.view(torch.float32)[:8], ref.view(torch.float32)[:8]
        err = ((g[:6] - r[:6]).abs() / r[:6].abs().clamp_min(1e-30))
        rep.note(op, "f32", err)
        ok = bool((err <= LOSS_RTOL).all()) and torch.equal(g[6:], r[6:]) and torch.equal(got[32:], ref[32:])
        if not ok:
            rep.fail(tag=tag, op=op, buf=buf.name, kind=kind, worst=float(err.max()), nbad=int((err > LOSS_RTOL).sum()),
                     first=[float(x) for x in g] + [float(x) for x in r])
        return ok
    if kind == "f64acc":
        regions = layout.acc.get(id(buf), {})
        covered = torch.zeros(n, dtype=torch.bool)
        ok = True
        for off, (ns, CA) in sorted(regions.items()):
            nb = ns * CA * 16
            covered[off: off + nb] = True
            if layout.acc_skip:
                continue
            g = got[off: off + nb].view(torch.float64).view(ns, CA, 2).sum(0)
            r = ref[off: off + nb].view(torch.float64).view(ns, CA, 2).sum(0)
            ok &= _f32_rule(buf, g, r, rep, tag, op, layout, what=f"@{off}")
        rest = (got != ref) & ~covered
        if bool(rest.any()):
            rep.fail(tag=tag, op=op, buf=buf.name, kind="exact", worst=float("inf"), nbad=int(rest.sum()),
                     first=int(rest.nonzero()[0]))
            ok = False
        return ok
    if kind == "f32":
        m = n // 4 * 4
        return _f32_rule(buf, got[:m].view(torch.float32), ref[:m].view(torch.float32), rep, tag, op, layout)
    return _bf16_rule(buf, got, ref, layout, rep, tag, op, mag)


def _f32_rule(buf, g, r, rep, tag, op, layout, what=""):
    g, r = g.double().flatten(), r.double().flatten()
    d = (g - r).abs()
    amax = float(r.abs().max()) if r.numel() else 0.0
    rel = float(d.norm() / max(float(r.norm()), 1e-300))
    el = d / max(amax, 1e-300)
    rep.note(op, "f32", el)
    rep.note(op, "f32-l2", torch.tensor([rel]))
    bad = (el > F32_REL) | ~torch.isfinite(g)
    if rel <= F32_REL and not bool(bad.any()):
        return True
    idx = int(bad.nonzero()[0]) if bool(bad.any()) else int(d.argmax())
    rep.fail(tag=tag, op=op, buf=buf.name + what, kind="f32", worst=max(rel, float(el.max())), nbad=int(bad.sum()),
             first=idx)
    return False


def _bf16_rule(buf, got, ref, layout, rep, tag, op, mag=None):
    n = buf.nbytes
    vs = layout.outs.get(id(buf), set())
    inview = torch.zeros(n // 2, dtype=torch.bool)
    views = []
    for (coff, C, ld, N, H, W) in vs:
        npx = N * H * W
        m = inview[: npx * ld].view(npx, ld)
        m[:, coff: coff + C] = True
        views.append((coff, C, ld, npx))
    g16, r16 = got[: n // 2 * 2].view(torch.bfloat16), ref[: n // 2 * 2].view(torch.bfloat16)
    ok = True
    outside = (g16.view(torch.int16) != r16.view(torch.int16)) & ~inview
    if bool(outside.any()):
        i = int(outside.nonzero()[0])
        rep.fail(tag=tag, op=op, buf=buf.name, kind="exact", worst=float("inf"), nbad=int(outside.sum()),
                 first=_first(buf, layout, 2 * i))
        ok = False
    g, r = g16.float(), r16.float()
    sel = inview
    if not bool(sel.any()):
        return ok
    rs = r[sel]
    rms = float(rs.pow(2).mean().sqrt())
    floor = FLOOR * rms
    d = (g - r).abs()
    ulp = bf16_ulp(r if mag is None else torch.maximum(r.abs(), mag[: r.numel()]))
    u = (d - floor).clamp_min(0) / ulp.clamp_min(2.0 ** -133)
    u = torch.where(sel, u, torch.zeros_like(u))
    u = torch.where(torch.isfinite(g) | ~sel, u, torch.full_like(u, float("inf")))
    rep.note(op, "bf16", u[sel])
    bad = u > ULPS
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        rep.fail(tag=tag, op=op, buf=buf.name, kind="bf16", worst=float(u.max()), nbad=int(bad.sum()),
                 first=_first(buf, layout, 2 * i),
                 bad=[(_first(buf, layout, 2 * int(j)), float(g[j]), float(r[j])) for j in bad.nonzero()[:64, 0]])
        ok = False
    # per channel of each view: least-squares gain of the error against the reference (a channel scaled by 1 + e shows
    # e; rounding noise averages out to ~ulp / sqrt(pixels))
    for (coff, C, ld, npx) in views:
        if npx < 64:
            continue
        gv = g[: npx * ld].view(npx, ld)[:, coff: coff + C]
        rv = r[: npx * ld].view(npx, ld)[:, coff: coff + C]
        den = rv.double().pow(2).sum(0)
        gain = ((gv - rv).double() * rv.double()).sum(0) / den.clamp_min(1e-300)
        gain = torch.where(den > 0, gain, torch.zeros_like(gain))
        badc = gain.abs() > GAIN
        if bool(badc.any()):
            c = int(badc.nonzero()[0])
            rep.fail(tag=tag, op=op, buf=buf.name, kind="bf16-gain", worst=float(gain.abs().max()), nbad=int(badc.sum()),
                     first=("channel", coff + c))
            ok = False
    return ok
