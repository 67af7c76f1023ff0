"""Step plan: the host-side graph builder that turns the reference's module tree
(BaseConv / CSPLayer / YOLOPAFPN / YOLOXHead ...) into two flat command lists (forward, backward)
over one device arena, executed by libmi355det's C++ command-list runner or replayed as a hipGraph.

Nothing here computes: it only lays out buffers (NHWC bf16 activations, concat buffers whose channel
slices are written in place by their producers, gradient mirrors, shared scratch) and records which
C-ABI entry runs on which pointers.  Gradient fan-in (a tensor read by several consumers) is resolved
statically: the first backward writer overwrites, later ones accumulate in their epilogue.
"""
import ctypes as C
import math
import os

import torch

from . import _lib as L


def _rup(a, b):
    return (a + b - 1) // b * b


class Buf:
    """A region of the arena (offset assigned at finalize)."""

    def __init__(self, name, nbytes, zero=False):
        self.name, self.nbytes, self.offset, self.zero = name, int(nbytes), None, zero
        self.base = None

    @property
    def ptr(self):
        return self.base + self.offset


class TRef:
    """bf16 NHWC view: N x H x W x C at channel offset `coff` of a buffer with pixel stride `ld`."""

    def __init__(self, buf, N, H, W, C, ld, coff=0, gbuf=None):
        self.buf, self.N, self.H, self.W, self.C, self.ld, self.coff, self.gbuf = buf, N, H, W, C, ld, coff, gbuf

    @property
    def ptr(self):
        return self.buf.ptr + 2 * self.coff

    @property
    def npix(self):
        return self.N * self.H * self.W

    @property
    def requires_grad(self):
        return self.gbuf is not None

    @property
    def grad(self):
        assert self.gbuf is not None, "tensor has no gradient buffer"
        return TRef(self.gbuf, self.N, self.H, self.W, self.C, self.ld, self.coff, None)

    def slice(self, c0, c1):
        assert 0 <= c0 < c1 <= self.C and c0 % 8 == 0 and c1 % 8 == 0
        return TRef(self.buf, self.N, self.H, self.W, c1 - c0, self.ld, self.coff + c0, self.gbuf)


class _Ptr:
    """late-bound pointer: buffer (+ byte offset) or torch tensor"""

    def __init__(self, obj, off=0):
        self.obj, self.off = obj, off

    def resolve(self):
        o = self.obj
        if o is None:
            return None
        if isinstance(o, (Buf, TRef)):
            return o.ptr + self.off
        if isinstance(o, torch.Tensor):
            return o.data_ptr() + self.off
        if isinstance(o, int):
            return o + self.off
        raise TypeError(type(o))


class _Cmd:
    def __init__(self, op, i=(), f=(), p=(), l=(), desc=None, tag=""):
        self.op, self.i, self.f, self.p, self.l, self.desc, self.tag = op, list(i), list(f), list(p), list(l), desc, tag
        self.lane = 0          # index of the independent chain (inside a parallel region) this command belongs to


class ConvSpec:
    """symbolic mi_conv_desc"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def lane_out_key(c):
    """identity of the tensor a groupable command writes (two commands with the same key must never share a launch and
    must keep their original order)"""
    if c.op == L.OP["CONV"]:
        y = c.desc.y
        return (id(getattr(y.obj, "buf", y.obj)), getattr(y.obj, "coff", 0), y.off)
    if c.op in (L.OP["BN_BWD_APPLY"], L.OP["BN_BWD_FUSED"]) and c.p[11].obj is not None:
        return (id(c.p[11].obj.buf), c.p[11].obj.coff, 0)
    return id(c)


def schedule_lanes(region):
    """list scheduling of the independent chains (lanes) of a parallel region (pure host logic, no device needed).
    Walks the chains in lock step: the op kind most lanes have next (convolutions / BatchNorm passes win ties) is taken
    from all those lanes at once.  Returns a list of issue sets; the commands of a set are mutually independent, have
    the same op and pairwise different output tensors - writers of one tensor (two data gradients accumulating into the
    same input gradient) are split into consecutive sets in their original order."""
    groupable = {L.OP["CONV"], L.OP["BN_ACT_FWD"], L.OP["BN_BWD_REDUCE"], L.OP["BN_BWD_APPLY"], L.OP["BN_BWD_FUSED"]}
    order = {id(r): i for i, r in enumerate(region)}
    lanes = sorted({r.lane for r in region})
    chains = [[r for r in region if r.lane == ln] for ln in lanes]
    pos = [0] * len(chains)
    sets = []
    # writers of one tensor must run in their original order (a first writer overwrites, later ones accumulate): a
    # command is ready only when every earlier writer of its output has been issued.  The earliest unissued command of
    # the original order is always ready, so the walk cannot dead-lock.
    writers = {}
    for r in region:
        writers.setdefault(lane_out_key(r), []).append(r)
    issued = set()

    def ready(c):
        for w in writers[lane_out_key(c)]:
            if w is c:
                return True
            if id(w) not in issued:
                return False
        return True

    while any(p < len(ch) for p, ch in zip(pos, chains)):
        kinds = {}
        for li, (p, ch) in enumerate(zip(pos, chains)):
            if p < len(ch) and ready(ch[p]):
                kinds.setdefault(ch[p].op, []).append(li)
        # most lanes first; on a tie the lanes that still have the most commands left (so shorter chains wait for longer
        # ones to catch up and their convolutions / BatchNorm passes line up), then groupable ops
        op = max(kinds, key=lambda o: (len(kinds[o]), sum(len(chains[li]) - pos[li] for li in kinds[o]), o in groupable))
        sel = kinds[op]
        cs = sorted((chains[li][pos[li]] for li in sel), key=lambda c: order[id(c)])
        for li in sel:
            pos[li] += 1
        seen, waves = {}, {}
        for c in cs:
            kk = lane_out_key(c)
            w = seen.get(kk, 0)
            seen[kk] = w + 1
            waves.setdefault(w, []).append(c)
        sets += [waves[w] for w in sorted(waves)]
        issued.update(id(c) for c in cs)
    return sets


class PlanBuilder:
    def __init__(self, device, training=True, bn_train=None, group_wgrad=None):
        import os
        self.device = torch.device(device)
        # all weight gradients in one grouped launch at the end of backward (each layer keeps its own dy buffer)
        self.group_wgrad = (os.environ.get("MI_WGRAD_GROUP", "1") != "0") if group_wgrad is None else group_wgrad
        # every command runs on the caller's stream: the head's FPN levels as parallel hipGraph branches measured 3 %
        # slower and the option was removed (docs/DESIGN_rounds_1_3.md, tools/micro/graph_branches.hip)
        self.cur_lane = 0
        # the independent chains of a parallel region (the head's FPN levels) zipped into grouped launches: one
        # CONV_GROUP / BN_GROUP per chain position instead of one launch per level
        self.group_lanes = os.environ.get("MI_GROUP_LEVELS", "1") != "0"
        # weight gradients of the head + neck layers in their own grouped launch as soon as those layers' backward is done,
        # so that their gradient bucket can be all-reduced while the backbone's backward still runs (data parallel only:
        # MI_WGRAD_SPLIT unset -> on iff torch.distributed is initialised with world_size > 1)
        ws_env = os.environ.get("MI_WGRAD_SPLIT", "")
        if ws_env:
            self.wgrad_split = ws_env != "0"
        else:
            import torch.distributed as dist
            self.wgrad_split = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        self.wgrad_early_prefixes = ("head.", "neck.")
        # the split as STAGES (backward order): each stage's weight gradients form one grouped launch issued right after
        # the stage's last backward command, and one gradient bucket (parameters are laid out backbone.stem .. dark5,
        # neck, head, so a stage is a contiguous range of the flat arena); whatever matches no stage runs at the end.
        # Three buckets: [neck + head] on the wire under the whole backbone, [dark4 + dark5] under dark3 .. stem, only the
        # last (stem .. dark3, 2.4 MB of the 35.9) is exposed.
        self.wgrad_stages = [("head.", "neck."), ("backbone.dark5.", "backbone.dark4.")]
        self.csp_lanes = os.environ.get("MI_CSP_LANES", "1") != "0"   # CSP conv1 / conv2 as lanes (see blocks.CSPLayer)
        self.training = training            # build the backward command list
        self.bn_train = training if bn_train is None else bn_train  # batch statistics vs running statistics
        self.bufs = []
        self.shared = {}
        self.prologue = []   # weight packing etc, start of forward
        self.fwd = []
        self.bwd_gens = []   # closures run in reverse at finalize
        self.bwd = []
        self._emitting_bwd = False
        self.grad_init = {}  # id(gbuf) -> list of (c0,c1) initialised channel intervals
        self.last_writer = {}  # id(gbuf) -> [(c0, c1, [conv cmds])]: channel ranges whose LATEST writer is a data-gradient conv
        # BatchNorm-backward sums taken by the data-gradient conv that writes the final da (MI_CONV_BNBWD) instead of a
        # separate reduce pass over (da, y): 53 of the 74 reduce launches of YOLOX-s disappear, but measured (A/B, round 1)
        # the step time does not move - the fp64 accumulator atomics a block must wait for cost the data-gradient
        # kernels what the reduce kernels cost -> opt-in
        self.fuse_bn_bwd = os.environ.get("MI_FUSE_BN_BWD", "0") != "0"
        self.keep = []       # python objects that must outlive the plan (ctypes descs, tensors)
        self.tune_restore = []   # tensors a replay of the forward list mutates (BN running statistics)
        self.loss = None
        self.conv_records = []  # (tag, spec) for roofline bookkeeping
        self.bias_jobs = []     # prediction-conv bias gradients (one BIAS_GRADS command after the loss backward)

    # ---------------------------------------------------------------- buffers
    def _new_buf(self, name, nbytes, zero=False):
        b = Buf(name, _rup(max(int(nbytes), 16), 256), zero)
        self.bufs.append(b)
        return b

    def new_act(self, N, H, W, C, name, requires_grad=True, pad=True):
        """bf16 NHWC activation (+ gradient mirror).  The pixel stride is C rounded up to 32 channels: a consumer conv
        reads whole 32-channel k-groups, so widths that are not multiples of 32 (24 / 48 / 80 ... of the 0.375 / 0.75 /
        1.25 width multipliers) carry zero pad channels that nothing ever writes (the arena starts zeroed; producers
        store real channel groups only) and that meet zero-padded weight rows in the packed weight images."""
        assert C % 8 == 0
        ld = _rup(C, 32) if pad else C
        b = self._new_buf(name, N * H * W * ld * 2)
        g = self._new_buf(name + ".grad", N * H * W * ld * 2) if (requires_grad and self.training) else None
        return TRef(b, N, H, W, C, ld, 0, g)

    def small(self, name, nbytes, zero=False):
        return self._new_buf(name, nbytes, zero)

    @staticmethod
    def bn_slots(nunits):
        """accumulator slots for a layer whose producers add `nunits` partial sums per channel: ~64+ adds per address
        keep the atomics cheap, few slots keep the BN kernels' statistics prologue short"""
        # measured (A/B, round 1): fewer slots shorten the BN prologue (0.78 -> 0.67 ms/step) but slow the conv
        # epilogues by more (same-address fp64 atomics): 16 everywhere was the best whole-step setting.  Round 3: the
        # persistent 1x1 / 3x3 kernels add one partial per BLOCK (256 per layer), which moves the optimum to 8
        # (same-box A/B: 16: 5.701, 8: 5.677, 4: 5.713, 2: 5.92 ms/step; MI_BN_NSLOTS overrides)
        ov = int(os.environ.get("MI_BN_NSLOTS", "0"))
        return ov if 1 <= ov <= L.MI_BN_SLOTS else 8

    def bn_acc(self, which, C, nslots=None):
        """fp64 BatchNorm accumulators [MI_BN_SLOTS][C][2] inside ONE contiguous region per direction, zeroed by a
        single MEMSET at the start of the forward / backward command list"""
        key = "bn_acc_" + which
        b = self.shared.get(key)
        if b is None:
            b = Buf("scratch." + key, 0)
            self.shared[key] = b
            self.bufs.append(b)
        off = b.nbytes
        b.nbytes += (L.MI_BN_SLOTS if nslots is None else nslots) * _rup(C, 32) * 2 * 8   # [slot][C rounded to 32][2]
        return _Ptr(b, off)

    def scratch(self, key, nbytes):
        """shared scratch (max size over requests); valid only between adjacent commands of one layer"""
        b = self.shared.get(key)
        if b is None:
            b = Buf("scratch." + key, 0)
            self.shared[key] = b
            self.bufs.append(b)
        b.nbytes = max(b.nbytes, _rup(int(nbytes), 256))
        return b

    # ---------------------------------------------------------------- command emission
    def emit(self, op, i=(), f=(), p=(), l=(), desc=None, tag="", prologue=False):
        c = _Cmd(L.OP[op], i, f, [x if isinstance(x, _Ptr) else _Ptr(x) for x in p], l, desc, tag)
        c.lane = 0 if prologue else self.cur_lane
        if self._emitting_bwd:
            self.bwd.append(c)
        elif prologue:
            self.prologue.append(c)
        else:
            self.fwd.append(c)
        return c

    def on_backward(self, fn):
        if self.training:
            self.bwd_gens.append((fn, self.cur_lane))

    # ---------------------------------------------------------------- parallel regions
    def par_begin(self, tag="par"):
        """start of a region of independent chains (see `on_lane`), marked by a NOP that Plan._group_lanes consumes.  The
        backward list gets the mirrored region automatically."""
        self.emit("NOP", tag=tag + ".begin")
        self.on_backward(lambda: self.emit("NOP", tag=tag + ".end"))

    def par_end(self, tag="par"):
        self.emit("NOP", tag=tag + ".end")
        self.on_backward(lambda: self.emit("NOP", tag=tag + ".begin"))

    def on_lane(self, lane):
        """commands emitted inside belong to independent chain `lane` of the enclosing parallel region (see
        Plan._group_lanes)"""
        b = self

        class _Ctx:
            def __enter__(self_):
                self_.prev = b.cur_lane
                b.cur_lane = lane

            def __exit__(self_, *a):
                b.cur_lane = self_.prev
        return _Ctx()

    def grad_mode(self, t):
        """returns 1 (accumulate) if t's gradient region was already written in this backward pass, else 0
        and marks it written."""
        key = id(t.gbuf)
        iv = self.grad_init.setdefault(key, [])
        c0, c1 = t.coff, t.coff + t.C
        lw = self.last_writer.setdefault(key, [])   # whoever asks is about to write [c0, c1): older records are stale
        lw[:] = [w for w in lw if not (w[0] < c1 and c0 < w[1])]
        covered = [a for a in iv if a[0] < c1 and c0 < a[1]]
        if not covered:
            iv.append((c0, c1))
            return 0
        # must be fully covered by the union of existing intervals
        pts = sorted(covered)
        cur = c0
        for a0, a1 in pts:
            if a0 > cur:
                break
            cur = max(cur, a1)
        if cur >= c1:
            return 1
        raise NotImplementedError(f"partial gradient overlap on {t.buf.name} [{c0},{c1}) vs {pts}")

    def grad_ready(self, t):
        iv = self.grad_init.get(id(t.gbuf), [])
        c0, c1 = t.coff, t.coff + t.C
        cur = c0
        for a0, a1 in sorted(iv):
            if a0 > cur:
                break
            cur = max(cur, a1)
        return cur >= c1

    # ---------------------------------------------------------------- conv helpers
    @staticmethod
    def fwd_taps(k, pad):
        return [(r - pad, s - pad, r * k + s) for r in range(k) for s in range(k)]

    def conv_cmd(self, tag, x, w_img, K8, y_ptr, ldy, outH, outW, Cout, CoutPad, taps, in_stride=1, out_stride=1,
                 out_oy=0, out_ox=0, gridH=None, gridW=None, bias=None, stats=None, flags=0, y_nstride=0,
                 inH=None, inW=None, stats_slots=0):
        spec = ConvSpec(x=_Ptr(x), w=_Ptr(w_img), y=y_ptr if isinstance(y_ptr, _Ptr) else _Ptr(y_ptr),
                        bias=_Ptr(bias), stats=stats if isinstance(stats, _Ptr) else _Ptr(stats), ldx=x.ld, ldy=ldy, y_nstride=y_nstride, N=x.N,
                        H=x.H if inH is None else inH, W=x.W if inW is None else inW, outH=outH, outW=outW,
                        gridH=outH if gridH is None else gridH, gridW=outW if gridW is None else gridW,
                        in_stride=in_stride, out_stride=out_stride, out_oy=out_oy, out_ox=out_ox, K8=K8, Cout=Cout,
                        CoutPad=CoutPad, taps=taps, flags=flags, tag=tag, stats_slots=stats_slots)
        self.conv_records.append(spec)
        return self.emit("CONV", desc=spec, tag=tag)

    def plan_conv_tiles(self, x, Ho, Wo, K8, Cout, taps, stride):
        """number of pixel tiles (rows of the stats partial buffer) the launcher will use for this forward conv:
        asked from the library itself (mi_conv2d_plan) so host and device agree on the tile heuristics"""
        d = L.mi_conv_desc()
        d.N, d.H, d.W, d.outH, d.outW, d.gridH, d.gridW = x.N, x.H, x.W, Ho, Wo, Ho, Wo
        d.in_stride, d.out_stride = stride, 1
        d.K8, d.Cout, d.CoutPad, d.ntaps = K8, Cout, _rup(Cout, 32), len(taps)
        for t, (dy, dx, w) in enumerate(taps):
            d.tap_dy[t], d.tap_dx[t], d.tap_w[t] = dy, dx, w
        d.ldx, d.ldy = x.ld, Cout
        d.x = d.w = d.y = 256  # non-null, 16B aligned dummies; nothing is launched
        n = L.lib().mi_conv2d_plan(C.byref(d))
        L.check(n, "mi_conv2d_plan")
        return n

    # ---------------------------------------------------------------- layers
    class DgradPair:
        """two 1x1 BaseConvs that read the SAME tensor (CSPLayer conv1 / conv2, darknetx CSPLayer.forward): their data
        gradients dx = W1^T dy1 + W2^T dy2 are ONE convolution over the channel concatenation [dy1 | dy2] with the two
        weight images stacked along K - one launch that writes dx once instead of a second launch that reads dx back and
        adds to it.  The two layers write their out-gradients into the two channel slices of one buffer."""

        def __init__(self, b, tag, x, couts):
            self.b, self.tag, self.x, self.couts = b, tag, x, list(couts)
            self.offs = [0]
            for c in couts:
                self.offs.append(self.offs[-1] + c)
            self.K = self.offs[-1]
            self.CinPadN = _rup(x.C, 32)
            self.wd = b.small(tag + ".wd_pair", self.K * self.CinPadN * 2)
            self.dy = None
            self.ready = []

        def wd_slice(self, slot):
            return _Ptr(self.wd, self.offs[slot] * self.CinPadN * 2)      # rows [k8][CinPadN][8]: slot's rows follow

        def dy_view(self, slot, N, H, W):
            if self.dy is None:
                self.dy = self.b._new_buf(self.tag + ".dy_pair", N * H * W * self.K * 2)
            self.ready.append(slot)
            return TRef(self.dy, N, H, W, self.couts[slot], self.K, self.offs[slot])

        def flush(self):
            """after both layers' backward commands (and after the parallel region that holds them): the one data gradient"""
            assert sorted(self.ready) == list(range(len(self.couts))), (self.tag, self.ready)
            x = self.x
            dyT = TRef(self.dy, x.N, x.H, x.W, self.K, self.K)
            self.b.dgrad_cmds(self.tag + ".pair", dyT, self.wd, self.K // 8, x, x.C, self.CinPadN, 1, 1, 0)

    def dgrad_pair(self, tag, x, couts):
        """-> DgradPair or None when the pair form does not apply (see base_conv(dgrad_pair=))"""
        ok = (self.training and x.requires_grad and self.group_wgrad and os.environ.get("MI_CSP_DGRAD_PAIR", "1") != "0"
              and all(c % 32 == 0 for c in couts) and x.C % 8 == 0)
        if not ok:
            return None
        pair = PlanBuilder.DgradPair(self, tag, x, couts)
        self.on_backward(pair.flush)
        return pair

    def base_conv(self, tag, x, weight, bn, k, stride, wgrad, out=None, res=None, act=1, groups=1, dgrad_pair=None):
        """Conv(k, stride, pad=(k-1)//2, no bias) -> BatchNorm -> SiLU (+ res).
        weight: fp32 OIHW tensor; wgrad: fp32 OIHW gradient view (training);
        bn: dict(gamma, beta, rm, rv, nbt, eps, momentum, ggamma, gbeta).
        groups: 1, or the channel count (depthwise 3x3: the dconv of DWConv, wrappers.py:86-102)."""
        Cout, Cin = weight.shape[0], weight.shape[1] * groups
        dw = groups != 1
        if dw:
            assert groups == Cout == Cin and k == 3 and weight.shape[1] == 1, (tag, groups, tuple(weight.shape))
        assert weight.shape[2] == k and Cout % 8 == 0, (tag, tuple(weight.shape))
        CoutPad = _rup(Cout, 32)        # cout tile granularity of the conv / weight-gradient kernels
        pad = (k - 1) // 2
        Ho = (x.H + 2 * pad - k) // stride + 1
        Wo = (x.W + 2 * pad - k) // stride + 1
        # readable input channels: whole 32-channel k-groups when the view has them (its buffer's pixel stride covers the
        # pad), 16 for the 12-channel stem.  Channels between Cin and CinPad meet zero weight rows.
        CinPad = _rup(Cin, 32) if x.coff + _rup(Cin, 32) <= x.ld else _rup(Cin, 16)
        assert x.C >= Cin and x.coff + CinPad <= x.ld, (tag, x.C, x.coff, x.ld, Cin)
        KK = k * k
        need_dgrad = self.training and x.requires_grad
        CinPadN = _rup(Cin, 32)
        wf = wd = None
        if dgrad_pair is not None:
            pair, slot = dgrad_pair
            assert k == 1 and stride == 1 and not dw and need_dgrad and Cout == CoutPad == pair.couts[slot] and pair.x is x
        if not dw:
            wf = self.small(tag + ".wf", KK * CinPad * CoutPad * 2)
            wd = self.small(tag + ".wd", KK * CoutPad * CinPadN * 2) if need_dgrad else None
            if dgrad_pair is not None:
                wd = pair.wd_slice(slot)
            self.emit("PACK_W", i=[Cout, Cin, k, k, CinPad, CoutPad, CoutPad, CinPadN], p=[weight, wf, wd],
                      tag=tag + ".pack", prologue=True)

        def fwd_conv(acc, nsl):
            if dw:     # no weight image: the kernel reads (and bf16-rounds) the fp32 parameter
                self.emit("DWCONV_FWD", i=[x.ld, y.ld, x.N, x.H, x.W, Cout, stride, Ho, Wo, nsl], p=[x, weight, y, acc],
                          tag=tag + ".conv")
            else:
                self.conv_cmd(tag + ".conv", x, wf, CinPad // 8, y, y.ld, Ho, Wo, Cout, CoutPad, taps, in_stride=stride,
                              stats=acc, stats_slots=nsl)
        y = self.new_act(x.N, Ho, Wo, Cout, tag + ".y", requires_grad=False, pad=False)
        if out is None:
            out = self.new_act(x.N, Ho, Wo, Cout, tag + ".out")
        assert (out.N, out.H, out.W, out.C) == (x.N, Ho, Wo, Cout)
        scale = self.small(tag + ".scale", Cout * 4)
        shift = self.small(tag + ".shift", Cout * 4)
        taps = self.fwd_taps(k, pad)
        count = x.N * Ho * Wo
        if self.bn_train:
            mean = self.small(tag + ".mean", Cout * 4)
            invstd = self.small(tag + ".invstd", Cout * 4)
            nsl = self.bn_slots(0 if dw else self.plan_conv_tiles(x, Ho, Wo, CinPad // 8, Cout, taps, stride))
            acc = self.bn_acc("fwd", Cout, nsl)
            fwd_conv(acc, nsl)
            self.tune_restore += [t for t in (bn["rm"], bn["rv"], bn["nbt"]) if torch.is_tensor(t)]
            self.emit("BN_ACT_FWD", i=[y.ld, res.ld if res is not None else 0, out.ld, Cout, act, nsl], l=[count, count],
                      f=[bn["eps"], bn["momentum"]],
                      p=[y, acc, bn["gamma"], bn["beta"], bn["rm"], bn["rv"], bn["nbt"], scale, shift, mean, invstd, res,
                         out], tag=tag + ".bnact")
        else:
            fwd_conv(None, 0)
            self.emit("BN_EVAL_AFFINE", i=[Cout], f=[bn["eps"]],
                      p=[bn["gamma"], bn["beta"], bn["rm"], bn["rv"], scale, shift], tag=tag + ".bnaff")
            self.emit("BN_ACT_FWD", i=[y.ld, res.ld if res is not None else 0, out.ld, Cout, act, 0], l=[0, count],
                      p=[y, None, None, None, None, None, None, scale, shift, None, None, res, out], tag=tag + ".bnact")

        def bwd():
            da = out.grad
            assert self.grad_ready(out), f"{tag}: output gradient never written"
            C8 = Cout // 8
            nblk = max(1, min(1024, math.ceil(count / (256 // C8) / 4)))
            nsl2 = self.bn_slots(nblk)
            fused = None
            if self.fuse_bn_bwd and Cout == CoutPad:   # the latest writer of exactly this gradient view is a data-gradient conv (set)
                for (w0, w1, cmds) in self.last_writer.get(id(out.gbuf), []):
                    if (w0, w1) == (out.coff, out.coff + Cout) and all(c.desc.ldy == da.ld for c in cmds):
                        fused = cmds
            if fused is not None:
                nsl2 = self.bn_slots(1 << 30)
            dacc = self.bn_acc("bwd", Cout, nsl2)
            # the out-gradient is read by the data / weight gradient kernels in whole 32-channel groups: pad channels
            # stay zero (a dedicated, never-written part of the zero-initialised arena)
            assert Cout == CoutPad or self.group_wgrad, "padded channel counts need per-layer dy buffers (MI_WGRAD_GROUP=1)"
            if dgrad_pair is not None:
                dyT = pair.dy_view(slot, x.N, Ho, Wo)
            else:
                dy = (self._new_buf(tag + ".dy", count * CoutPad * 2) if self.group_wgrad
                      else self.scratch("dy", count * CoutPad * 2))
                dyT = TRef(dy, x.N, Ho, Wo, CoutPad, CoutPad)
            if fused is not None:
                for c in fused:
                    sp = c.desc
                    sp.flags |= L.MI_CONV_BNBWD
                    sp.stats, sp.stats_slots = (dacc if isinstance(dacc, _Ptr) else _Ptr(dacc)), nsl2
                    sp.bnb = dict(y=_Ptr(y), ldy=y.ld, scale=_Ptr(scale), shift=_Ptr(shift), mean=_Ptr(mean),
                                  invstd=_Ptr(invstd), act=act)
                    c.tag += "+bnred"
            else:
                self.emit("BN_BWD_REDUCE", i=[da.ld, y.ld, nblk, Cout, act, nsl2], l=[count],
                          p=[da, y, scale, shift, mean, invstd, dacc], tag=tag + ".bnred")
            dres, dres_acc = None, 0
            if res is not None and res.requires_grad:
                dres = res.grad
                dres_acc = self.grad_mode(res)
            self.emit("BN_BWD_APPLY", i=[da.ld, y.ld, dyT.ld, dres.ld if dres is not None else 0, dres_acc, Cout, act, nsl2],
                      l=[count, count], p=[da, y, scale, shift, mean, invstd, bn["gamma"], dacc, bn["ggamma"], bn["gbeta"],
                                           dyT, dres, self.small(tag + ".bar", 4 * L.MI_BN_BAR_WORDS)], tag=tag + ".bnapply")
            if dw:
                nb = L.lib().mi_dwconv3x3_wgrad_ws_bytes(Cout)
                self.emit("DWCONV_WGRAD", i=[x.ld, dyT.ld, x.N, x.H, x.W, Cout, stride, Ho, Wo], l=[nb],
                          p=[x, dyT, self.scratch("dw_wgrad_ws", nb), wgrad], tag=tag + ".wgrad")
                if need_dgrad:
                    self.emit("DWCONV_DGRAD", i=[dyT.ld, x.grad.ld, x.N, x.H, x.W, Cout, stride, Ho, Wo, self.grad_mode(x)],
                              p=[dyT, weight, x.grad], tag=tag + ".dgrad")
                return
            self.wgrad_cmds(tag, x, dyT, CinPad if (k > 1 or CinPad % 32 == 0) else _rup(Cin, 32), CoutPad, Cin, Cout, k,
                            stride, pad, wgrad)
            if need_dgrad and dgrad_pair is None:      # (a pair's single data gradient is emitted by DgradPair.flush)
                self.dgrad_cmds(tag, dyT, wd, CoutPad // 8, x, Cin, CinPadN, k, stride, pad)

        self.on_backward(bwd)
        return out

    def wgrad_cmds(self, tag, x, dyT, CinPad, CoutPad, Cin, Cout, k, stride, pad, wgrad):
        """weight gradient straight into the fp32 OIHW gradient view (split-K workspace shared by all layers)"""
        taps = [(r - pad, s - pad) for r in range(k) for s in range(k)]
        spec = ConvSpec(kind="wgrad", x=_Ptr(x), dy=_Ptr(dyT), gw=_Ptr(wgrad), ldx=x.ld, ldy=dyT.ld, N=x.N, H=x.H,
                        W=x.W, outH=dyT.H, outW=dyT.W, stride=stride, Cin=Cin, Cout=Cout, CinPad=CinPad,
                        CoutPad=CoutPad, taps=taps, tag=tag)
        d = self._wgrad_desc(spec)
        nbytes = L.lib().mi_conv2d_wgrad_plan(C.byref(d))
        L.check(nbytes, "mi_conv2d_wgrad_plan")
        spec.ws = self.scratch("wgrad_ws", nbytes)
        self.emit("WGRAD", desc=spec, tag=tag + ".wgrad")

    @staticmethod
    def _wgrad_desc(spec):
        d = L.mi_wgrad_desc()
        for kk in ("ldx", "ldy", "N", "H", "W", "outH", "outW", "stride", "Cin", "Cout", "CinPad", "CoutPad"):
            setattr(d, kk, int(getattr(spec, kk)))
        d.ntaps = len(spec.taps)
        for t, (dy, dx) in enumerate(spec.taps):
            d.tap_dy[t], d.tap_dx[t] = dy, dx
        return d

    def dgrad_cmds(self, tag, dyT, wd, K8, x, Cin, CinPadN, k, stride, pad):
        """data gradient into x.grad; dyT: out-grad view with K8*8 readable channels"""
        dx = x.grad
        acc = self.grad_mode(x)
        if acc:
            # test-only mutation (tests/test_gpu_parity_bench.py): MI_TEST_DROP_ACCUM=n makes the n-th accumulating data
            # gradient OVERWRITE its target, i.e. drops the earlier consumers' contribution - the whole-step parity
            # check must catch it
            self._n_accum = getattr(self, "_n_accum", 0) + 1
            if os.environ.get("MI_TEST_DROP_ACCUM", "") == str(self._n_accum):
                acc = 0
        flags = L.MI_CONV_ACCUM if acc else 0
        # output channels written: the real Cin (x may carry zero pad channels, e.g. the 12->16 stem)
        cmds = []
        if stride == 1:
            taps = [(pad - r, pad - s, r * k + s) for r in range(k) for s in range(k)]
            cmds.append(self.conv_cmd(tag + ".dgrad", dyT, wd, K8, dx, dx.ld, x.H, x.W, Cin, CinPadN, taps, flags=flags))
        else:
            assert stride == 2 and k == 3 and pad == 1
            cls_taps = {0: [(1, 0)], 1: [(0, 1), (2, 0)]}  # parity -> [(r, offset)]
            for py in (0, 1):
                for px in (0, 1):
                    taps = [(oy, ox, r * 3 + s) for (r, oy) in cls_taps[py] for (s, ox) in cls_taps[px]]
                    gh, gw_ = (x.H - py + 1) // 2, (x.W - px + 1) // 2
                    cmds.append(self.conv_cmd(f"{tag}.dgrad{py}{px}", dyT, wd, K8, dx, dx.ld, x.H, x.W, Cin, CinPadN, taps,
                                              out_stride=2, out_oy=py, out_ox=px, gridH=gh, gridW=gw_, flags=flags))
        if x.C == Cin and Cin % 8 == 0:
            self.last_writer.setdefault(id(x.gbuf), []).append((x.coff, x.coff + x.C, cmds))

    def pred_conv(self, tag, x, weight, bias, wgrad, bgrad, preds, A, a0, c0, nch):
        """biased 1x1 prediction conv writing fp32 straight into preds[B][A][nch] at (anchor a0, channel c0)."""
        Cout, Cin = weight.shape[0], weight.shape[1]
        CoutPad = _rup(Cout, 32)
        wf = self.small(tag + ".wf", Cin * CoutPad * 2)
        need_dgrad = self.training and x.requires_grad
        wd = self.small(tag + ".wd", CoutPad * Cin * 2) if need_dgrad else None
        self.emit("PACK_W", i=[Cout, Cin, 1, 1, Cin, CoutPad, CoutPad, Cin], p=[weight, wf, wd], tag=tag + ".pack",
                  prologue=True)
        yptr = _Ptr(preds, (a0 * nch + c0) * 4)
        self.conv_cmd(tag + ".conv", x, wf, Cin // 8, yptr, nch, x.H, x.W, Cout, CoutPad, [(0, 0, 0)], bias=bias,
                      flags=L.MI_CONV_OUT_F32, y_nstride=A * nch)
        HW = x.H * x.W
        self.bias_jobs.append(dict(out=bgrad, a0=a0, HW=HW, c0=c0, nc=Cout, tag=tag))   # gathered by the loss backward

        def bwd():
            dmap = (self._new_buf(tag + ".dmap", x.N * HW * CoutPad * 2) if self.group_wgrad
                    else self.scratch("dpred_map", x.N * HW * CoutPad * 2))
            dT = TRef(dmap, x.N, x.H, x.W, CoutPad, CoutPad)
            self.emit("SPLIT_DPREDS", i=[x.N, A, nch, a0, HW, c0, Cout, CoutPad], p=[self.loss["dpreds"], dT],
                      tag=tag + ".split")
            self.wgrad_cmds(tag, x, dT, Cin, CoutPad, Cin, Cout, 1, 1, 0, wgrad)
            if need_dgrad:
                self.dgrad_cmds(tag, dT, wd, CoutPad // 8, x, Cin, Cin, 1, 1, 0)

        self.on_backward(bwd)

    def focus(self, image_ptr_holder, N, H, W):
        out = self.new_act(N, H // 2, W // 2, 16, "focus", requires_grad=False)
        u8 = int(torch.is_tensor(image_ptr_holder) and image_ptr_holder.dtype == torch.uint8)
        self.emit("FOCUS", i=[N, H, W, out.ld, u8], p=[image_ptr_holder, out], tag="focus")
        return out

    def upsample_into(self, tag, x, out):
        assert (out.H, out.W, out.C) == (2 * x.H, 2 * x.W, x.C)
        self.emit("UPSAMPLE_FWD", i=[x.ld, out.ld, x.N, x.H, x.W, x.C], p=[x, out], tag=tag)

        def bwd():
            assert self.grad_ready(out), tag
            acc = self.grad_mode(x)
            self.emit("UPSAMPLE_BWD", i=[out.ld, x.ld, acc, x.N, x.H, x.W, x.C], p=[out.grad, x.grad], tag=tag + ".bwd")

        self.on_backward(bwd)

    def spp_into(self, tag, x, o5, o9, o13):
        idx = self.small(tag + ".idx", 6 * x.npix * x.C)   # [dy codes x3][dx codes x3]
        assert o5.ld == o9.ld == o13.ld
        self.emit("SPP_FWD", i=[x.ld, o5.ld, x.N, x.H, x.W, x.C], p=[x, o5, o9, o13, idx], tag=tag)

        def bwd():
            acc = self.grad_mode(x)
            self.emit("SPP_BWD", i=[o5.ld, x.ld, acc, x.N, x.H, x.W, x.C],
                      p=[o5.grad, o9.grad, o13.grad, idx, x.grad], tag=tag + ".bwd")

        self.on_backward(bwd)

    def yolox_loss(self, preds, labels_t, anchors_t, B, A, ncls, max_labels, gmax, use_l1=False):
        nch = 5 + ncls
        nb = (A + 255) // 256
        ws = dict(
            cost=self.small("loss.cost", B * gmax * A * 4), iou=self.small("loss.iou", B * gmax * A * 4),
            match=self.small("loss.match", B * gmax * A), ngt=self.small("loss.ngt", B * 4),
            fg=self.small("loss.fg", B * A), matched_gt=self.small("loss.mgt", B * A * 4),
            matched_iou=self.small("loss.miou", B * A * 4), partial=self.small("loss.partial", nb * B * 4 * 4),
            out=self.small("loss.out", 8 * 4), gw=self.small("loss.gw", 5 * 4),
            partial_l1=self.small("loss.partial_l1", nb * B * 4),
            dpreds=self.small("loss.dpreds", B * A * nch * 4) if self.training else None)
        spec = ConvSpec(kind="loss", preds=_Ptr(preds), labels=_Ptr(labels_t), anchors=_Ptr(anchors_t), B=B, A=A,
                        ncls=ncls, max_labels=max_labels, gmax=gmax, ws=ws, use_l1=bool(use_l1))
        self.loss = ws
        self.loss["spec"] = spec
        self.emit("LOSS_FWD", desc=spec, tag="loss")

        def bwd():
            self.emit("LOSS_BWD", desc=spec, p=[None, ws["gw"], ws["dpreds"]], tag="loss.bwd")
            if self.bias_jobs:
                jobs = ConvSpec(kind="bias_jobs", jobs=list(self.bias_jobs))
                self.emit("BIAS_GRADS", i=[B, A, nch, len(self.bias_jobs)], desc=jobs,
                          p=[None, ws["dpreds"], self._new_buf("loss.bias_ws", 16 * 512 * 128 * 4)], tag="loss.bias_grads")

        self.on_backward(bwd)
        return ws

    # ---------------------------------------------------------------- finalize
    def finalize(self, materialize=True):
        # backward command generation, reverse order of forward emission
        self._emitting_bwd = True
        for fn, lane in reversed(self.bwd_gens):
            self.cur_lane = lane
            fn()
        self.cur_lane = 0
        self._emitting_bwd = False
        self.bwd_gens = []
        for which, lst in (("fwd", self.fwd), ("bwd", self.bwd)):
            b = self.shared.get("bn_acc_" + which)
            if b is not None and b.nbytes:
                nb = b.nbytes
                b.nbytes = _rup(nb, 256)
                lst.insert(0, _Cmd(L.OP["MEMSET"], i=[0], l=[nb], p=[_Ptr(b)], tag="bn_acc_zero." + which))
        wg = [c for c in self.bwd if c.op == L.OP["WGRAD"]]
        if self.group_wgrad and len(wg) >= 2:
            descs = (L.mi_wgrad_desc * len(wg))()
            for d, c in zip(descs, wg):
                C.memmove(C.byref(d), C.byref(self._wgrad_desc(c.desc)), C.sizeof(L.mi_wgrad_desc))
            meta = L.mi_wgrad_group()
            L.check(L.lib().mi_conv2d_wgrad_group_plan(descs, len(wg), None, None, 0, C.byref(meta)), "wgrad_group_plan")
            ws = self.scratch("wgrad_ws", 0)
            ws.nbytes = _rup(int(meta.ws_bytes), 256)   # replaces the per-layer maximum
            self.wgrad_group_ws = ws
        return Plan(self) if materialize else None


class Plan:
    def __init__(self, b, dry_run=False):
        """dry_run (tests only): materialise the command lists, descriptors and job tables against a HOST arena so that
        the host-side scheduling (grouped launches, gradient write ranges, all-reduce buckets) can be checked without a
        GPU; such a plan cannot be run - every executor entry point refuses without a device."""
        self.b = b
        if not (dry_run and b.device.type == "cpu"):
            L.require_device()
        off = 0
        for buf in b.bufs:
            buf.offset = off
            off += _rup(buf.nbytes, 256)
        self.arena_bytes = off
        self.arena = torch.zeros(off + 256, dtype=torch.uint8, device=b.device)
        base = self.arena.data_ptr()
        base = _rup(base, 256)
        for buf in b.bufs:
            buf.base = base
        self.descs = []
        self.cmd_descs = {}
        # (the weight pack and Focus as two graph branches measured 1.7 % slower, the option was removed: DESIGN.md §10)
        self.fwd_cmds, self.fwd_tags = self._materialize(self._batch_packs(b.prologue) + b.fwd, "fwd")
        self.graphs = {}
        # BatchNorm backward as one fused launch per layer or as reduce + apply: MI_BN_FUSED=1 / 0, default "auto" = both
        # backward lists are captured and timed ON THIS DEVICE and the faster one is kept.  (Measured: on most boxes of the
        # pool the fused form gains 2.3 % of the YOLOX-s step, on some - identical kernel timings in isolation, ~3 us more
        # per kernel boundary in the step - it loses 1 %.)
        mode = os.environ.get("MI_BN_FUSED")
        if mode is None:
            # data parallel: RCCL's kernels share the CUs with the backward pass and the fused kernel's grid barrier needs
            # every block resident - two-pass until the collective's footprint has been measured (MI_BN_FUSED=1 forces it)
            import torch.distributed as dist
            mode = "0" if (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1) else "auto"
        self.bn_fused = mode != "0"
        self.bn_fused_timing = None
        self._materialize_bwd()
        if (mode == "auto" and not dry_run and b.device.type == "cuda" and b.training
                and any(L.OPS[self.bwd_cmds[0][k].op] == "BN_BWD_FUSED" or
                        (L.OPS[self.bwd_cmds[0][k].op] == "BN_GROUP" and self.bwd_cmds[0][k].i[0] == 3)
                        for k in range(self.bwd_cmds[1]))):
            self._select_bn_backward()

    def check_bn_barriers(self):
        """raise if any grid barrier of the one-launch BatchNorm backward gave up since the last check (word 2 of a
        layer's barrier record; the kernel NaN-poisons what the timed-out block wrote).  Host-synchronising: called
        where the trainer reads the losses anyway."""
        if self.b.device.type != "cuda":
            return
        bars = [bf for bf in self.b.bufs if bf.name.endswith(".bar")]
        if not bars:
            return
        flags = torch.stack([self.buf_view(bf, torch.int32, 4)[2] for bf in bars])
        if int(flags.max()) != 0:
            bad = [bf.name for bf, f in zip(bars, flags.tolist()) if f]
            for bf in bars:
                self.buf_view(bf, torch.int32, 4)[2] = 0
            raise L.MI355Error(f"BatchNorm backward grid barrier timed out in {bad[:4]} ({len(bad)} layers): a block was not "
                               "resident (another kernel holds CUs?); set MI_BN_FUSED=0")

    def _materialize_bwd(self):
        b = self.b
        bwd = self._fuse_loss_bwd(self._batch_splits(b.bwd))
        if self.bn_fused:
            bwd = self._fuse_bn_bwd_pairs(bwd)
        self.bwd_cmds, self.bwd_tags = self._materialize(self._group_wgrads(bwd), "bwd")

    def _select_bn_backward(self, rounds=3, launches=4):
        """time the fused and the two-pass backward lists as hipGraphs (alternating, best mean of `rounds`) and keep the
        faster.  The replays only write buffers that every step overwrites (activation / parameter gradients, scratch)."""
        lib = L.lib()
        s = torch.cuda.Stream()
        sp = L.stream_ptr(s)
        best = {}
        handles = {}
        keep = {}
        for fused in (True, False):
            self.bn_fused = fused
            self._materialize_bwd()
            arr, n = self.bwd_cmds
            keep[fused] = (self.bwd_cmds, self.bwd_tags, self.cmd_descs["bwd"], self.cmd_members["bwd"],
                           list(self.wgrad_descs), list(getattr(self, "wgrad_stage_tags", [])), self.cmd_objs["bwd"])
            with torch.cuda.stream(s):
                L.check(lib.mi_cmdlist_run(arr, n, sp), "bn select: eager run")
                handles[fused] = L.check(lib.mi_graph_capture(arr, n, sp), "bn select: capture")
        with torch.cuda.stream(s):
            for r in range(rounds + 1):
                for fused in (True, False):
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(s)
                    for _ in range(launches):
                        L.check(lib.mi_graph_launch(handles[fused], sp), "bn select: launch")
                    e.record(s)
                    e.synchronize()
                    if r > 0:   # round 0 warms up
                        t = a.elapsed_time(e) / launches
                        best[fused] = min(best.get(fused, 1e9), t)
        for h in handles.values():
            lib.mi_graph_destroy(h)
        self.bn_fused_timing = dict(fused_ms=round(best[True], 4), two_pass_ms=round(best[False], 4))
        self.bn_fused = best[True] <= best[False]
        (self.bwd_cmds, self.bwd_tags, self.cmd_descs["bwd"], self.cmd_members["bwd"], self.wgrad_descs,
         self.wgrad_stage_tags, self.cmd_objs["bwd"]) = keep[self.bn_fused]

    def _group_wgrads(self, bwd):
        """all WGRAD commands become ONE grouped launch at the end of backward (mi_conv2d_wgrad_group_run) - or two when
        the builder asks for the split (data parallel): the head + neck layers' group is issued right after the last of
        their backward commands, the backbone's group at the end.  Both share the split-K workspace (they run one after
        the other on the stream)."""
        b = self.b
        wg = [c for c in bwd if c.op == L.OP["WGRAD"]]
        self.wgrad_descs = []
        if not (b.group_wgrad and len(wg) >= 2):
            return bwd
        stages, rest = [], list(wg)
        if b.wgrad_split:
            for pre in b.wgrad_stages:
                st = [c for c in rest if c.tag.startswith(tuple(pre))]
                if len(st) >= 2:
                    stages.append(st)
                    rest = [c for c in rest if not any(c is x for x in st)]
        if len(rest) < 2:          # nothing (or a single layer) left for the final group: fold the last stage back in
            if stages:
                rest = stages.pop() + rest
        pos = {id(c): i for i, c in enumerate(bwd)}
        issue_at = {max(pos[id(c)] for c in st): si for si, st in enumerate(stages)}
        out = []
        for i, c in enumerate(bwd):
            if c.op != L.OP["WGRAD"]:
                out.append(c)
            if i in issue_at:
                si = issue_at[i]
                out.append(self._wgrad_group_cmd(stages[si], "wgrad_group.early" if si == 0 else f"wgrad_group.stage{si}"))
        out.append(self._wgrad_group_cmd(rest, "wgrad_group"))
        self.wgrad_stage_tags = [[c.tag for c in st] for st in stages] + [[c.tag for c in rest]]
        return out

    def _wgrad_group_cmd(self, wg, tag):
        ws = self.b.wgrad_group_ws
        descs = (L.mi_wgrad_desc * len(wg))()
        for d, c in zip(descs, wg):
            t = PlanBuilder._wgrad_desc(c.desc)
            t.x, t.dy, t.gw = c.desc.x.resolve(), c.desc.dy.resolve(), c.desc.gw.resolve()
            C.memmove(C.byref(d), C.byref(t), C.sizeof(L.mi_wgrad_desc))
        meta = L.mi_wgrad_group()
        L.check(L.lib().mi_conv2d_wgrad_group_plan(descs, len(wg), ws.ptr, None, 0, C.byref(meta)), "wgrad_group_plan")
        assert meta.ws_bytes <= ws.nbytes, (meta.ws_bytes, ws.nbytes)
        host = (C.c_char * int(meta.table_bytes))()
        L.check(L.lib().mi_conv2d_wgrad_group_plan(descs, len(wg), ws.ptr, host, meta.table_bytes, C.byref(meta)),
                "wgrad_group_plan")
        table = self._upload_table(host, meta.table_bytes)
        self.descs += [meta, descs]
        self.wgrad_descs += list(descs)
        grp = _Cmd(L.OP["WGRAD_GROUP"], p=[_Ptr(C.addressof(meta)), _Ptr(table)], tag=tag)
        grp.group_descs = list(descs)
        grp.parts = list(wg)
        return grp

    def _fuse_bn_bwd_pairs(self, bwd):
        """BN_BWD_REDUCE + BN_BWD_APPLY of one layer -> ONE launch that keeps (da, y) in registers across a grid-wide
        barrier (mi_bn_act_bwd_fused): 3 tensor passes instead of 5."""
        RED, APP = L.OP["BN_BWD_REDUCE"], L.OP["BN_BWD_APPLY"]
        out, k = [], 0
        while k < len(bwd):
            c = bwd[k]
            n = bwd[k + 1] if k + 1 < len(bwd) else None
            if (c.op == RED and n is not None and n.op == APP and c.tag.endswith(".bnred")
                    and n.tag == c.tag[:-len(".bnred")] + ".bnapply" and len(n.p) > 12 and n.p[12].obj is not None):
                f = _Cmd(L.OP["BN_BWD_FUSED"], i=n.i, l=n.l, p=n.p, tag=c.tag[:-len(".bnred")] + ".bnbwd")
                f.lane = n.lane
                f.members = [c, n]
                out.append(f)
                k += 2
            else:
                out.append(c)
                k += 1
        return out

    def _batch_splits(self, bwd):
        """the out-gradient maps of all prediction convs (SPLIT_DPREDS, one per conv) in ONE launch right after the loss
        backward: every map has its own buffer (group_wgrad), so writing them early is safe"""
        sp = [c for c in bwd if c.op == L.OP["SPLIT_DPREDS"]]
        if not (self.b.group_wgrad and 2 <= len(sp) <= 16) or os.environ.get("MI_SPLIT_BATCH", "1") == "0":
            return bwd
        at = max(k for k, c in enumerate(bwd) if c.op in (L.OP["LOSS_BWD"], L.OP["BIAS_GRADS"]))
        assert all(k > at for k, c in enumerate(bwd) if c.op == L.OP["SPLIT_DPREDS"])
        B, A, nch = sp[0].i[:3]
        spec = ConvSpec(kind="split_jobs", jobs=[dict(dst=c.p[1], a0=c.i[3], HW=c.i[4], c0=c.i[5], nc=c.i[6], ld=c.i[7])
                                                 for c in sp])
        cmd = _Cmd(L.OP["SPLIT_DPREDS_BATCH"], i=[B, A, nch, len(sp)], p=[_Ptr(None), sp[0].p[0]], desc=spec,
                   tag="loss.split_all")
        cmd.lane = bwd[at].lane
        cmd.members = list(sp)
        rest = [c for c in bwd if c.op != L.OP["SPLIT_DPREDS"]]
        k = next(k for k, c in enumerate(rest) if c is bwd[at])
        return rest[:k + 1] + [cmd] + rest[k + 1:]

    def _fuse_loss_bwd(self, bwd):
        """LOSS_BWD + BIAS_GRADS + SPLIT_DPREDS_BATCH (three passes over the [B][A][5 + ncls] gradient: write, read, read)
        -> one LOSS_BWD_FUSED pass that writes the fp32 tensor, the prediction convs' bf16 out-gradient maps and the bias
        gradients' block sums together.  MI_LOSS_BWD_FUSED=0 keeps the three commands."""
        if os.environ.get("MI_LOSS_BWD_FUSED", "1") == "0":
            return bwd
        ops = [c.op for c in bwd]
        try:
            k = ops.index(L.OP["LOSS_BWD"])
        except ValueError:
            return bwd
        if ops[k + 1: k + 3] != [L.OP["BIAS_GRADS"], L.OP["SPLIT_DPREDS_BATCH"]]:
            return bwd
        lb, bg, sp = bwd[k: k + 3]
        B, A, nch = sp.i[:3]
        cells = sum(j["HW"] * j["nc"] for j in sp.desc.jobs)
        if cells != A * nch or len(sp.desc.jobs) > 16:       # the maps do not tile the gradient: keep the separate passes
            return bwd
        sj, bj = self._make_desc(sp.desc), self._make_desc(bg.desc)
        # the fp32 [B][A][5 + ncls] tensor itself has no consumer left; MI_LOSS_DPREDS=1 (the parity tests, which hand it to
        # the oracle's backward) keeps it
        keep = os.environ.get("MI_LOSS_DPREDS", "0") == "1"
        cmd = _Cmd(L.OP["LOSS_BWD_FUSED"], i=[len(sp.desc.jobs), len(bg.desc.jobs)], l=[bg.p[2].obj.nbytes // 4], desc=lb.desc,
                   p=[_Ptr(None), lb.p[1], lb.p[2] if keep else _Ptr(None), _Ptr(C.addressof(sj)), _Ptr(C.addressof(bj)), bg.p[2]],
                   tag="loss.bwd_fused")
        cmd.lane = getattr(lb, "lane", 0)
        cmd.members = [lb, bg] + list(sp.members)
        cmd.bias_jobs = bj
        return bwd[:k] + [cmd] + bwd[k + 3:]

    def _batch_packs(self, prologue):
        """all PACK_W commands of the prologue become ONE launch over a device job table"""
        packs = [c for c in prologue if c.op == L.OP["PACK_W"]]
        rest = [c for c in prologue if c.op != L.OP["PACK_W"]]
        if len(packs) < 2:
            return prologue
        jobs = (L.mi_pack_job * len(packs))()
        for j, c in zip(jobs, packs):
            Cout, Cin, KH, KW, CinPad, CoutPad, CoutPadK, CinPadN = c.i[:8]
            j.w, j.wf, j.wd = c.p[0].resolve(), c.p[1].resolve(), c.p[2].resolve()
            j.Cout, j.Cin, j.KK, j.CinPad, j.CoutPad, j.CoutPadK, j.CinPadN = Cout, Cin, KH * KW, CinPad, CoutPad, CoutPadK, CinPadN
        nblk = L.check(L.lib().mi_pack_jobs_layout(jobs, len(packs)), "pack_jobs_layout")
        tab = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(self.b.device)
        self.pack_table = tab
        cmd = _Cmd(L.OP["PACK_W_BATCH"], i=[len(packs), nblk, max(j.KK for j in jobs)], p=[_Ptr(tab)], tag="pack_all")
        cmd.parts = packs
        return rest + [cmd]

    def _make_desc(self, spec):
        kind = getattr(spec, "kind", "conv")
        if kind == "conv":
            d = L.mi_conv_desc()
            d.x, d.w, d.y = spec.x.resolve(), spec.w.resolve(), spec.y.resolve()
            d.bias, d.stats_acc = spec.bias.resolve(), spec.stats.resolve()
            for k in ("ldx", "ldy", "y_nstride", "N", "H", "W", "outH", "outW", "gridH", "gridW", "in_stride",
                      "out_stride", "out_oy", "out_ox", "K8", "Cout", "CoutPad", "flags", "stats_slots"):
                setattr(d, k, int(getattr(spec, k)))
            d.ntaps = len(spec.taps)
            for t, (dy, dx, w) in enumerate(spec.taps):
                d.tap_dy[t], d.tap_dx[t], d.tap_w[t] = dy, dx, w
            if getattr(spec, "tps", 0):
                d.TPS = int(spec.tps)       # taps per main-loop step forced by the plan (see _group_parity)
            xf = getattr(spec, "xf", None)
            if xf is not None:
                d.xf, d.xf_write, d.xf_C = xf.resolve(), int(spec.xf_write), int(spec.xf_C)
            bnb = getattr(spec, "bnb", None)
            if bnb is not None:
                d.bn_y, d.bn_ldy, d.bn_act = bnb["y"].resolve(), bnb["ldy"], bnb["act"]
                d.bn_scale, d.bn_shift = bnb["scale"].resolve(), bnb["shift"].resolve()
                d.bn_mean, d.bn_invstd = bnb["mean"].resolve(), bnb["invstd"].resolve()
        elif kind == "bias_jobs":
            d = (L.mi_bias_job * len(spec.jobs))()
            for jd, j in zip(d, spec.jobs):
                jd.out, jd.a0, jd.HW, jd.c0, jd.nc = j["out"].data_ptr(), j["a0"], j["HW"], j["c0"], j["nc"]
        elif kind == "split_jobs":
            d = (L.mi_split_job * len(spec.jobs))()
            for jd, j in zip(d, spec.jobs):
                jd.dst, jd.a0, jd.HW, jd.c0, jd.nc, jd.ld = j["dst"].resolve(), j["a0"], j["HW"], j["c0"], j["nc"], j["ld"]
        elif kind == "wgrad":
            d = PlanBuilder._wgrad_desc(spec)
            d.x, d.dy, d.gw = spec.x.resolve(), spec.dy.resolve(), spec.gw.resolve()
            d.ws, d.ws_bytes = spec.ws.ptr, spec.ws.nbytes
        else:
            d = L.mi_yolox_loss_desc()
            d.preds, d.labels, d.anchors = spec.preds.resolve(), spec.labels.resolve(), spec.anchors.resolve()
            d.B, d.A, d.ncls, d.max_labels, d.gmax = spec.B, spec.A, spec.ncls, spec.max_labels, spec.gmax
            for k in ("cost", "iou", "match", "ngt", "fg", "matched_gt", "matched_iou", "partial", "out", "partial_l1"):
                setattr(d, k, spec.ws[k].ptr)
            d.use_l1 = int(getattr(spec, "use_l1", False))
        self.descs.append(d)
        return d

    def _group_lanes(self, cmds):
        """parallel region = independent chains (lanes).  A list scheduler walks the chains in lock step: the op kind
        most lanes have next is issued for all of them at once - as ONE grouped launch when it is a convolution or a
        BatchNorm pass (CONV_GROUP / BN_GROUP), one command per lane otherwise.  Commands that write the same tensor
        (two data gradients accumulating into one input gradient) are never grouped and keep their original order.  The
        region's .begin / .end NOP markers are dropped."""
        NOP, CONV = L.OP["NOP"], L.OP["CONV"]
        BN_KIND = {L.OP["BN_ACT_FWD"]: 0, L.OP["BN_BWD_REDUCE"]: 1, L.OP["BN_BWD_APPLY"]: 2, L.OP["BN_BWD_FUSED"]: 3}

        def issue(cs, order):
            cs = sorted(cs, key=lambda c: order[id(c)])
            if len(cs) < 2:
                return cs
            if cs[0].op == CONV:
                # all lanes' convolutions of this position in one launch.  (History, measured with in-graph traces: mixing a
                # 3x3 level-0 job with the small levels first LOST 15 us per launch - the small maps' wide 3x40 tiles raised
                # the launch's LDS footprint past 80 KB and halved the occupancy of every block; mi_conv2d_group_plan now
                # picks tile shapes within the leading job's footprint and the same grouping gains 3 % of the step.
                # MI_GROUP_LONG=0 restores the conservative rule: jobs with more than two k-steps share a launch only if
                # the whole group fits one round of ~512 blocks.)
                parts = [cs]
                if os.environ.get("MI_GROUP_LONG", "1") == "0":
                    def nblocks(c):
                        d = self._make_desc(c.desc)
                        self.descs.pop()
                        n_ = L.lib().mi_conv2d_plan(C.byref(d))
                        return max(n_, 1) * (d.CoutPad // d.BN), (d.K8 * 8 // d.KC) * (d.ntaps // d.TPS)
                    info = [nblocks(c) for c in cs]
                    if not all(st <= 2 for _, st in info):
                        parts, cur, tot = [], [], 0
                        for c, (nb_, _) in sorted(zip(cs, info), key=lambda t: t[1][0]):
                            if nb_ >= 384 or tot + nb_ > 640:
                                if cur:
                                    parts.append(cur)
                                cur, tot = [], 0
                            if nb_ >= 384:
                                parts.append([c])
                            else:
                                cur.append(c)
                                tot += nb_
                        if cur:
                            parts.append(cur)
                res = []
                for part in parts:
                    part = sorted(part, key=lambda c: order[id(c)])
                    g = self._conv_group_cmd(part) if len(part) >= 2 else None
                    res += [g] if g is not None else part
                return res
            if cs[0].op in BN_KIND:
                # bandwidth-sized jobs (> 512 blocks) per shared launch: round 3 measured two of them together slower than apart
                # and kept one; re-measured at the end of round 6 (same box, three interleaved rounds): two 5.385 ms, one 5.411,
                # all 5.391 - two it is (the head's level-0 cls / reg tower BatchNorms share their launch)
                def bn_blocks(c):
                    npix, Cc = (c.l[1], c.i[3]) if cs[0].op == L.OP["BN_ACT_FWD"] else (c.l[0], c.i[3] if cs[0].op == L.OP["BN_BWD_REDUCE"] else c.i[5])
                    return npix * (Cc // 8) / 2048
                big = [c for c in cs if bn_blocks(c) > 512]
                small = [c for c in cs if bn_blocks(c) <= 512]
                nbig = int(os.environ.get("MI_BN_GROUP_BIG", "2"))
                parts = [small + big[:nbig]] + [[c] for c in big[nbig:]]
                res = []
                for part in parts:
                    part = sorted(part, key=lambda c: order[id(c)])
                    g = self._bn_group_cmd(BN_KIND[cs[0].op], part) if len(part) >= 2 else None
                    res += [g] if g is not None else part
                return res
            return cs

        out, k = [], 0
        while k < len(cmds):
            c = cmds[k]
            if not (c.op == NOP and c.tag.endswith(".begin")):
                out.append(c)
                k += 1
                continue
            e = k + 1
            while not (cmds[e].op == NOP and cmds[e].tag.endswith(".end")):
                e += 1
            region = cmds[k + 1: e]
            order = {id(r): i for i, r in enumerate(region)}
            lanes = sorted({r.lane for r in region})
            skip = os.environ.get("MI_GROUP_SKIP", "")
            if not self.b.group_lanes or len(lanes) < 2 or (skip and any(t and t in c.tag for t in skip.split(","))):
                out += region
            else:
                for cs in schedule_lanes(region):
                    out += issue(cs, order)
            k = e + 1
        return out

    def _group_parity(self, cmds):
        """the data gradient of a stride-2 3x3 conv is four launches, one per output-pixel parity class (1, 2, 2 and 4
        taps); they write disjoint pixels of the same tensor, so they share ONE grouped launch (4-tap class first - its
        blocks run longest - when the group's kernel configuration allows it)"""
        if not self.b.group_lanes or os.environ.get("MI_GROUP_PARITY", "1") == "0":
            return cmds
        out, k, CONV = [], 0, L.OP["CONV"]
        while k < len(cmds):
            run = cmds[k:k + 4]
            base = cmds[k].tag[:-2] if cmds[k].op == CONV and cmds[k].tag.endswith(".dgrad00") else None
            if base and len(run) == 4 and all(c.op == CONV and c.tag == base + s and c.lane == run[0].lane
                                              for c, s in zip(run, ("00", "01", "10", "11"))):
                g = self._conv_group_cmd(run[::-1], tag=base + "(4 classes)") or self._conv_group_cmd(run, tag=base + "(4 classes)")
                if g is None and os.environ.get("MI_GROUP_PARITY_TPS1", "1") != "0":
                    # K = 256 / 512 (dark5.0, bu_conv1): the 4-tap class picks two taps per step, which the 1-tap class cannot
                    # follow - one tap per step for all four classes lets them share a launch (was four launches of 8-18 us)
                    one = []
                    for c in run[::-1]:
                        sp = ConvSpec(**c.desc.__dict__)
                        sp.tps = 1
                        nc = _Cmd(c.op, c.i, c.f, c.p, c.l, sp, c.tag)
                        nc.lane = c.lane
                        one.append(nc)
                    g = self._conv_group_cmd(one, tag=base + "(4 classes)")
                if g is not None:
                    g.lane = run[0].lane
                    out.append(g)
                    k += 4
                    continue
            out.append(cmds[k])
            k += 1
        return out

    def _upload_table(self, host, nbytes):
        t = torch.frombuffer(bytearray(bytes(host)[:nbytes]), dtype=torch.uint8).to(self.b.device)
        self.descs.append(t)
        return t

    def _conv_group_cmd(self, cs, tag=None):
        n = len(cs)
        descs = (L.mi_conv_desc * n)()
        keep = [self._make_desc(c.desc) for c in cs]
        for d, t in zip(descs, keep):
            C.memmove(C.byref(d), C.byref(t), C.sizeof(L.mi_conv_desc))
        meta = L.mi_conv_group()
        lib = L.lib()
        if lib.mi_conv2d_group_plan(descs, n, None, 0, C.byref(meta)) < 0:
            lib.mi_last_error()
            return None     # shapes that do not share a kernel configuration stay separate launches
        host = (C.c_char * int(meta.table_bytes))()
        L.check(lib.mi_conv2d_group_plan(descs, n, host, meta.table_bytes, C.byref(meta)), "conv_group_plan")
        tab = self._upload_table(host, meta.table_bytes)
        self.descs += [meta, descs]
        g = _Cmd(L.OP["CONV_GROUP"], p=[_Ptr(C.addressof(meta)), _Ptr(tab)], tag=tag or "+".join(c.tag for c in cs))
        g.group_descs = list(descs)
        g.members = list(cs)
        return g

    def _bn_group_cmd(self, kind, cs):
        n = len(cs)
        jobs = (L.mi_bn_job * n)()
        for j, c in zip(jobs, cs):
            P = [x.resolve() for x in c.p]
            if kind == 0:
                self._fill_bn_fwd_job(j, c)
            elif kind == 1:  # BN_BWD_REDUCE: i=[ldda, ldy, nblk, C, act, nslots] l=[npix]
                j.da, j.y, j.scale, j.shift, j.mean, j.invstd, j.acc = P[:7]
                j.ldda, j.ldy, j.nblk, j.C, j.act, j.nslots = c.i[:6]
                j.npix = j.count = c.l[0]
            else:            # BN_BWD_APPLY / BN_BWD_FUSED: i=[ldda, ldy, lddy, lddres, dres_acc, C, act, nslots] l=[count, npix]
                (j.da, j.y, j.scale, j.shift, j.mean, j.invstd, j.gamma, j.acc, j.dgamma, j.dbeta, j.dy,
                 j.dres) = P[:12]
                j.bar = P[12] if kind == 3 else None
                j.ldda, j.ldy, j.lddy, j.lddres, j.dres_accum, j.C, j.act, j.nslots = c.i[:8]
                j.npix, j.count = c.l[0], c.l[1]
        meta = L.mi_bn_group()
        lib = L.lib()
        if lib.mi_bn_group_plan(kind, jobs, n, None, 0, C.byref(meta)) < 0:
            lib.mi_last_error()
            return None
        host = (C.c_char * int(meta.table_bytes))()
        L.check(lib.mi_bn_group_plan(kind, jobs, n, host, meta.table_bytes, C.byref(meta)), "bn_group_plan")
        tab = self._upload_table(host, meta.table_bytes)
        self.descs += [meta, jobs]
        g = _Cmd(L.OP["BN_GROUP"], i=[kind, n], p=[_Ptr(C.addressof(meta)), _Ptr(tab)], tag="+".join(c.tag for c in cs))
        g.group_jobs = list(jobs)
        g.members = list(cs)
        return g

    # ---------------------------------------------------------------- BatchNorm + SiLU in the consumer
    @staticmethod
    def _cmd_bufs(c):
        """ids of the arena buffers a (possibly merged) command touches"""
        out = set()

        def add(o):
            if isinstance(o, _Ptr):
                o = o.obj
            if isinstance(o, TRef):
                out.add(id(o.buf))
                if o.gbuf is not None:
                    out.add(id(o.gbuf))
            elif isinstance(o, Buf):
                out.add(id(o))

        for m in (getattr(c, "members", None) or [c]):
            for x in m.p:
                add(x)
            if m.desc is not None:
                for v in m.desc.__dict__.values():
                    if isinstance(v, dict):
                        for w in v.values():
                            add(w)
                    else:
                        add(v)
        return out

    def _defer_bn(self, cmds):
        """BatchNorm(train) + SiLU of a layer applied by the layer's FIRST reader instead of a launch of its own
        (MI_BN_IN_CONSUMER=0 keeps every BN_ACT_FWD).  A BN_ACT_FWD job (alone or inside a BN_GROUP) without a residual
        whose output tensor is first read - whole, as the input view - by a forward convolution launch that runs on the
        streaming 1x1 / weight-stationary 3x3 kernel is dropped; that launch reads the raw conv output y instead, derives
        scale / shift from the accumulators in its prologue, rewrites the tiles it fetched in LDS and stores the activated
        tensor for the later readers (csrc/conv_bn.h BnXf; mi_conv_desc.xf).  All members of a grouped launch convert
        together or not at all.  Bit-identical to the two-launch form (same expression, same rounding point); the builder's
        own lists are not touched (tests/plan_interp.py keeps interpreting BaseConv as conv, BatchNorm, conv)."""
        self.deferred_bn = []
        mode = os.environ.get("MI_BN_IN_CONSUMER", "auto")
        if mode == "0" or not self.b.bn_train:
            return cmds

        def pays(sp, x):
            """MI_BN_IN_CONSUMER=auto (default): only where the fold measured FASTER than the launch it removes (same-box
            in-graph traces, profiles/r05_bn_in_consumer_ab.txt).  SiLU costs two quarter-rate transcendentals per element
            and a consumer launch of this network is a serial chain of one or two tiles per block, so the transform adds
            its whole latency to the chain: 3x3 readers (halo pixels transformed 1.3 - 2.6 times, 7 - 35 us added against
            6 - 21 us removed) and the 20x20 / 40x40 maps (6 - 11 us added against 6 - 8 us) LOSE; the streaming 1x1
            readers of the large maps and the K = 32 stride-2 stem win 2 - 8 us each.  MI_BN_IN_CONSUMER=1 converts every
            eligible layer."""
            if mode != "auto":
                return True
            k3 = len(sp.taps) == 9
            elems = x.N * x.H * x.W * x.C
            if k3:
                return sp.in_stride == 2 and x.C == 32
            return x.C <= 128 and elems >= 6_000_000
        only = [t for t in os.environ.get("MI_BN_IN_CONSUMER_ONLY", "").split(",") if t]   # substrings of BatchNorm tags (A/B runs)
        CONV, CONVG, BNF, BNG = L.OP["CONV"], L.OP["CONV_GROUP"], L.OP["BN_ACT_FWD"], L.OP["BN_GROUP"]
        lib = L.lib()
        pending = {}        # (buf id, coff) of an activation -> (container command, symbolic BN_ACT_FWD command)
        drop = {}           # id(container) -> [symbolic BN commands taken out of it]
        replace = {}        # id(conv launch) -> new command

        def bn_jobs(c):
            if c.op == BNF:
                return [(c, c)]
            if c.op == BNG and c.i[0] == 0:
                return [(c, m) for m in c.members]
            return []

        def try_convert(c):
            members = [c] if c.op == CONV else list(c.members)
            picks = []
            for m in members:
                sp = m.desc
                x = sp.x.obj
                if getattr(sp, "kind", "conv") != "conv" or not isinstance(x, TRef) or sp.x.off or getattr(sp, "xf", None) is not None:
                    return None
                ent = pending.get((id(x.buf), x.coff))
                if ent is None or sp.stats.obj is None or sp.flags or sp.bias.obj is not None:
                    return None
                bn = ent[1]
                out, y = bn.p[12].obj, bn.p[0].obj
                Cc = bn.i[3]
                if not (out.C == Cc == sp.K8 * 8 == x.C and x.ld == out.ld and isinstance(y, TRef) and y.C == Cc
                        and (x.N, x.H, x.W) == (y.N, y.H, y.W)):
                    return None
                if (only and not any(t in bn.tag for t in only)) or not pays(sp, x):
                    return None
                picks.append((m, ent))
            # one device record per input tensor
            keys = []
            for m, ent in picks:
                if id(ent[1]) not in [id(k_) for k_ in keys]:
                    keys.append(ent[1])
            recs = (L.mi_bnx * len(keys))()
            for r, bn in zip(recs, keys):
                P = [q.resolve() for q in bn.p]
                (_, r.acc, r.gamma, r.beta, r.rmean, r.rvar, r.nbt, r.scale, r.shift, r.mean, r.invstd, _, r.a) = P[:13]
                out = bn.p[12].obj
                r.lda, r.act, r.C, r.nslots = out.ld, bn.i[4], bn.i[3], bn.i[5]
                r.sld = _rup(bn.i[3], 32) * 2
                cnt = bn.l[0]
                r.inv_count = 1.0 / cnt
                r.unbias = cnt / (cnt - 1.0) if cnt > 1 else 1.0
                r.eps, r.momentum = (bn.f + [0.0, 0.0])[:2]
            tab = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(self.b.device)
            new, seen = [], set()
            for m, ent in picks:
                bn = ent[1]
                y = bn.p[0].obj
                sp = ConvSpec(**m.desc.__dict__)
                sp.x, sp.ldx = _Ptr(y), y.ld
                sp.xf = _Ptr(tab, C.sizeof(L.mi_bnx) * [id(k_) for k_ in keys].index(id(bn)))
                sp.xf_write, sp.xf_C = int(id(bn) not in seen), bn.i[3]
                sp.xf_bn = bn       # (the symbolic BN_ACT_FWD behind the record: tests/plan_interp.py)
                seen.add(id(bn))
                nm = _Cmd(m.op, m.i, m.f, m.p, m.l, sp, m.tag)
                nm.lane = m.lane
                new.append(nm)
            if c.op == CONV:
                d = self._make_desc(new[0].desc)
                self.descs.pop()
                if lib.mi_conv2d_route(C.byref(d)) not in (1, 2):
                    return None
                res = new[0]
            else:
                res = self._conv_group_cmd(new, tag=c.tag)
                if res is None:
                    return None
                res.lane = c.lane
            self.descs.append(tab)
            res.deferred_bn = [ent[1] for _, ent in picks]
            return res, picks

        for c in cmds:
            refs = self._cmd_bufs(c)
            if c.op in (CONV, CONVG) and pending:
                got = try_convert(c)
                if got is not None:
                    res, picks = got
                    replace[id(c)] = res
                    done = set()
                    for _, (cont, bn) in picks:
                        if id(bn) not in done:
                            done.add(id(bn))
                            drop.setdefault(id(cont), []).append(bn)
                            self.deferred_bn.append(bn.tag)
            for key in [k_ for k_, ent in pending.items() if k_[0] in refs]:
                del pending[key]
            for cont, bn in bn_jobs(c):
                out = bn.p[12].obj
                if bn.p[1].obj is not None and bn.p[11].obj is None and isinstance(out, TRef) and bn.i[3] % 32 == 0:
                    pending[(id(out.buf), out.coff)] = (cont, bn)
        if not replace:
            return cmds
        out = []
        for c in cmds:
            if id(c) in replace:
                out.append(replace[id(c)])
            elif id(c) in drop:
                rest = [m for m in (c.members if c.op == BNG else [c]) if not any(m is d_ for d_ in drop[id(c)])]
                if len(rest) >= 2:
                    g = self._bn_group_cmd(0, rest)
                    if g is None:
                        out += rest
                    else:
                        g.lane = c.lane
                        out.append(g)
                else:
                    out += rest
            else:
                out.append(c)
        return out

    @staticmethod
    def _fill_bn_fwd_job(j, c):
        """BN_ACT_FWD command -> mi_bn_job: i=[ldy, ldres, lda, C, act, nslots] l=[count, npix] f=[eps, momentum]"""
        P = [x.resolve() for x in c.p]
        (j.y, j.acc, j.gamma, j.beta, j.rmean, j.rvar, j.nbt, j.scale, j.shift, j.mean, j.invstd, j.res, j.a) = P[:13]
        j.ldy, j.ldres, j.lda, j.C, j.act, j.nslots = c.i[:6]
        j.count, j.npix = c.l[0], c.l[1]
        j.eps, j.momentum = (c.f + [0.0, 0.0])[:2]

    def _materialize(self, cmds, which):
        cmds = self._group_lanes(self._group_parity(cmds))
        if which == "fwd":
            cmds = self._defer_bn(cmds)
        arr = (L.mi_cmd * max(1, len(cmds)))()
        tags = []
        if which == "fwd":
            self.fwd_list = cmds
        self.cmd_descs[which] = [None] * len(cmds)
        # symbolic builder commands behind a merged launch (None: the command is its own member); tests/plan_interp.py runs those.
        # `parts`: the members of a launch whose operands live in a device job table only (PACK_W_BATCH, WGRAD_GROUP) - kept
        # out of `members`, which _cmd_bufs / _defer_bn read
        self.cmd_members = getattr(self, "cmd_members", {})
        self.cmd_members[which] = [getattr(c, "members", None) or getattr(c, "parts", None) for c in cmds]
        self.cmd_objs = getattr(self, "cmd_objs", {})
        self.cmd_objs[which] = list(cmds)
        for k, c in enumerate(cmds):
            m = arr[k]
            m.op = c.op
            for j, v in enumerate(c.i):
                m.i[j] = int(v)
            for j, v in enumerate(c.f):
                m.f[j] = float(v)
            for j, v in enumerate(c.l):
                m.l[j] = int(v)
            for j, v in enumerate(c.p):
                m.p[j] = v.resolve()
            if c.desc is not None:
                d = self._make_desc(c.desc)
                m.p[0] = C.cast(C.pointer(d), C.c_void_p).value
                self.cmd_descs[which][k] = d
            elif hasattr(c, "group_descs"):
                self.cmd_descs[which][k] = c.group_descs
            elif hasattr(c, "group_jobs"):
                self.cmd_descs[which][k] = c.group_jobs
            tags.append(c.tag)
        return (arr, len(cmds)), tags

    # ---------------------------------------------------------------- execution
    def run(self, which, stream=None):
        arr, n = self.fwd_cmds if which == "fwd" else self.bwd_cmds
        L.check(L.lib().mi_cmdlist_run(arr, n, L.stream_ptr(stream)), f"plan.{which}")

    def capture(self, which, stream):
        arr, n = self.fwd_cmds if which == "fwd" else self.bwd_cmds
        h = L.lib().mi_graph_capture(arr, n, L.stream_ptr(stream))
        L.check(h, f"graph_capture.{which}")
        self.graphs[which] = h
        return h

    def launch(self, which, stream=None):
        L.check(L.lib().mi_graph_launch(self.graphs[which], L.stream_ptr(stream)), f"graph_launch.{which}")

    def time_cmds(self, which, iters=3, stream=None):
        """per-command HIP-event timings (ms) -> list of (tag, ms)"""
        arr, n = self.fwd_cmds if which == "fwd" else self.bwd_cmds
        tags = self.fwd_tags if which == "fwd" else self.bwd_tags
        per = (C.c_float * max(1, n))()
        tot = C.c_float(0)
        L.check(L.lib().mi_cmdlist_time(arr, n, iters, C.byref(tot), per, L.stream_ptr(stream)), "cmdlist_time")
        return tot.value, [(tags[k], per[k]) for k in range(n)]

    # ---------------------------------------------------------------- conv autotuning
    def _time_list(self, which, iters, sp):
        arr, n = self.fwd_cmds if which == "fwd" else self.bwd_cmds
        per = (C.c_float * max(1, n))()
        L.check(L.lib().mi_cmdlist_time(arr, n, iters, None, per, sp), "cmdlist_time")
        return per

    @staticmethod
    def _valid_cfg(d0, cfg):
        d = L.mi_conv_desc.from_buffer_copy(d0)
        d.KC, d.BN, d.TH, d.TW, d.TPS = cfg
        if L.lib().mi_conv2d_plan(C.byref(d)) < 0:
            return None
        return (d.KC, d.BN, d.TH, d.TW, d.TPS)

    def autotune_convs(self, iters=5, stream=None, verbose=False, min_gain=0.03):
        """choose (pixel tile, cout tile, k-chunk, taps per step) of every conv launch by timing candidates ON THE
        DEVICE, IN SEQUENCE: the whole forward / backward list is replayed command by command (HIP events around
        each launch) with candidate r applied to every conv at once, so each conv sees the cache state its producer
        leaves behind - timing a conv in isolation (operands L2-hot) prefers big-LDS, low-occupancy configurations
        that lose inside the step.  Phase A varies the tiles with the heuristic k-chunk, phase B the k-chunk / taps per
        step on the chosen tile.  Must run before the lists are captured into graphs; the replays only write buffers
        that every step overwrites, plus BN running statistics (saved and restored here)."""
        lib, sp = L.lib(), L.stream_ptr(stream)
        lib.mi_last_error()
        saved = [(t, t.clone()) for t in getattr(self.b, "tune_restore", [])]
        convs = {}
        for which in ("fwd", "bwd"):
            arr, n = self.fwd_cmds if which == "fwd" else self.bwd_cmds
            convs[which] = [k for k in range(n) if arr[k].op == L.OP["CONV"]]
        report = {}

        def phase(gen):
            for which in ("fwd", "bwd"):
                idx = convs[which]
                descs = self.cmd_descs[which]
                cur = {k: (descs[k].KC, descs[k].BN, descs[k].TH, descs[k].TW, descs[k].TPS) for k in idx}
                cands = {}
                for k in idx:
                    base = self._valid_cfg(descs[k], cur[k])
                    lst = []
                    for c in gen(descs[k], base):
                        v = self._valid_cfg(descs[k], c)
                        if v is not None and v != base and v not in lst:
                            lst.append(v)
                    cands[k] = [base] + lst
                R = max(len(v) for v in cands.values())
                best = {k: (None, None) for k in idx}
                t0 = {}
                for r in range(R):
                    for k in idx:
                        c = cands[k][r] if r < len(cands[k]) else cands[k][0]
                        descs[k].KC, descs[k].BN, descs[k].TH, descs[k].TW, descs[k].TPS = c
                    per = self._time_list(which, iters, sp)
                    for k in idx:
                        if r < len(cands[k]):
                            t = per[k]
                            if r == 0:
                                t0[k] = t
                                best[k] = (t, cands[k][0])
                            elif t < best[k][0] and t < (1.0 - min_gain) * t0[k]:
                                best[k] = (t, cands[k][r])
                # validation: candidates won a noisy one-shot comparison (winner's curse) - replay base and winners
                # alternately and keep a winner only if it is still ahead on the means
                tb, tw = {k: 0.0 for k in idx}, {k: 0.0 for k in idx}
                rounds = 3
                for _ in range(rounds):
                    for cfgs, acc in ((cands, None), (best, tw)):
                        for k in idx:
                            c = cands[k][0] if acc is None else best[k][1]
                            descs[k].KC, descs[k].BN, descs[k].TH, descs[k].TW, descs[k].TPS = c
                        per = self._time_list(which, iters, sp)
                        for k in idx:
                            (tb if acc is None else tw)[k] += per[k] / rounds
                for k in idx:
                    keep = best[k][1] != cands[k][0] and tw[k] < (1.0 - min_gain) * tb[k]
                    c = best[k][1] if keep else cands[k][0]
                    descs[k].KC, descs[k].BN, descs[k].TH, descs[k].TW, descs[k].TPS = c
                    first = report[(which, k)][0] if (which, k) in report else tb[k]
                    report[(which, k)] = (first, tw[k] if keep else tb[k], c)

        def gen_tiles(d, base):
            tiles = [(8, 16), (4, 32), (8, 8), (4, 16)]
            if d.gridH * d.gridW <= 1600:
                tiles += [(3, 40), (6, 20), (5, 20), (3, 20), (2, 20)]
            for th, tw in tiles:
                if tw > 2 * d.gridW:
                    continue
                for bn in (32, 64, 128):
                    if d.CoutPad % bn == 0:
                        yield (0, bn, th, tw, 0)

        def gen_k(d, base):
            K = d.K8 * 8
            for kc in (128, 64, 32, 16):
                if K % kc:
                    continue
                for tps in range(d.ntaps, 0, -1):
                    if d.ntaps % tps == 0:
                        yield (kc, base[1], base[2], base[3], tps)

        phase(gen_tiles)
        phase(gen_k)
        for t, v in saved:
            t.copy_(v)
        auto = sum(v[0] for v in report.values()) * 1e3
        tuned = sum(v[1] for v in report.values()) * 1e3
        if verbose:
            for (which, k), v in sorted(report.items()):
                tag = (self.fwd_tags if which == "fwd" else self.bwd_tags)[k]
                print(f"[tune] {which} {tag:40s} {v[0] * 1e3:7.1f} -> {v[1] * 1e3:7.1f} us  {v[2]}", flush=True)
        return auto, tuned

    def view(self, t, dtype=torch.bfloat16):
        """torch view of a TRef (for tests / module outputs): shape [N,C,H,W] with channels_last strides"""
        base = self.arena.data_ptr()
        off = t.ptr - base
        es = 2
        flat = self.arena[off: off + ((t.npix - 1) * t.ld + t.C) * es].view(dtype)
        return flat.as_strided((t.N, t.C, t.H, t.W), (t.H * t.W * t.ld, 1, t.W * t.ld, t.ld))

    def buf_view(self, buf, dtype, numel=None):
        base = self.arena.data_ptr()
        off = buf.ptr - base
        es = torch.empty((), dtype=dtype).element_size()
        n = buf.nbytes // es if numel is None else numel
        return self.arena[off: off + n * es].view(dtype)

    def __del__(self):
        try:
            for h in self.graphs.values():
                L.lib().mi_graph_destroy(h)
        except Exception:
            pass
