"""TEST INFRASTRUCTURE: a CPU interpreter of the symbolic step plan (yolov7_d2_amd.plan.PlanBuilder).

It executes the forward / backward command lists with torch CPU ops over byte buffers laid out exactly as
the plan lays them out (bf16 NHWC views, concat slices, gradient mirrors, packed weight images, tap
tables, accumulate flags).  It checks the HOST LOGIC of the product (graph wiring, buffer aliasing,
gradient fan-in, dgrad parity classes, weight packing) against the oracle without a GPU; the kernels
themselves are checked on the GPU by the `-m gpu` tests.  Lives under tests/: never imported by the
product.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import yolox_oracle as O  # noqa: E402

from yolov7_d2_amd import _lib as L  # noqa: E402
from yolov7_d2_amd.plan import Buf, TRef  # noqa: E402

OPN = {v: k for k, v in L.OP.items()}


class Interp:
    def __init__(self, builder, dtype=torch.bfloat16):
        """dtype=torch.float32 stores activations / weight images in fp32 (same element strides): separates
        host-logic errors from bf16 storage noise."""
        self.b = builder
        self.dt = dtype
        self.mul = 2 if dtype == torch.float32 else 1
        self.store = {}
        self.tmap = {}     # id(device tensor) -> (tensor, host mirror): see T()
        # id(buf) -> the device's bytes of that buffer AFTER the command: the statistics epilogues of a convolution sum the
        # values the device stored, so the teacher-forced check takes them from those (the stored tensor itself is
        # compared on its own)
        self.dev_out = {}
        # id(buf) -> fp32 magnitudes [nbytes / 2] of the OPERANDS of an accumulating bf16 store (max |old|, |new|): a sum that
        # cancels is exact to a rounding of its operands, not of itself (tests/plan_compare.py sizes its ulps by these)
        self.mag = {}

    # ---- host mirrors of device state (tests/test_gpu_plan_commands.py: teacher forcing per command)
    def T(self, o):
        """the tensor the interpreter reads / writes for a command operand: a CPU tensor itself, a device tensor's host
        mirror (copied on first use; reset() drops them)"""
        if not isinstance(o, torch.Tensor) or o.device.type == "cpu":
            return o
        e = self.tmap.get(id(o))
        if e is None:
            e = (o, o.detach().to("cpu", copy=True))
            self.tmap[id(o)] = e
        return e[1]

    def mirror(self, buf, data):
        """host copy of an arena buffer's bytes (uint8, buf.nbytes long): the interpreter's storage of that buffer"""
        s = torch.zeros(buf.nbytes * self.mul + 64, dtype=torch.uint8)
        s[: data.numel()] = data
        self.store[id(buf)] = s

    def reset(self):
        self.store.clear()
        self.tmap.clear()
        self.dev_out = {}
        self.mag = {}

    def tv_stored(self, t, C=None):
        """tv(), from the device's stored bytes when they are given (dev_out)"""
        d = self.dev_out.get(id(t.buf))
        if d is None:
            return self.tv(t, C)
        C = t.C if C is None else C
        return d.view(self.dt).as_strided((t.N, t.H, t.W, C), (t.H * t.W * t.ld, t.W * t.ld, t.ld, 1), t.coff)

    # ---- storage
    def raw(self, buf):
        s = self.store.get(id(buf))
        if s is None or s.numel() < buf.nbytes * self.mul:
            s = torch.zeros(buf.nbytes * self.mul + 64, dtype=torch.uint8)
            self.store[id(buf)] = s
        return s

    def tv(self, t, C=None):
        """bf16 NHWC view [N,H,W,C] of a TRef"""
        C = t.C if C is None else C
        flat = self.raw(t.buf).view(self.dt)
        return flat.as_strided((t.N, t.H, t.W, C), (t.H * t.W * t.ld, t.W * t.ld, t.ld, 1), t.coff)

    def f32(self, p, n, off_bytes=0):
        o = p.obj
        if o is None:
            return None
        if isinstance(o, torch.Tensor):
            o = self.T(o)
            return o.view(-1)[:n] if p.off == 0 else o.view(-1)[p.off // 4: p.off // 4 + n]
        assert isinstance(o, Buf), type(o)
        return self.raw(o).view(torch.float32)[(p.off + off_bytes) // 4: (p.off + off_bytes) // 4 + n]

    def f64(self, p, n):
        assert isinstance(p.obj, Buf) and p.off % 8 == 0
        return self.raw(p.obj).view(torch.float64)[p.off // 8: p.off // 8 + n]

    def rawbytes(self, p, n):
        o = p.obj
        if isinstance(o, torch.Tensor):
            return self.T(o).view(torch.uint8).view(-1)[p.off: p.off + n]
        return self.raw(o)[p.off: p.off + n]

    # ---- ops
    def run(self, cmds):
        for c in cmds:
            getattr(self, "op_" + OPN[c.op])(c)

    @staticmethod
    def members(c):
        """the symbolic builder commands behind a (possibly merged, possibly nested) materialised command, in order"""
        ms = getattr(c, "members", None) or getattr(c, "parts", None)
        return [x for m in ms for x in Interp.members(m)] if ms else [c]

    def run_materialized(self, plan, which, lo=0, hi=None):
        """commands lo..hi of a materialised list (Plan.cmd_objs): each one's members in order"""
        cmds = plan.cmd_objs[which]
        for c in cmds[lo: len(cmds) if hi is None else hi]:
            self.run(self.members(c))

    def op_NOP(self, c):
        pass

    def op_MEMSET(self, c):
        self.rawbytes(c.p[0], c.l[0]).fill_(c.i[0])

    def op_PACK_W(self, c):
        Cout, Cin, KH, KW, CinPad, CoutPad, CoutPadK, CinPadN = c.i[:8]
        w = self.T(c.p[0].obj).detach().float().reshape(Cout, Cin, KH * KW)
        KK = KH * KW
        if c.p[1].obj is not None:  # wf[tap][ci/8][co][ci%8]
            img = torch.zeros(KK, CinPad // 8, CoutPad, 8)
            wp = torch.zeros(KK, CoutPad, CinPad)
            wp[:, :Cout, :Cin] = w.permute(2, 0, 1)
            img[:] = wp.view(KK, CoutPad, CinPad // 8, 8).permute(0, 2, 1, 3)
            o = c.p[1].off // 2
            self.raw(c.p[1].obj).view(self.dt)[o: o + img.numel()] = img.reshape(-1).to(self.dt)
        if c.p[2].obj is not None:  # wd[tap][co/8][ci][co%8]
            wp = torch.zeros(KK, CinPadN, CoutPadK)
            wp[:, :Cin, :Cout] = w.permute(2, 1, 0)
            img = wp.view(KK, CinPadN, CoutPadK // 8, 8).permute(0, 2, 1, 3).contiguous()
            o = c.p[2].off // 2      # (a CSP pair's two data-gradient images are row ranges of one buffer)
            self.raw(c.p[2].obj).view(self.dt)[o: o + img.numel()] = img.reshape(-1).to(self.dt)

    def _conv_core(self, s, xin=None):
        x = s.x.obj
        K = s.K8 * 8
        if xin is None:
            xin = self.tv(x, K).float() if not isinstance(x, Buf) else None
        N, H, W = s.N, s.H, s.W
        nslab = max(t[2] for t in s.taps) + 1
        wo = s.w.off // 2
        wimg = self.raw(s.w.obj).view(self.dt)[wo: wo + nslab * s.K8 * s.CoutPad * 8].float().view(nslab, s.K8, s.CoutPad, 8)
        wt = wimg.permute(0, 2, 1, 3).reshape(nslab, s.CoutPad, K)
        P = 4
        xp = F.pad(xin, (0, 0, P, P + 2 * s.gridW, P, P + 2 * s.gridH))
        acc = torch.zeros(N, s.gridH, s.gridW, s.CoutPad)
        for (dy, dx, ws) in s.taps:
            sl = xp[:, P + dy: P + dy + s.gridH * s.in_stride: s.in_stride, P + dx: P + dx + s.gridW * s.in_stride: s.in_stride, :]
            acc += torch.einsum("nhwk,ck->nhwc", sl, wt[ws])
        return acc

    def op_CONV(self, c):
        s = c.desc
        xin = None
        if getattr(s, "xf", None) is not None:
            # BatchNorm(train) + activation of the input applied by this launch (Plan._defer_bn): x is the producer's raw
            # output; the same finalisation and rounding point as BN_ACT_FWD, whose records / activated tensor / running
            # statistics only the launch with xf_write stores
            assert s.xf_C == s.K8 * 8 and s.xf_bn.p[0].obj is s.x.obj, c.tag
            xin = self._bn_act(s.xf_bn, write=bool(s.xf_write)).float()
            a = s.xf_bn.p[12].obj
            if id(a.buf) in self.dev_out:
                # teacher forcing at the inner stage: the activated tensor the launch stored is what its matrix cores read
                # (it is compared with the BatchNorm above on its own); a one-ulp flip of the transform must not count
                # again in the convolution's output
                xin = self.tv_stored(a).float()
        acc = self._conv_core(s, xin)
        Cout = s.Cout
        res = acc[..., :Cout].clone()
        bias = self.T(s.bias.obj)
        if bias is not None:
            res += bias.detach().float().view(1, 1, 1, -1)
        ys = slice(s.out_oy, s.out_oy + s.gridH * s.out_stride, s.out_stride)
        xs = slice(s.out_ox, s.out_ox + s.gridW * s.out_stride, s.out_stride)
        if s.flags & L.MI_CONV_OUT_F32:
            nstr = s.y_nstride if s.y_nstride else s.outH * s.outW * s.ldy
            base = self.raw(s.y.obj).view(torch.float32)
            yv = base.as_strided((s.N, s.outH, s.outW, Cout), (nstr, s.outW * s.ldy, s.ldy, 1), s.y.off // 4)
        else:
            t = s.y.obj
            assert isinstance(t, TRef)
            yv = self.tv(t, Cout)
        if s.flags & L.MI_CONV_ACCUM:
            # two roundings, like autograd's sum of two bf16 gradients: bf16(this launch's result), then bf16(that + old)
            new, old = res.to(yv.dtype).float(), yv[:, ys, xs, :].float()
            res = new + old
            if not (s.flags & L.MI_CONV_OUT_F32):
                mb = self.mag.get(id(t.buf))
                if mb is None:
                    mb = self.mag[id(t.buf)] = torch.zeros(t.buf.nbytes // 2)
                mv = mb.as_strided((t.N, t.H, t.W, Cout), (t.H * t.W * t.ld, t.W * t.ld, t.ld, 1), t.coff)[:, ys, xs, :]
                mv.copy_(torch.maximum(torch.maximum(new.abs(), old.abs()), mv))
        yv[:, ys, xs, :] = res.to(yv.dtype)
        if not (s.flags & L.MI_CONV_OUT_F32):
            yv = self.tv_stored(t, Cout)
        if s.flags & L.MI_CONV_BNBWD:   # BatchNorm-backward sums of the layer that produced this gradient's tensor
            b = s.bnb
            C = Cout
            yy = self.tv(b["y"].obj).float()[:, ys, xs, :]
            z = yy * self.f32(b["scale"], C) + self.f32(b["shift"], C)
            sg = torch.sigmoid(z)
            g = sg * (1 + z * (1 - sg)) if b["act"] else torch.ones_like(z)
            dz = yv[:, ys, xs, :].float() * g
            xh = (yy - self.f32(b["mean"], C)) * self.f32(b["invstd"], C)
            st = self.f64(s.stats, C * 2).view(C, 2)
            st[:, 0] += dz.double().sum((0, 1, 2))
            st[:, 1] += (dz * xh).double().sum((0, 1, 2))
        elif s.stats.obj is not None:   # fp64 accumulators [SLOTS][CoutPad][2]: the interpreter adds everything to slot 0
            st = self.f64(s.stats, s.CoutPad * 2).view(s.CoutPad, 2)
            stored = yv[:, ys, xs, :].float() if not (s.flags & L.MI_CONV_OUT_F32) else res
            st[:Cout, 0] += stored.double().sum((0, 1, 2))
            st[:Cout, 1] += (stored.double() ** 2).sum((0, 1, 2))

    def op_WGRAD(self, c):
        s = c.desc
        x, dyT = s.x.obj, s.dy.obj
        xin = self.tv(x, s.CinPad).float()
        dy = self.tv(dyT, s.CoutPad).float()
        P = 4
        xp = F.pad(xin, (0, 0, P, P + 2 * s.outW, P, P + 2 * s.outH))
        KK = len(s.taps)
        g = self.T(s.gw.obj)   # fp32 OIHW gradient tensor (overwritten)
        kk = int(round(KK ** 0.5))
        res = torch.zeros(s.Cout, s.Cin, KK)
        for t, (ty, tx) in enumerate(s.taps):
            sl = xp[:, P + ty: P + ty + s.outH * s.stride: s.stride, P + tx: P + tx + s.outW * s.stride: s.stride, :]
            res[:, :, t] = torch.einsum("nhwo,nhwi->oi", dy, sl)[: s.Cout, : s.Cin]
        g.copy_(res.view(s.Cout, s.Cin, kk, kk))

    # ---- depthwise 3x3 (DWConv.dconv)
    def _dw_w(self, p, C):
        return self.T(p.obj).detach().float().to(self.dt).float().view(C, 1, 3, 3)   # rounded like every conv operand

    def op_DWCONV_FWD(self, c):
        ldx, ldy, N, H, W, C, stride, Ho, Wo, nsl = c.i[:10]
        x, y = c.p[0].obj, c.p[2].obj
        xin = self.tv(x, C).float().permute(0, 3, 1, 2)
        res = F.conv2d(xin, self._dw_w(c.p[1], C), None, stride=stride, padding=1, groups=C).permute(0, 2, 3, 1)
        assert tuple(res.shape) == (N, Ho, Wo, C)
        self.tv(y, C)[:] = res.to(self.dt)
        if c.p[3].obj is not None:
            CA = (C + 31) // 32 * 32
            st = self.f64(c.p[3], CA * 2).view(CA, 2)
            stored = self.tv(y, C).float()
            st[:C, 0] += stored.double().sum((0, 1, 2))
            st[:C, 1] += (stored.double() ** 2).sum((0, 1, 2))

    def op_DWCONV_DGRAD(self, c):
        lddy, lddx, N, H, W, C, stride, Ho, Wo, acc = c.i[:10]
        dy = self.tv(c.p[0].obj, C).float().permute(0, 3, 1, 2)
        dxv = self.tv(c.p[2].obj, C)
        xz = torch.zeros(N, C, H, W, requires_grad=True)
        F.conv2d(xz, self._dw_w(c.p[1], C), None, stride=stride, padding=1, groups=C).backward(dy)
        g = xz.grad.permute(0, 2, 3, 1)
        dxv[:] = (g + (dxv.float() if acc else 0)).to(self.dt)

    def op_DWCONV_WGRAD(self, c):
        ldx, lddy, N, H, W, C, stride, Ho, Wo = c.i[:9]
        x = self.tv(c.p[0].obj, C).float().permute(0, 3, 1, 2)
        dy = self.tv(c.p[1].obj, C).float().permute(0, 3, 1, 2)
        wz = torch.zeros(C, 1, 3, 3, requires_grad=True)
        F.conv2d(x, wz, None, stride=stride, padding=1, groups=C).backward(dy)
        self.T(c.p[3].obj).copy_(wz.grad)

    def op_BN_EVAL_AFFINE(self, c):
        C = c.i[0]
        g, b, rm, rv = (self.T(c.p[k].obj).detach().float() for k in range(4))
        inv = 1.0 / torch.sqrt(rv + c.f[0])
        self.f32(c.p[4], C).copy_(g * inv)
        self.f32(c.p[5], C).copy_(b - rm * g * inv)

    def op_BN_ACT_FWD(self, c):
        self._bn_act(c, write=True)

    def _bn_act(self, c, write):
        """BN_ACT_FWD: -> the activated tensor (storage dtype); write=False (a BatchNorm applied by a consumer launch
        that is not the record's writer) stores nothing"""
        y, res, a = c.p[0].obj, c.p[11].obj, c.p[12].obj
        C, act = c.i[3], c.i[4]
        if c.p[1].obj is not None:   # train mode: finalize the statistics first
            count = c.l[0]
            nsl = c.i[5]
            CA = (C + 31) // 32 * 32   # accumulator layout [slot][C rounded up to 32][2] (bn_act.hip BN_ACC_C)
            part = self.f64(c.p[1], nsl * CA * 2).view(nsl, CA, 2).sum(0)[:C]
            mean = part[:, 0] / count
            var = (part[:, 1] / count - mean * mean).clamp(min=0)
            invstd = 1.0 / torch.sqrt(var + c.f[0])
            gamma, beta = self.T(c.p[2].obj).detach().double(), self.T(c.p[3].obj).detach().double()
            sc, sh = (gamma * invstd).float(), (beta - mean * gamma * invstd).float()
            if write:
                self.f32(c.p[7], C).copy_(sc)
                self.f32(c.p[8], C).copy_(sh)
                self.f32(c.p[9], C).copy_(mean.float())
                self.f32(c.p[10], C).copy_(invstd.float())
                m = c.f[1]
                rm, rv, nbt = self.T(c.p[4].obj), self.T(c.p[5].obj), self.T(c.p[6].obj)
                if rm is not None:
                    rm.mul_(1 - m).add_(m * mean.float())
                    rv.mul_(1 - m).add_(m * (var * count / max(count - 1, 1)).float())
                    nbt += 1
        else:
            sc, sh = self.f32(c.p[7], C), self.f32(c.p[8], C)
        z = self.tv(y).float() * sc + sh
        o = z * torch.sigmoid(z) if act else z
        if res is not None:
            o = o + self.tv(res).float()
        o = o.to(self.dt)
        if write:
            self.tv(a)[:] = o
        return o

    def _dz(self, c, da, y, C, act):
        yy = self.tv(y).float()
        z = yy * self.f32(c.p[2], C) + self.f32(c.p[3], C)
        s = torch.sigmoid(z)
        g = s * (1 + z * (1 - s)) if act else torch.ones_like(z)
        dz = self.tv(da).float() * g
        xh = (yy - self.f32(c.p[4], C)) * self.f32(c.p[5], C)
        return dz, xh

    def op_BN_BWD_REDUCE(self, c):
        C, act = c.i[3], c.i[4]
        dz, xh = self._dz(c, c.p[0].obj, c.p[1].obj, C, act)
        part = self.f64(c.p[6], ((C + 31) // 32 * 32) * 2).view(-1, 2)[:C]   # slot 0, [C rounded up to 32][2]
        part[:, 0] += dz.double().sum((0, 1, 2))
        part[:, 1] += (dz * xh).double().sum((0, 1, 2))

    def op_BN_BWD_APPLY(self, c):
        C, act = c.i[5], c.i[6]
        count = c.l[1]
        da = c.p[0].obj
        dz, xh = self._dz(c, da, c.p[1].obj, C, act)
        nsl = c.i[7]
        CA = (C + 31) // 32 * 32
        part = self.f64(c.p[7], nsl * CA * 2).view(nsl, CA, 2).sum(0)[:C]
        if c.p[8].obj is not None:
            self.T(c.p[8].obj).copy_(part[:, 1].float())
        if c.p[9].obj is not None:
            self.T(c.p[9].obj).copy_(part[:, 0].float())
        c1, c2 = (part[:, 0] / count).float(), (part[:, 1] / count).float()
        gamma = self.T(c.p[6].obj).detach().float()
        dy = gamma * self.f32(c.p[5], C) * (dz - c1 - xh * c2)
        self.tv(c.p[10].obj)[..., :C] = dy.to(self.dt)   # the out-gradient view carries zero pad channels up to 32
        dres = c.p[11].obj
        if dres is not None:
            v = self.tv(da).float()
            if c.i[4]:
                v = v + self.tv(dres).float()
            self.tv(dres)[:] = v.to(self.dt)

    def op_FOCUS(self, c):
        img = self.T(c.p[0].obj).float()
        out = c.p[1].obj
        tl, tr = img[..., ::2, ::2], img[..., ::2, 1::2]
        bl, br = img[..., 1::2, ::2], img[..., 1::2, 1::2]
        cat = torch.cat((tl, bl, tr, br), 1).permute(0, 2, 3, 1)
        v = self.tv(out)
        v.zero_()
        v[..., :12] = cat.to(self.dt)

    def op_UPSAMPLE_FWD(self, c):
        x, y = c.p[0].obj, c.p[1].obj
        self.tv(y)[:] = self.tv(x).repeat_interleave(2, 1).repeat_interleave(2, 2)

    def op_UPSAMPLE_BWD(self, c):
        dy, dx = c.p[0].obj, c.p[1].obj
        g = self.tv(dy).float()
        v = g[:, 0::2, 0::2] + g[:, 0::2, 1::2] + g[:, 1::2, 0::2] + g[:, 1::2, 1::2]
        if c.i[2]:
            v = v + self.tv(dx).float()
        self.tv(dx)[:] = v.to(self.dt)

    # SPP: argmax codes as csrc/misc_ops.hip stores them - idx = [dy code x3][dx code x3] planes of N*H*W*C bytes; dx code
    # (+6) of the first maximum of the row segment around a pixel, dy code (+6) of the first row whose segment maximum
    # equals the window maximum.  The backward pass reads the codes (teacher forcing: the device's own on the GPU).
    def _spp_codes(self, c):
        x = c.p[0].obj
        return self.rawbytes(c.p[4], 6 * x.npix * x.C).view(6, x.N, x.H, x.W, x.C)

    def op_SPP_FWD(self, c):
        x = c.p[0].obj
        xin = self.tv(x).float()
        codes = self._spp_codes(c)
        for k, o in enumerate((c.p[1].obj, c.p[2].obj, c.p[3].obj)):
            r = 2 + 2 * k
            hm, hc = self._first_max(xin, r, 2)
            vm, vc = self._first_max(hm, r, 1)
            codes[3 + k] = hc
            codes[k] = vc
            self.tv(o)[:] = vm.to(self.dt)

    @staticmethod
    def _first_max(v, r, dim):
        """max over [p - r, p + r] along dim (out-of-range skipped) and the offset + 6 of its first occurrence"""
        n = v.shape[dim]
        pad = [0, 0] * (v.dim() - 1 - dim) + [r, r]
        vp = F.pad(v, pad, value=float("-inf"))
        m = torch.full_like(v, float("-inf"))
        am = torch.full(v.shape, 6, dtype=torch.uint8)
        for d in range(-r, r + 1):
            cand = vp.narrow(dim, r + d, n)
            upd = cand > m
            m = torch.where(upd, cand, m)
            am[upd] = d + 6
        return m, am

    def op_SPP_BWD(self, c):
        x = c.p[4].obj
        N, H, W, C_ = x.N, x.H, x.W, x.C
        codes = self.rawbytes(c.p[3], 6 * x.npix * C_).view(6, N, H, W, C_).long()
        acc = torch.zeros(N, H * W, C_)
        py = torch.arange(H).view(1, H, 1, 1)
        px = torch.arange(W).view(1, 1, W, 1)
        for k, d in enumerate((c.p[0].obj, c.p[1].obj, c.p[2].obj)):
            g = self.tv(d).float()
            sy = (py + codes[k] - 6).clamp(0, H - 1)
            dxc = torch.gather(codes[3 + k], 1, sy)            # the dx code of the source row's segment maximum
            sx = (px + dxc - 6).clamp(0, W - 1)
            acc.scatter_add_(1, (sy * W + sx).view(N, H * W, C_), g.reshape(N, H * W, C_))   # overlapping windows ADD
        v = acc.view(N, H, W, C_)
        if c.i[2]:
            v = v + self.tv(x).float()
        self.tv(x)[:] = v.to(self.dt)
    def op_COPY(self, c):
        raise NotImplementedError

    def op_BIAS_GRADS(self, c):
        B, A, nch, n = c.i[:4]
        dp = self.f32(c.p[1], B * A * nch).view(B, A, nch)
        for j in c.desc.jobs:
            self.T(j["out"]).copy_(dp[:, j["a0"]: j["a0"] + j["HW"], j["c0"]: j["c0"] + j["nc"]].sum((0, 1)).view_as(j["out"]))

    def op_COLSUM(self, c):
        x, out = c.p[0].obj, self.T(c.p[1].obj)
        C = c.i[1]
        v = self.tv(x, C).float().sum((0, 1, 2))
        if c.i[2]:
            out.add_(v.view_as(out))
        else:
            out.copy_(v.view_as(out))

    def _loss_inputs(self, s):
        nch = 5 + s.ncls
        preds = self.f32(s.preds, s.B * s.A * nch).view(s.B, s.A, nch)
        return preds, self.T(s.labels.obj), self.T(s.anchors.obj)

    def op_LOSS_FWD(self, c):
        s = c.desc
        preds, labels, anchors = self._loss_inputs(s)
        res, assigns = O.yolox_losses(preds.clone(), labels, anchors, s.ncls, return_assign=True,
                                      use_l1=getattr(s, "use_l1", False))
        out = self.raw(s.ws["out"]).view(torch.float32)
        nfg = sum(a["num_fg"] for a in assigns if a is not None)
        ngt = int((labels.sum(2) > 0).sum())
        out[:8] = torch.tensor([float(res[0]), float(res[1]), float(res[2]), float(res[3]), float(res[4]), float(res[5]),
                                float(nfg), float(ngt)])
        # the SimOTA assignment (integers; the matched IoU of a foreground anchor)
        B, A = s.B, s.A
        fg = self.raw(s.ws["fg"])[: B * A].view(B, A)
        mgt = self.raw(s.ws["matched_gt"]).view(torch.int32)[: B * A].view(B, A)
        miou = self.raw(s.ws["matched_iou"]).view(torch.float32)[: B * A].view(B, A)
        self.raw(s.ws["ngt"]).view(torch.int32)[:B] = (labels.sum(2) > 0).sum(1).to(torch.int32)
        fg.zero_(); mgt.fill_(-1); miou.zero_()
        for b, a in enumerate(assigns):
            if a is None:
                continue
            f = a["fg"].bool()
            fg[b] = f.to(torch.uint8)
            mgt[b][f] = a["matched_gt"].to(torch.int32)
            miou[b][f] = a["matched_iou"].float().detach()

    def op_LOSS_BWD(self, c):
        s = c.desc
        preds, labels, anchors = self._loss_inputs(s)
        raw = preds.clone().requires_grad_(True)
        l1 = getattr(s, "use_l1", False)
        res = O.yolox_losses(raw, labels, anchors, s.ncls, use_l1=l1)
        gw = self.f32(c.p[1], 5 if l1 else 4)
        tot = gw[0] * res[0] + gw[1] * res[1] + gw[2] * res[2] + gw[3] * res[3]
        if l1:
            tot = tot + gw[4] * res[4]
        tot.backward()
        self.f32(c.p[2], raw.numel()).copy_(raw.grad.reshape(-1))

    def op_SPLIT_DPREDS(self, c):
        B, A, nch, a0, HW, c0, nc, ld = c.i[:8]
        dp = self.f32(c.p[0], B * A * nch).view(B, A, nch)
        dst = c.p[1].obj
        v = self.tv(dst)
        v.zero_()
        v.view(B, HW, ld)[..., :nc] = dp[:, a0:a0 + HW, c0:c0 + nc].to(self.dt)

    def op_DECODE(self, c):
        B, A, ncls = c.i[:3]
        p = self.f32(c.p[0], B * A * (5 + ncls)).view(B, A, 5 + ncls)
        p.copy_(O.decode_eval(p.clone(), self.T(c.p[1].obj)))
