"""detectron2's RegNet (`build_regnet_backbone`: SimpleStem + ResBottleneckBlock, train-mode BatchNorm, ReLU) on the MI355X
kernels - the backbone of configs/coco/detr/detr_256_6_6_regnetx_0.4g.yaml (yolov7/modeling/backbone/regnet.py builds
detectron2's RegNet with norm = "SyncBN").  detectron2 is NOT vendored in the reference and not installed here: module
structure, state_dict keys (`stem.conv.weight`, `stem.bn.*`, `s2.b1.proj.weight`, `s2.b1.bn.*`, `s2.b1.f.a.weight`,
`s2.b1.f.a_bn.*`, `s2.b1.f.b.*`, `s2.b1.f.c.*` ...), the width rule (generate_regnet_parameters + adjust_block_compatibility)
and init_weights are restated from d2 upstream's modeling/backbone/regnet.py (parity unpinned: the CPU restatement is
tests/regnet_ref.py).

How it runs (activations are bf16 NCHW tensors in channels_last memory = NHWC for the kernels):
  * one autograd node per conv + BatchNorm (+ ReLU) layer (_ConvBnFn) and one for the block tail (_TailFn: the `c` convolution,
    the projection, both norms, the shortcut add and the ReLU);
  * 1x1 layers and the 3x3 stem: the implicit-GEMM convolution with its own statistics epilogue (_ConvGeom.fwd(stats = acc));
    grouped 3x3 layers: mi_gconv_fwd, then mi_bn_stats (conv_grouped.hip has no statistics epilogue);
  * the norm, the residual and the ReLU: mi_bn_relu_fwd, ONE launch with one rounding - relu(BN_p(proj(x)) + BN_c(c)) or
    relu(x + BN_c(c)) for the tail; the running statistics and num_batches_tracked are updated inside that launch, so a replay
    of a captured step advances them; eval mode is the same launch with scale / shift from mi_bn_eval_affine;
  * backward: mi_bn_relu_bwd_reduce / _apply, then the existing data gradients.  The two gradients of a block input are summed
    without a pass of their own: the tail leaves its share (the identity tail's dres buffer, or the projection's dy) with the
    block, and the `a` layer's data gradient accumulates into it (dgrad(accum = True));
  * 1x1 weight gradients join WgradBatch (one grouped launch per block), the grouped one runs directly; the image needs none.
Statistics are per process: the reference's SyncBN shares them across ranks, which is a later change (one warning at build
time under torch.distributed with more than one rank).
"""
import ctypes as C
import warnings

import numpy as np
import torch
from torch import nn

from .. import _lib as L
from ..d2shim import BACKBONE_REGISTRY, Backbone, ShapeSpec
from ..ops import (_ConvGeom, _gconv_desc, _gconv_images, _gconv_out, _ld, _nchw, _nhwc_v, _rup, wgrad_can_defer,
                   wgrad_flush_point)

SLOTS = L.MI_BN_SLOTS


# ------------------------------------------------------------------------------------------------------ the kernels' side
class _Conv:
    """one convolution's operands and launches: dense (1x1, or the 3x3 stem) on the implicit-GEMM kernels, grouped 3x3 on
    conv_grouped.hip.  run() leaves y [N, Ho, Wo, Cout] (raw output, bf16) and, in train mode, the statistics accumulators"""

    def __init__(self, x, weight, stride, groups, need_dx, stats):
        self.groups, self.weight = groups, weight
        dev = x.device
        N = x.shape[0]
        self.Cout = weight.shape[0]
        self.CA = _rup(self.Cout, 32)
        self.acc = torch.zeros(SLOTS * self.CA * 2, dtype=torch.float64, device=dev) if stats else None
        if groups == 1:
            g = self.g = _ConvGeom(x.shape, weight.shape, stride, (weight.shape[2] - 1) // 2)
            self.xh = g.pad_in(x)
            wf, self.wd = g.pack(weight, dgrad=need_dx)
            self.Ho, self.Wo = g.Ho, g.Wo
            self.y = torch.empty(N, g.Ho, g.Wo, g.Cout, dtype=torch.bfloat16, device=dev)
            g.fwd(self.xh, wf, self.y, stats=self.acc, nslots=SLOTS if stats else 0)
        else:
            d = self.d = _gconv_desc(x.shape, weight.shape, stride, 1, groups)
            L.check(L.lib().mi_gconv_wgrad_plan(C.byref(d), None), "RegNet grouped 3x3")
            self.xh = _nhwc_v(x)
            wf, self.wd = _gconv_images(weight, self.Cout, self.Cout // groups, True, need_dx)
            self.Ho, self.Wo = _gconv_out(x.shape[2], x.shape[3], stride)
            self.y = torch.empty(N, self.Ho, self.Wo, self.Cout, dtype=torch.bfloat16, device=dev)
            d.x, d.ldx, d.y, d.ldy, d.w = self.xh.data_ptr(), _ld(self.xh), self.y.data_ptr(), self.Cout, wf.data_ptr()
            L.check(L.lib().mi_gconv_fwd(C.byref(d), L.stream_ptr()), "mi_gconv_fwd")
            if stats:
                L.check(L.lib().mi_bn_stats(self.y.data_ptr(), self.Cout, N * self.Ho * self.Wo, self.Cout, self.acc.data_ptr(),
                                            SLOTS, L.stream_ptr()), "mi_bn_stats")
        self.npix = N * self.Ho * self.Wo
        self.stat = torch.empty(4, self.Cout, dtype=torch.float32, device=dev)     # scale, shift, mean, invstd

    def dy_buffer(self):
        """the gradient of y as the data / weight gradients read it: dense convolutions take CoutPad channels (pads zero)"""
        CP = self.CA if self.groups == 1 else self.Cout
        dy = torch.empty(self.y.shape[0], self.Ho, self.Wo, CP, dtype=torch.bfloat16, device=self.y.device)
        if CP != self.Cout:
            dy[..., self.Cout:].zero_()
        return dy

    def dgrad(self, dyh, dx=None, accum=False):
        """-> dx [N, H, W, CinPad] (dense) / [N, H, W, C] (grouped); every real channel of every pixel is written"""
        if self.groups == 1:
            g = self.g
            if dx is None:
                full = not (g.k == 1 and g.s == 2)
                dx = (torch.empty if full else torch.zeros)(g.N, g.H, g.W, g.CinP, dtype=torch.bfloat16, device=dyh.device)
            g.dgrad(dyh, self.wd, dx, accum=accum)
            return dx
        d = self.d
        dx = torch.empty(d.N, d.H, d.W, self.Cout, dtype=torch.bfloat16, device=dyh.device)
        d.x, d.ldx, d.y, d.ldy, d.w = dx.data_ptr(), self.Cout, dyh.data_ptr(), _ld(dyh), self.wd.data_ptr()
        L.check(L.lib().mi_gconv_dgrad(C.byref(d), L.stream_ptr()), "mi_gconv_dgrad")
        return dx

    def wgrad(self, dyh):
        if self.groups == 1:
            df = wgrad_can_defer(self.weight)
            return self.g.wgrad(self.xh, dyh, defer=df, owner=self.weight if df else None)
        d = self.d
        gw = torch.empty(self.weight.shape, dtype=torch.float32, device=dyh.device)
        d.x, d.ldx, d.y, d.ldy = self.xh.data_ptr(), _ld(self.xh), dyh.data_ptr(), _ld(dyh)
        need = L.check(L.lib().mi_gconv_wgrad_plan(C.byref(d), None), "mi_gconv_wgrad_plan")
        ws = torch.empty(max(int(need), 16), dtype=torch.uint8, device=dyh.device)
        d.gw, d.gbias, d.ws, d.ws_bytes = gw.data_ptr(), None, ws.data_ptr(), ws.numel()
        L.check(L.lib().mi_gconv_wgrad(C.byref(d), L.stream_ptr()), "mi_gconv_wgrad")
        return gw


def _f32(t):
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def _fill_fwd(n, cv, bn, training):
    """norm operand of the forward launch; returns the tensors that must outlive it"""
    ga, be = _f32(bn.weight), _f32(bn.bias)
    st = cv.stat
    n.y, n.ldy = cv.y.data_ptr(), cv.Cout
    n.scale, n.shift, n.mean, n.invstd = (st[i].data_ptr() for i in range(4))
    n.gamma, n.beta, n.eps = ga.data_ptr(), be.data_ptr(), bn.eps
    if training:
        n.acc, n.nslots, n.count = cv.acc.data_ptr(), SLOTS, cv.npix
        n.momentum = 0.0 if bn.momentum is None else bn.momentum
        if bn.track_running_stats and bn.running_mean is not None:
            n.running_mean, n.running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
            n.num_batches_tracked = bn.num_batches_tracked.data_ptr()
    else:
        L.check(L.lib().mi_bn_eval_affine(ga.data_ptr(), be.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                          bn.eps, cv.Cout, st[0].data_ptr(), st[1].data_ptr(), L.stream_ptr()), "mi_bn_eval_affine")
    return ga, be


def _fill_bwd(n, cv, gamma, dy):
    """norm operand of the backward launches -> (dacc, dgamma, dbeta)"""
    dev = cv.y.device
    dacc = torch.zeros(SLOTS * cv.CA * 2, dtype=torch.float64, device=dev)
    dg = torch.empty(cv.Cout, dtype=torch.float32, device=dev)
    db = torch.empty(cv.Cout, dtype=torch.float32, device=dev)
    n.y, n.ldy, n.mean, n.invstd = cv.y.data_ptr(), cv.Cout, cv.stat[2].data_ptr(), cv.stat[3].data_ptr()
    n.gamma, n.dacc, n.nslots, n.count = gamma.data_ptr(), dacc.data_ptr(), SLOTS, cv.npix
    n.dy, n.lddy, n.dgamma, n.dbeta = dy.data_ptr(), dy.shape[-1], dg.data_ptr(), db.data_ptr()
    return dacc, dg, db


def _bn_backward(d):
    L.check(L.lib().mi_bn_relu_bwd_reduce(C.byref(d), L.stream_ptr()), "mi_bn_relu_bwd_reduce")
    L.check(L.lib().mi_bn_relu_bwd_apply(C.byref(d), L.stream_ptr()), "mi_bn_relu_bwd_apply")


class _Link:
    """what a block's tail leaves for the block's first layer: the shortcut's share of the block-input gradient"""
    __slots__ = ("pending",)

    def __init__(self):
        self.pending = None


def _no_eval_backward(what):
    raise L.MI355Error(f"RegNet {what}: backward through the eval-mode (running statistics) form is not implemented")


class _ConvBnFn(torch.autograd.Function):
    """a = [relu](BN(conv(x))): the stem, and the `a` (1x1) and `b` (grouped 3x3) layers of a block"""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, bn, stride, groups, relu, link):
        training = bn.training
        need_dx = ctx.needs_input_grad[0]
        cv = _Conv(x, weight, stride, groups, need_dx, training)
        out = torch.empty(x.shape[0], cv.Ho, cv.Wo, cv.Cout, dtype=torch.bfloat16, device=x.device)
        d = L.mi_bn_relu_desc()
        keep = _fill_fwd(d.n1, cv, bn, training)
        d.a, d.lda, d.npix, d.C, d.relu = out.data_ptr(), cv.Cout, cv.npix, cv.Cout, int(relu)
        L.check(L.lib().mi_bn_relu_fwd(C.byref(d), L.stream_ptr()), "mi_bn_relu_fwd")
        del keep
        cv.acc = None
        ctx.cv, ctx.out, ctx.relu, ctx.link, ctx.training, ctx.gamma = cv, out, relu, link, training, gamma
        return _nchw(out, cv.Cout)

    @staticmethod
    def backward(ctx, grad):
        cv = ctx.cv
        if not ctx.training:
            _no_eval_backward("layer")
        da = _nhwc_v(grad)
        dyh = cv.dy_buffer()
        d = L.mi_bn_relu_desc()
        ga = _f32(ctx.gamma)
        dacc, dg, db = _fill_bwd(d.n1, cv, ga, dyh)
        d.da, d.ldda, d.a, d.lda = da.data_ptr(), _ld(da), ctx.out.data_ptr(), cv.Cout
        d.npix, d.C, d.relu = cv.npix, cv.Cout, int(ctx.relu)
        _bn_backward(d)
        dx = None
        if ctx.needs_input_grad[0]:
            pend = None
            if ctx.link is not None:
                pend, ctx.link.pending = ctx.link.pending, None
            if pend is None:
                dx = cv.dgrad(dyh)
            elif pend[0] == "buf":              # identity tail: its dres buffer already holds dz
                dx = cv.dgrad(dyh, dx=pend[1], accum=True)
            else:                               # projection tail: its data gradient adds onto this layer's
                dx = cv.dgrad(dyh)
                pend[1].dgrad(pend[2], dx=dx, accum=True)
            dx = _nchw(dx, cv.Cout if cv.groups > 1 else cv.g.Cin)
        gw = cv.wgrad(dyh) if ctx.needs_input_grad[1] else None
        return dx, gw, dg.to(ctx.gamma.dtype), db.to(ctx.gamma.dtype), None, None, None, None, None


class _TailFn(torch.autograd.Function):
    """out = relu(shortcut + BN_c(c(h))), shortcut = BN_p(proj(x)) or x: both 1x1 convolutions with their statistics epilogue
    and ONE apply launch"""

    @staticmethod
    def forward(ctx, x, h, wc, gc, bc, wp, gp, bp, blk, link):
        f = blk.f
        training = f.c_bn.training
        need_dx = ctx.needs_input_grad[0]
        cc = _Conv(h, wc, 1, 1, ctx.needs_input_grad[1], training)
        cp = _Conv(x, wp, blk.stride, 1, need_dx, training) if wp is not None else None
        out = torch.empty(x.shape[0], cc.Ho, cc.Wo, cc.Cout, dtype=torch.bfloat16, device=x.device)
        d = L.mi_bn_relu_desc()
        keep = [_fill_fwd(d.n1, cc, f.c_bn, training)]
        xh = None
        if cp is not None:
            keep.append(_fill_fwd(d.n2, cp, blk.bn, training))
        else:
            xh = _nhwc_v(x)
            d.res, d.ldres = xh.data_ptr(), _ld(xh)
        d.a, d.lda, d.npix, d.C, d.relu = out.data_ptr(), cc.Cout, cc.npix, cc.Cout, 1
        L.check(L.lib().mi_bn_relu_fwd(C.byref(d), L.stream_ptr()), "mi_bn_relu_fwd (block tail)")
        del keep
        cc.acc = None
        if cp is not None:
            cp.acc = None
        ctx.cc, ctx.cp, ctx.out, ctx.link, ctx.training, ctx.params = cc, cp, out, link, training, (gc, gp)
        ctx.x_shape = tuple(x.shape)
        return _nchw(out, cc.Cout)

    @staticmethod
    def backward(ctx, grad):
        cc, cp = ctx.cc, ctx.cp
        if not ctx.training:
            _no_eval_backward("block tail")
        gc, gp = ctx.params
        da = _nhwc_v(grad)
        d = L.mi_bn_relu_desc()
        dyc = cc.dy_buffer()
        kc = _fill_bwd(d.n1, cc, _f32(gc), dyc)
        need_x = ctx.needs_input_grad[0]
        kp = dyp = dres = None
        if cp is not None:
            dyp = cp.dy_buffer()
            kp = _fill_bwd(d.n2, cp, _f32(gp), dyp)
        elif need_x:
            N, Cin, H, W = ctx.x_shape
            dres = torch.empty(N, H, W, _rup(Cin, 32), dtype=torch.bfloat16, device=da.device)
            d.dres, d.lddres = dres.data_ptr(), dres.shape[-1]
        d.da, d.ldda, d.a, d.lda = da.data_ptr(), _ld(da), ctx.out.data_ptr(), cc.Cout
        d.npix, d.C, d.relu = cc.npix, cc.Cout, 1
        _bn_backward(d)
        dh = _nchw(cc.dgrad(dyc), cc.g.Cin) if ctx.needs_input_grad[1] else None
        gwc = cc.wgrad(dyc) if ctx.needs_input_grad[2] else None
        gwp = dgp = dbp = None
        dx = None
        if cp is not None:
            gwp = cp.wgrad(dyp) if ctx.needs_input_grad[5] else None
            dgp, dbp = kp[1].to(gp.dtype), kp[2].to(gp.dtype)
            if need_x:
                if ctx.link is not None:
                    ctx.link.pending = ("proj", cp, dyp)
                else:
                    dx = _nchw(cp.dgrad(dyp), cp.g.Cin)
        elif need_x:
            if ctx.link is not None:
                ctx.link.pending = ("buf", dres)
            else:
                dx = _nchw(dres, ctx.x_shape[1])
        return dx, dh, gwc, kc[1].to(gc.dtype), kc[2].to(gc.dtype), gwp, dgp, dbp, None, None


def _need_cuda(x, who):
    if not x.is_cuda:
        raise L.MI355Error(f"{who}: the MI355X path needs device tensors (no CPU fallback)")


# ------------------------------------------------------------------------------------------------------ d2's module tree
def conv2d(w_in, w_out, k, *, stride=1, groups=1, bias=False):
    assert k % 2 == 1, "Only odd size kernels supported to avoid padding issues."
    return nn.Conv2d(w_in, w_out, k, stride=stride, padding=(k - 1) // 2, groups=groups, bias=bias)


def _norm(c):
    """the holder of a norm's parameters and running statistics (nn.BatchNorm2d's names and defaults: eps 1e-5, momentum 0.1);
    its arithmetic runs in mi_bn_relu_fwd"""
    return nn.BatchNorm2d(c, eps=1e-5, momentum=0.1)


def init_weights(m):
    """d2 regnet.py init_weights"""
    if isinstance(m, nn.Conv2d):
        fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
        m.weight.data.normal_(mean=0.0, std=float(np.sqrt(2.0 / fan_out)))
    elif isinstance(m, nn.BatchNorm2d):
        m.weight.data.fill_(1.0)
        m.bias.data.zero_()
    elif isinstance(m, nn.Linear):
        m.weight.data.normal_(mean=0.0, std=0.01)
        m.bias.data.zero_()


def _layer(x, conv, bn, relu, link=None):
    return _ConvBnFn.apply(x, conv.weight, bn.weight, bn.bias, bn, conv.stride[0], conv.groups, relu, link)


class SimpleStem(nn.Module):
    """conv 3x3 stride 2 (3 -> w_out, no bias), bn, ReLU"""

    def __init__(self, w_in, w_out):
        super().__init__()
        self.in_channels, self.out_channels, self.stride = w_in, w_out, 2
        self.conv = conv2d(w_in, w_out, 3, stride=2)
        self.bn = _norm(w_out)

    def forward(self, x):
        _need_cuda(x, "SimpleStem")
        return _layer(x, self.conv, self.bn, True)


class BottleneckTransform(nn.Module):
    """a 1x1 + bn + ReLU, b 3x3 (stride, groups = w_b / group_width) + bn + ReLU, c 1x1 + bn (applied by the block's tail)"""

    def __init__(self, w_in, w_out, stride, params):
        super().__init__()
        w_b = int(round(w_out * params["bot_mul"]))
        if params["se_r"]:
            raise NotImplementedError("RegNet BottleneckTransform: the squeeze-excitation block (se_ratio > 0, RegNetY) is not built")
        self.groups = w_b // params["group_w"]
        self.a = conv2d(w_in, w_b, 1)
        self.a_bn = _norm(w_b)
        self.b = conv2d(w_b, w_b, 3, stride=stride, groups=self.groups)
        self.b_bn = _norm(w_b)
        self.c = conv2d(w_b, w_out, 1)
        self.c_bn = _norm(w_out)
        self.c_bn.final_bn = True


class ResBottleneckBlock(nn.Module):
    """x + F(x), F = bottleneck transform; proj + bn on the shortcut when the shape changes"""

    def __init__(self, w_in, w_out, stride, params):
        super().__init__()
        self.in_channels, self.out_channels, self.stride = w_in, w_out, stride
        self.proj, self.bn = None, None
        if (w_in != w_out) or (stride != 1):
            self.proj = conv2d(w_in, w_out, 1, stride=stride)
            self.bn = _norm(w_out)
        self.f = BottleneckTransform(w_in, w_out, stride, params)

    def forward(self, x):
        _need_cuda(x, "ResBottleneckBlock")
        f = self.f
        x = wgrad_flush_point(x)
        # the tail hands its share of x's gradient to the `a` layer only when that layer's backward is certain to run
        link = _Link() if (torch.is_grad_enabled() and x.requires_grad) else None
        h = _layer(x, f.a, f.a_bn, True, link)
        h = _layer(h, f.b, f.b_bn, True)
        if self.proj is not None:
            return _TailFn.apply(x, h, f.c.weight, f.c_bn.weight, f.c_bn.bias, self.proj.weight, self.bn.weight, self.bn.bias,
                                 self, link)
        return _TailFn.apply(x, h, f.c.weight, f.c_bn.weight, f.c_bn.bias, None, None, None, self, link)


class AnyStage(nn.Module):
    """blocks b1 ... bd, the first with the stage's stride"""

    def __init__(self, w_in, w_out, stride, d, params):
        super().__init__()
        for i in range(d):
            self.add_module("b{}".format(i + 1), ResBottleneckBlock(w_in, w_out, stride, params))
            stride, w_in = 1, w_out

    def forward(self, x):
        for block in self.children():
            x = block(x)
        return x


def adjust_block_compatibility(ws, bs, gs):
    """d2 regnet.py: adjusts the compatibility of widths, bottlenecks and groups"""
    assert len(ws) == len(bs) == len(gs)
    assert all(w > 0 and b > 0 and g > 0 for w, b, g in zip(ws, bs, gs))
    vs = [int(max(1, w * b)) for w, b in zip(ws, bs)]
    gs = [int(min(g, v)) for g, v in zip(gs, vs)]
    ms = [np.lcm(g, b) if b > 1 else g for g, b in zip(gs, bs)]
    vs = [max(m, int(round(v / m) * m)) for v, m in zip(vs, ms)]
    ws = [int(v / b) for v, b in zip(vs, bs)]
    assert all(w * b % g == 0 for w, b, g in zip(ws, bs, gs))
    return ws, bs, gs


def generate_regnet_parameters(w_a, w_0, w_m, d, q=8):
    """d2 regnet.py: per-stage widths and depths from the RegNet parameters"""
    assert w_a >= 0 and w_0 > 0 and w_m > 1 and w_0 % q == 0
    ws_cont = np.arange(d) * w_a + w_0
    ks = np.round(np.log(ws_cont / w_0) / np.log(w_m))
    ws_all = w_0 * np.power(w_m, ks)
    ws_all = np.round(np.divide(ws_all, q)).astype(int) * q
    ws, ds = np.unique(ws_all, return_counts=True)
    num_stages, total_stages = len(ws), ks.max() + 1
    ws, ds, ws_all, ws_cont = (x.tolist() for x in (ws, ds, ws_all, ws_cont))
    return ws, ds, num_stages, total_stages, ws_all, ws_cont


class AnyNet(Backbone):
    """stem, s1 ... sn"""

    def __init__(self, *, stem_width, depths, widths, group_widths, strides, bottleneck_ratios, se_ratio, freeze_at=0,
                 out_features=None):
        super().__init__()
        self.stem = SimpleStem(3, stem_width)
        current_stride = self.stem.stride
        self._out_feature_strides = {"stem": current_stride}
        self._out_feature_channels = {"stem": self.stem.out_channels}
        self.stages_and_names = []
        prev_w = stem_width
        for i, (d, w, s, b, g) in enumerate(zip(depths, widths, strides, bottleneck_ratios, group_widths)):
            params = {"bot_mul": b, "group_w": g, "se_r": se_ratio}
            stage = AnyStage(prev_w, w, s, d, params)
            name = "s{}".format(i + 1)
            self.add_module(name, stage)
            self.stages_and_names.append((stage, name))
            self._out_feature_strides[name] = current_stride = int(current_stride * s)
            self._out_feature_channels[name] = w
            prev_w = w
        self.depths, self.widths, self.group_widths = list(depths), list(widths), list(group_widths)
        self.apply(init_weights)
        if out_features is None:
            out_features = [name]
        self._out_features = list(out_features)
        assert len(self._out_features)
        children = [x[0] for x in self.named_children()]
        for out_feature in self._out_features:
            assert out_feature in children, "Available children: {} does not include {}".format(", ".join(children), out_feature)
        self.freeze(freeze_at)

    def forward(self, x):
        _need_cuda(x, "RegNet")
        assert x.dim() == 4, f"Model takes an input of shape (N, C, H, W). Got {x.shape} instead!"
        outputs = {}
        x = self.stem(x)
        if "stem" in self._out_features:
            outputs["stem"] = x
        for stage, name in self.stages_and_names:
            x = stage(x)
            if name in self._out_features:
                outputs[name] = x
        return outputs

    def output_shape(self):
        return {name: ShapeSpec(channels=self._out_feature_channels[name], stride=self._out_feature_strides[name])
                for name in self._out_features}

    def stage_modules(self):
        """s1 .. s4 in forward order: single-tensor outputs that cut the backward into stages"""
        return [s for s, _ in self.stages_and_names]

    def freeze(self, freeze_at=0):
        """d2 AnyNet.freeze: 1 = the stem, 2 = stem + s1, ...  A frozen layer's norm keeps its place in the tree (d2 converts
        it to FrozenBatchNorm2d): here it runs in eval mode"""
        if freeze_at >= 1:
            self._freeze_module(self.stem)
        for idx, (stage, _) in enumerate(self.stages_and_names, start=2):
            if freeze_at >= idx:
                self._freeze_module(stage)
        return self

    @staticmethod
    def _freeze_module(m):
        if any(True for _ in m.parameters()):
            raise NotImplementedError("RegNet: freeze_at > 0 is not served (the reference's builder passes none: everything trains)")


class RegNet(AnyNet):
    def __init__(self, *, stem_width, depth, w_a, w_0, w_m, group_width, stride=2, bottleneck_ratio=1.0, se_ratio=0.0,
                 freeze_at=0, out_features=None):
        ws, ds = generate_regnet_parameters(w_a, w_0, w_m, depth)[0:2]
        ss = [stride for _ in ws]
        bs = [bottleneck_ratio for _ in ws]
        gs = [group_width for _ in ws]
        ws, bs, gs = adjust_block_compatibility(ws, bs, gs)
        super().__init__(stem_width=stem_width, depths=ds, widths=ws, group_widths=gs, strides=ss, bottleneck_ratios=bs,
                         se_ratio=se_ratio, freeze_at=freeze_at, out_features=out_features)


# yolov7/modeling/backbone/regnet.py: Regnet_types_config
Regnet_types_config = {
    "RegNetX_200MF": {"stem_width": 32, "w_a": 36.44, "w_0": 24, "w_m": 2.49, "group_width": 8, "depth": 13},
    "RegNetX_400MF": {"stem_width": 32, "w_a": 24.48, "w_0": 24, "w_m": 2.54, "group_width": 16, "depth": 22},
    "RegNetX_600MF": {"stem_width": 32, "w_a": 36.97, "w_0": 48, "w_m": 2.24, "group_width": 24, "depth": 16},
    # regnety series
    "RegNetY_200MF": {"stem_width": 32, "w_a": 36.44, "w_0": 24, "w_m": 2.49, "group_width": 8, "depth": 13, "se_ratio": 0.25},
    "RegNetY_400MF": {"stem_width": 32, "w_a": 27.89, "w_0": 48, "w_m": 2.09, "group_width": 8, "depth": 16, "se_ratio": 0.25},
    "RegNetY_600MF": {"stem_width": 32, "w_a": 32.54, "w_0": 48, "w_m": 2.32, "group_width": 16, "depth": 15, "se_ratio": 0.25},
    "RegNetY_800MF": {"stem_width": 32, "w_a": 38.84, "w_0": 56, "w_m": 2.4, "group_width": 16, "depth": 14, "se_ratio": 0.25},
    "RegNetY_1_6GF": {"stem_width": 32, "w_a": 20.71, "w_0": 48, "w_m": 2.65, "group_width": 24, "depth": 27, "se_ratio": 0.25},
    "RegNetY_3_2GF": {"stem_width": 32, "w_a": 42.63, "w_0": 80, "w_m": 2.66, "group_width": 24, "depth": 21, "se_ratio": 0.25},
    "RegNetY_4_0GF": {"stem_width": 32, "w_a": 31.41, "w_0": 96, "w_m": 2.24, "group_width": 64, "depth": 22, "se_ratio": 0.25},
    "RegNetY_6_4GF": {"stem_width": 32, "w_a": 33.22, "w_0": 112, "w_m": 2.27, "group_width": 72, "depth": 25, "se_ratio": 0.25},
    "RegNetY_8_0GF": {"stem_width": 32, "w_a": 76.82, "w_0": 192, "w_m": 2.19, "group_width": 56, "depth": 17, "se_ratio": 0.25},
    "RegNetY_12GF": {"stem_width": 32, "w_a": 73.36, "w_0": 168, "w_m": 2.37, "group_width": 112, "depth": 19, "se_ratio": 0.25},
    "RegNetY_16GF": {"stem_width": 32, "w_a": 106.23, "w_0": 200, "w_m": 2.48, "group_width": 112, "depth": 18, "se_ratio": 0.25},
    "RegNetY_32GF": {"stem_width": 32, "w_a": 115.89, "w_0": 232, "w_m": 2.53, "group_width": 232, "depth": 20, "se_ratio": 0.25},
}
SERVED_GROUP_WIDTHS = (8, 16, 24)

_warned_ranks = False


def _warn_per_rank_statistics():
    global _warned_ranks
    import torch.distributed as dist
    if not _warned_ranks and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        _warned_ranks = True
        warnings.warn("build_regnet_backbone: the reference builds RegNet with norm = \"SyncBN\" (batch statistics shared across "
                      "ranks); here every rank normalises with the statistics of its own images (cross-rank statistics are not "
                      "built yet)")


@BACKBONE_REGISTRY.register()
def build_regnet_backbone(cfg, input_shape=None):
    t = cfg.MODEL.REGNETS.TYPE
    out_features = cfg.MODEL.REGNETS.OUT_FEATURES
    assert t in Regnet_types_config.keys(), "type must be one of: {}".format(Regnet_types_config.keys())
    args = Regnet_types_config[t]
    if args.get("se_ratio", 0.0):
        msg = f"build_regnet_backbone: {t} needs the squeeze-excitation block (se_ratio {args['se_ratio']}), which is not built"
        if args["group_width"] not in SERVED_GROUP_WIDTHS:
            msg += f"; its group width {args['group_width']} is not one the grouped 3x3 kernels serve {SERVED_GROUP_WIDTHS} either"
        raise NotImplementedError(msg + " (served: RegNetX_200MF, RegNetX_400MF, RegNetX_600MF)")
    _warn_per_rank_statistics()
    # the reference's builder passes no freeze_at: d2's default 0, everything trains (MODEL.BACKBONE.FREEZE_AT is not read)
    return RegNet(out_features=out_features, **args)
