"""ResNet-vd (`build_resnet_vd_backbone`, yolov7/modeling/backbone/resnetvd.py) on the MI355X kernels - the backbone of
configs/coco/sparseinst/sparse_inst_r50vd_{base,giam,giam_aug}.yaml.  Only the path the reference's builder takes:
stem_type "deep", stem_width 32, avg_down True, bottleneck blocks, depth 50 / 101.  timm (whose `Bottleneck` the reference
imports) is not vendored there: the block is restated from the reference's own DeformableBottleneck (resnetvd.py:23-117),
the same layout without the offset branch - conv1/bn1/act1, conv2/bn2/act2 with the stride in conv2, conv3/bn3, downsample,
act3.

state_dict keys are the reference's (= timm's resnet50d, apart from fc.* and num_batches_tracked):
  conv1.{0,3,6}.weight, conv1.{1,4}.*, bn1.*, layer{1..4}.{i}.conv{1,2,3}.weight, layer{1..4}.{i}.bn{1,2,3}.*,
  layer{k}.0.downsample.1.weight, layer{k}.0.downsample.2.*      (downsample.0: the parameter-free pool / Identity)
Every norm is a FrozenBatchNorm2d (four buffers).  The nn.Conv2d modules only HOLD the weights (nn.Conv2d's default
initialisation: the reference never re-initialises them); nothing here calls their forward.

How it runs (on top of modeling/resnet.py: frozen affine folded into the packed weights, one-node bottlenecks, grouped
weight gradients):
  * deep stem = four launches + the pool: mi_focus_pack (space-to-depth, 12 channels in 16), the first 3x3 stride-2
    convolution as a 2x2-tap stride-1 convolution on that image (the 3x3 taps scattered into a 4x4 kernel whose first row /
    column are zero, the 7x7 stem's idea), two 3x3 stride-1 convolutions; every frozen affine + ReLU in an epilogue
    (bn1 / act1 are the third convolution's), then MaxPool2d(3, 2, 1);
  * projection shortcut = AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) (mi_avgpool2x2s2_*, skipped for the
    stride-1 layer1.0) + a 1x1 stride-1 convolution on the pooled map; conv3 + shortcut + ReLU in conv3's epilogue.  In the
    backward the shortcut's data gradient is a quarter-size map; mi_avgpool2x2s2_bwd spreads it INTO conv1's data gradient
    and, as it writes every pixel, takes the block input's ReLU mask there as well.
MODEL.BACKBONE.FREEZE_AT is not read (the reference's builder does not): everything trains.
"""
import ctypes as C

import torch
from torch import nn

from .. import _lib as L
from ..d2shim import BACKBONE_REGISTRY, Backbone, ShapeSpec
from ..ops import WgradBatch, _ConvGeom, _conv_desc, _ld, _nhwc, _run_conv, wgrad_can_defer
from .resnet import (FrozenBatchNorm2d, _BLOCK_FN, _EPI_FUSE, _FOLDED_FN, _MASK_FUSE, _MaxPool, _add_relu, _conv_relu_fused,
                     _premask_note, _premask_take, _relu, _relu_mask, _same_address, conv_norm_forward)


def avgpool2x2(xh):
    """bf16 NHWC (dense or a channel slice) -> AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) of it, dense"""
    N, H, W, Cc = xh.shape
    y = torch.empty(N, (H + 1) // 2, (W + 1) // 2, Cc, dtype=torch.bfloat16, device=xh.device)
    L.check(L.lib().mi_avgpool2x2s2_fwd(xh.data_ptr(), _ld(xh), y.data_ptr(), Cc, N, H, W, Cc, L.stream_ptr()), "mi_avgpool2x2s2_fwd")
    return y


def avgpool2x2_bwd(dyh, dxh, accumulate=False, mask=None):
    """dxh [N,H,W,C] (+)= dyh[iy / 2][ix / 2] / count, zeroed where mask <= 0 (mask: bf16 NHWC of dxh's shape)"""
    N, H, W, Cc = dxh.shape
    L.check(L.lib().mi_avgpool2x2s2_bwd(dyh.data_ptr(), _ld(dyh), dxh.data_ptr(), _ld(dxh), L.ptr(mask), _ld(mask) if mask is not None else 0,
                                        1 if accumulate else 0, N, H, W, Cc, L.stream_ptr()), "mi_avgpool2x2s2_bwd")
    return dxh


class _AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xh):          # xh bf16 [N,H,W,C] contiguous
        ctx.in_shape = tuple(xh.shape)
        return avgpool2x2(xh)

    @staticmethod
    def backward(ctx, g):
        return avgpool2x2_bwd(g.contiguous(), torch.empty(ctx.in_shape, dtype=torch.bfloat16, device=g.device))


class AvgPool2x2(nn.Module):
    """downsample.0 of a stride-2 projection shortcut: nn.AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False)"""

    def forward(self, x):          # NCHW (channels_last memory) bf16
        return _AvgPoolFn.apply(_nhwc(x)).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ deep stem
# the first convolution: out[oy][ox] = sum_{r,s} w[r][s] * img[2 oy - 1 + r][2 ox - 1 + s].  With R = r + 1 = 2 Ay + py
# (a 4x4 kernel whose row / column 0 are zero) the image row is 2 (oy + Ay - 1) + py: pixel (oy + Ay - 1) of the
# space-to-depth image, parity py - 2x2 taps (ay, ax) = (Ay - 1, Ax - 1) in {-1, 0}
_STEM_TAPS2 = [(ay - 1, ax - 1, ay * 2 + ax) for ay in range(2) for ax in range(2)]


def _w3_to_w2(w3s):
    """3x3 kernel -> 4x4 with a zero first row / column -> [Cout][q = py + 2 px][c] x 2x2 taps (mi_focus_pack's channel order)"""
    Cout, Cin = w3s.shape[:2]
    w4 = w3s.new_zeros(Cout, Cin, 4, 4)
    w4[:, :, 1:, 1:] = w3s
    return w4.view(Cout, Cin, 2, 2, 2, 2).permute(0, 5, 3, 1, 2, 4).reshape(Cout, 4 * Cin, 2, 2)   # ch = (px*2+py)*Cin+c


def _pack_stem(w3s):
    Cout, Cin = w3s.shape[:2]
    w2 = _w3_to_w2(w3s).contiguous()
    wf = torch.empty(4 * 16 * Cout, dtype=torch.bfloat16, device=w3s.device)
    L.check(L.lib().mi_pack_conv_weight(w2.data_ptr(), Cout, 4 * Cin, 2, 2, wf.data_ptr(), 16, Cout, None, 0, 0, L.stream_ptr()),
            "mi_pack_conv_weight (deep stem)")
    return wf


def _stem_conv(s2d, wf, shift, Cout):
    N, Hh, Wh, _ = s2d.shape
    a = torch.empty(N, Hh, Wh, Cout, dtype=torch.bfloat16, device=s2d.device)
    _run_conv(_conv_desc(s2d.data_ptr(), 16, N, Hh, Wh, wf, 16, a.data_ptr(), Cout, Hh, Wh, Cout, Cout, _STEM_TAPS2,
                         bias=shift, flags=L.MI_CONV_RELU), "mi_conv2d (3x3 s2 stem as 2x2 over space-to-depth, ReLU in the epilogue)")
    return a


class _Stem0Fn(torch.autograd.Function):
    """conv1.0 + conv1.1 + ReLU of a trainable deep stem.  Backward: ReLU mask, then the weight gradient in the 9-tap form (a
    3x3 stride-1 convolution on the space-to-depth image; the weight-gradient kernel serves 1, 9 or 16 taps) with the five
    taps outside {-1, 0}^2 dropped when mapping back to [Cout, 3, 3, 3].  The image needs no gradient."""

    @staticmethod
    def forward(ctx, s2d, w3, scale, shift):
        Cout = w3.shape[0]
        if Cout % 32:
            raise L.MI355Error("ResNet-vd stem: the first convolution's width must be a multiple of 32")
        a = _stem_conv(s2d, _pack_stem(w3 * scale.view(-1, 1, 1, 1)), shift, Cout)
        ctx.save_for_backward(s2d, a, scale)
        ctx.shape = (Cout, w3.shape[1])
        return a

    @staticmethod
    def backward(ctx, g):
        s2d, a, scale = ctx.saved_tensors
        Cout, Cin = ctx.shape
        N, Hh, Wh, _ = s2d.shape
        lib = L.lib()
        dy = _relu_mask(g.contiguous(), a)
        gw9 = torch.empty(Cout, 4 * Cin, 3, 3, dtype=torch.float32, device=a.device)
        d = L.mi_wgrad_desc()
        d.x, d.dy, d.gw = s2d.data_ptr(), dy.data_ptr(), gw9.data_ptr()
        d.ldx, d.ldy, d.N, d.H, d.W, d.outH, d.outW, d.stride = 16, Cout, N, Hh, Wh, Hh, Wh, 1
        d.Cin, d.Cout, d.CinPad, d.CoutPad, d.ntaps = 4 * Cin, Cout, 16, Cout, 9
        for t in range(9):
            d.tap_dy[t], d.tap_dx[t] = t // 3 - 1, t % 3 - 1
        need = lib.mi_conv2d_wgrad_plan(C.byref(d))
        L.check(need, "mi_conv2d_wgrad_plan (deep stem)")
        ws = torch.empty(max(int(need), 16), dtype=torch.uint8, device=a.device)
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
        L.check(lib.mi_conv2d_wgrad(C.byref(d), L.stream_ptr()), "mi_conv2d_wgrad (deep stem)")
        # [Cout][(px*2+py)*Cin + c][Ay][Ax] (taps -1, 0 of the nine) -> 4x4 kernel rows R = 2 Ay + py -> drop the zero row / column
        g4 = gw9[:, :, :2, :2].reshape(Cout, 2, 2, Cin, 2, 2).permute(0, 3, 4, 2, 5, 1).reshape(Cout, Cin, 4, 4)
        return None, g4[:, :, 1:, 1:] * scale.view(-1, 1, 1, 1), None, None


class BottleneckVD(nn.Module):
    """timm's Bottleneck as the reference builds it (cardinality 1, base_width 64, no attention / anti-aliasing / drop
    layers), restated from resnetvd.py:23-117"""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        outplanes = planes * self.expansion
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = FrozenBatchNorm2d(planes)
        self.act1 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = FrozenBatchNorm2d(planes)
        self.act2 = nn.ReLU(inplace=True)
        self.conv3 = nn.Conv2d(planes, outplanes, 1, bias=False)
        self.bn3 = FrozenBatchNorm2d(outplanes)
        self.act3 = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def zero_init_last_bn(self):
        nn.init.zeros_(self.bn3.weight)

    def _pairs(self):
        p = [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]
        if self.downsample is not None:
            p.append((self.downsample[1], self.downsample[2]))
        return p

    def forward(self, x):
        pairs = self._pairs()
        pooled = self.downsample is not None and isinstance(self.downsample[0], AvgPool2x2)
        if _BLOCK_FN() and torch.is_grad_enabled() and all(c.weight.requires_grad for c, _ in pairs):
            aff = [t for _, n in pairs for t in n.affine()]
            return _BottleneckVDFn.apply(x, self.stride, len(pairs) == 4, pooled, getattr(self, "input_is_relu", False),
                                         *[c.weight for c, _ in pairs], *aff)

        def conv(i, inp, stride=1, **kw):
            c, n = pairs[i]
            return conv_norm_forward(c, c.weight, n, stride, (c.weight.shape[-1] - 1) // 2, inp, **kw)
        if _conv_relu_fused():
            out = conv(1, conv(0, x, relu=True), self.stride, relu=True)
        else:
            out = _relu(conv(1, _relu(conv(0, x)), self.stride))
        sc = x
        if self.downsample is not None:
            sc = conv(3, self.downsample[0](x))
        no_grad_path = not (torch.is_grad_enabled() and (x.requires_grad or any(c.weight.requires_grad for c, _ in pairs)))
        if no_grad_path and _EPI_FUSE() and _FOLDED_FN() and self.conv3.weight.shape[0] % 32 == 0:
            return conv(2, out, add_relu=sc)       # inference: the residual add + ReLU in conv3's epilogue
        return _add_relu(conv(2, out), sc)


class _BottleneckVDFn(torch.autograd.Function):
    """A trainable BottleneckVD as ONE autograd node, in the manner of resnet._BottleneckFn (same kernels, same roundings
    as the per-module composition).  What differs is the projection shortcut: a 1x1 stride-1 convolution on the 2x2 average
    of the block input.  Its weight gradient reads the saved pooled map and joins the block's grouped launch; its data
    gradient is a quarter-size map that mi_avgpool2x2s2_bwd adds into conv1's data gradient - a pass over every pixel of the
    block input, so the input's ReLU mask is taken there (and noted for the previous block) for stride-2 blocks too, which
    the d2 block's strided shortcut cannot do."""

    @staticmethod
    def forward(ctx, x, s2, proj, pooled, in_relu, *rest):
        n = 4 if proj else 3
        ws, aff = rest[:n], rest[n:]
        ctx.in_relu = bool(in_relu)
        scales, shifts = aff[0::2], aff[1::2]
        need_dx = x.requires_grad
        N, Cin, H, W = x.shape
        bc = ws[0].shape[0]
        g1 = _ConvGeom((N, Cin, H, W), ws[0].shape, 1, 0)
        g2 = _ConvGeom((N, bc, H, W), ws[1].shape, s2, 1)
        g3 = _ConvGeom((N, bc, g2.Ho, g2.Wo), ws[2].shape, 1, 0)
        Hp, Wp = ((H + 1) // 2, (W + 1) // 2) if pooled else (H, W)
        gs = _ConvGeom((N, Cin, Hp, Wp), ws[3].shape, 1, 0) if proj else None
        geoms = [g1, g2, g3] + ([gs] if proj else [])
        for g in geoms:
            if g.CinP != g.Cin or g.CoutP != g.Cout:
                raise L.MI355Error("ResNet-vd bottleneck: channel counts must be multiples of 32")
        if (proj and (gs.Ho, gs.Wo) != (g2.Ho, g2.Wo)) or (not proj and (s2 != 1 or Cin != ws[2].shape[0])):
            raise L.MI355Error("ResNet-vd bottleneck: the shortcut's map does not match conv3's")
        imgs = [g.pack(w, dgrad=(need_dx or i in (1, 2)), scale=sc)
                for i, (g, w, sc) in enumerate(zip(geoms, ws, scales))]
        dev = x.device
        xh = _nhwc(x)

        def run(g, inp, i, relu, add_relu=None):
            y = torch.empty(g.N, g.Ho, g.Wo, g.CoutP, dtype=torch.bfloat16, device=dev)
            g.fwd(inp, imgs[i][0], y, bias=shifts[i], relu=relu, add_relu=add_relu)
            return y
        a1 = run(g1, xh, 0, True)
        a2 = run(g2, a1, 1, True)
        xp = avgpool2x2(xh) if pooled else xh
        sc = run(gs, xp, 3, False) if proj else xh
        ctx.epi = _EPI_FUSE()
        if ctx.epi:
            y = run(g3, a2, 2, False, add_relu=sc)            # relu(bf16(conv3 + shift) + shortcut) in conv3's epilogue
        else:
            o = run(g3, a2, 2, False)
            y = torch.empty_like(o)
            L.check(L.lib().mi_ew_bf16(o.data_ptr(), sc.data_ptr(), y.data_ptr(), o.numel(), 7, L.stream_ptr()), "mi_ew_bf16 add+relu")
        ctx.geoms, ctx.proj, ctx.pooled = geoms, bool(proj), bool(pooled)
        ctx.params = ws
        ctx.save_for_backward(xh, a1, a2, y, xp if pooled else None, *[im[1] for im in imgs], *scales)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        n = 4 if ctx.proj else 3
        xh, a1, a2, y, xp = ctx.saved_tensors[:5]
        wds, scales = ctx.saved_tensors[5:5 + n], ctx.saved_tensors[5 + n:]
        g1, g2, g3 = ctx.geoms[:3]
        gs = ctx.geoms[3] if ctx.proj else None
        gyh = _nhwc(gy)
        if _premask_take(gyh):
            gm = gyh                        # the next block's backward masked it in its last pass (and owns no other use of it)
        else:
            gm = _relu_mask(gyh, y)         # (a fresh tensor: identity blocks accumulate the input gradient into it)
        gws = [None] * n
        # the block's three or four weight gradients as ONE grouped launch (ops.WgradBatch), issued below - before the input
        # gradient is accumulated INTO gm, which two of the jobs read
        df = wgrad_can_defer(*ctx.params)
        gws[2] = g3.wgrad_scaled(a2, gm, scales[2], defer=df, owner=ctx.params[2] if df else None)
        da2 = torch.empty_like(a2)
        if ctx.epi:
            g3.dgrad(gm, wds[2], da2, relu_mask=a2)
        else:
            g3.dgrad(gm, wds[2], da2)
            da2 = _relu_mask(da2, a2)
        gws[1] = g2.wgrad_scaled(a1, da2, scales[1], defer=df, owner=ctx.params[1] if df else None)
        da1 = torch.empty_like(a1)
        if ctx.epi:
            g2.dgrad(da2, wds[1], da1, relu_mask=a1)
        else:
            g2.dgrad(da2, wds[1], da1)
            da1 = _relu_mask(da1, a1)
        gws[0] = g1.wgrad_scaled(xh, da1, scales[0], defer=df, owner=ctx.params[0] if df else None)
        if gs is not None:
            gws[3] = gs.wgrad_scaled(xp if ctx.pooled else xh, gm, scales[3], defer=df, owner=ctx.params[3] if df else None)
        if df:
            WgradBatch.flush()
        dx = None
        if ctx.needs_input_grad[0]:
            # the block input is a ReLU output (ResNetVD sets input_is_relu): its mask goes into the LAST pass over its gradient
            mask = ctx.in_relu and _MASK_FUSE()
            fuse = mask and (ctx.epi or ctx.pooled)
            if gs is None:
                dxh = gm
                g1.dgrad(da1, wds[0], dxh, accum=True, relu_mask=xh if fuse else None)
            else:
                dxh = torch.empty_like(xh)
                g1.dgrad(da1, wds[0], dxh)
                if ctx.pooled:
                    dp = torch.empty_like(xp)
                    gs.dgrad(gm, wds[3], dp)
                    avgpool2x2_bwd(dp, dxh, accumulate=True, mask=xh if fuse else None)
                else:
                    gs.dgrad(gm, wds[3], dxh, accum=True, relu_mask=xh if fuse else None)
            if fuse:
                _premask_note(dxh)
            dx = dxh.permute(0, 3, 1, 2)
        return (dx, None, None, None, None, *gws, *([None] * (2 * n)))


def _downsample_avg(cin, cout, stride):
    """resnetvd.py:157-182 (dilation 1): [pool | Identity, 1x1 stride-1 convolution, norm]"""
    return nn.Sequential(AvgPool2x2() if stride != 1 else nn.Identity(), nn.Conv2d(cin, cout, 1, bias=False), FrozenBatchNorm2d(cout))


class ResNetVD(Backbone):
    """resnetvd.py:277-513 with stem_type "deep", stem_width 32, avg_down True and FrozenBatchNorm2d.

    Initialisation mirrors the reference: convolution weights keep nn.Conv2d's default (kaiming_uniform, a = sqrt(5)); the
    reference's constant_ initialisation touches nn.BatchNorm2d instances only, so the frozen norms keep their identity
    buffers - except that `zero_init_last_bn` (default True there, and the builder does not override it) ZEROES every
    block's bn3.weight: a freshly built backbone computes relu(bn3.bias + shortcut) per block until a checkpoint is loaded."""

    def __init__(self, layers=(3, 4, 6, 3), stem_width=32, zero_init_last_bn=True):
        super().__init__()
        if len(layers) != 4:
            raise ValueError("ResNetVD: four stages")
        inplanes = stem_width * 2
        self.conv1 = nn.Sequential(
            nn.Conv2d(3, stem_width, 3, stride=2, padding=1, bias=False), FrozenBatchNorm2d(stem_width), nn.ReLU(inplace=True),
            nn.Conv2d(stem_width, stem_width, 3, stride=1, padding=1, bias=False), FrozenBatchNorm2d(stem_width), nn.ReLU(inplace=True),
            nn.Conv2d(stem_width, inplanes, 3, stride=1, padding=1, bias=False))
        self.bn1 = FrozenBatchNorm2d(inplanes)
        self.act1 = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.stage_names = []
        self._shapes = {}
        net_stride = 4
        for i, (planes, nb) in enumerate(zip((64, 128, 256, 512), layers)):
            stride = 1 if i == 0 else 2
            net_stride *= stride
            blocks = []
            for k in range(nb):
                down = None
                if k == 0 and (stride != 1 or inplanes != planes * BottleneckVD.expansion):
                    down = _downsample_avg(inplanes, planes * BottleneckVD.expansion, stride)
                blocks.append(BottleneckVD(inplanes, planes, stride if k == 0 else 1, down))
                inplanes = planes * BottleneckVD.expansion
            for blk in blocks:
                blk.input_is_relu = True    # every block's input is a ReLU output (the stem's max-pooled ReLU, the previous block)
            name = f"layer{i + 1}"
            self.add_module(name, nn.Sequential(*blocks))
            self.stage_names.append(name)
            self._shapes[f"res{i + 2}"] = ShapeSpec(channels=inplanes, stride=net_stride)
        if zero_init_last_bn:
            for m in self.modules():
                if hasattr(m, "zero_init_last_bn"):
                    m.zero_init_last_bn()
        self._out_features = ["res2", "res3", "res4", "res5"]

    def stem(self, x):
        """x: fp32 NCHW image (already normalised) -> bf16 NCHW (channels_last), stride 4, 64 channels"""
        c = self.conv1
        N, Cin, H, W = x.shape
        He, We = H + (H & 1), W + (W & 1)
        with torch.no_grad():
            if (He, We) != (H, W):       # an odd border: one more zero row / column = the conv's own zero padding
                xp = x.new_zeros(N, Cin, He, We)
                xp[:, :, :H, :W] = x
                x = xp
            x = x.float().contiguous()
            s2d = torch.empty(N, He // 2, We // 2, 16, dtype=torch.bfloat16, device=x.device)
            L.check(L.lib().mi_focus_pack(x.data_ptr(), N, He, We, s2d.data_ptr(), 16, L.stream_ptr()), "mi_focus_pack")
        w0 = c[0].weight
        scale, shift = c[1].affine()
        if w0.requires_grad and torch.is_grad_enabled():
            a = _Stem0Fn.apply(s2d, w0, scale, shift)
        else:
            with torch.no_grad():
                # (a TRAINABLE stem run without autograd is packed per call: kernels that update weights bypass torch's
                #  version counter, see resnet.conv_norm_forward; a frozen one keeps its image)
                key = None if w0.requires_grad else (w0.data_ptr(), w0._version, c[1].__dict__["_affine"][0])
                img = c[0].__dict__.get("_image")
                if key is None or img is None or img[0] != key:
                    wf = _pack_stem(w0 * scale.view(-1, 1, 1, 1))
                    img = (key, _same_address(img, wf) if key is not None else wf)
                    if key is not None:
                        c[0].__dict__["_image"] = img
                a = _stem_conv(s2d, img[1], shift, w0.shape[0])
        a = a.permute(0, 3, 1, 2)
        a = conv_norm_forward(c[3], c[3].weight, c[4], 1, 1, a, relu=True)
        a = conv_norm_forward(c[6], c[6].weight, self.bn1, 1, 1, a, relu=True)
        return _MaxPool.apply(_nhwc(a)).permute(0, 3, 1, 2)

    def forward(self, x):
        if not x.is_cuda:
            raise L.MI355Error("ResNetVD: the MI355X path needs device tensors (no CPU fallback)")
        x = self.stem(x)
        outs = {}
        for name, res in zip(self.stage_names, ("res2", "res3", "res4", "res5")):
            x = getattr(self, name)(x)
            if res != "res2":               # resnetvd.py:505-513: res2 is computed and not returned
                outs[res] = x
        return outs

    def output_shape(self):
        return {k: self._shapes[k] for k in self._out_features}

    def stage_modules(self):
        """layer1 .. layer4 in forward order: single-tensor outputs that cut the backward into stages
        (graph_step.GraphedTrainStep's data-parallel overlap)"""
        return [getattr(self, n) for n in self.stage_names]

    @property
    def size_divisibility(self):
        return 32


@BACKBONE_REGISTRY.register()
def build_resnet_vd_backbone(cfg, input_shape=None):
    """resnetvd.py:516-550.  Served: depth 50 / 101, FrozenBN, no deformable stage"""
    r = cfg.MODEL.RESNETS
    if r.NORM != "FrozenBN":
        raise NotImplementedError(f"build_resnet_vd_backbone: MODEL.RESNETS.NORM {r.NORM!r} (only \"FrozenBN\", the norm of the "
                                  "reference's SparseInst configs, runs here)")
    layers = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}.get(r.DEPTH)
    if layers is None:
        raise NotImplementedError(f"build_resnet_vd_backbone: MODEL.RESNETS.DEPTH {r.DEPTH} (50 or 101)")
    deform = list(r.get("DEFORM_ON_PER_STAGE", [False] * 4))
    if any(deform):
        raise NotImplementedError(f"build_resnet_vd_backbone: MODEL.RESNETS.DEFORM_ON_PER_STAGE {deform} (deformable "
                                  "convolution is not implemented)")
    return ResNetVD(layers)
