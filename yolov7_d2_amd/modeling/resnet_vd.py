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
import functools

import torch
from torch import nn

from .. import _lib as L
from ..d2shim import BACKBONE_REGISTRY, Backbone, ShapeSpec
from ..ops import _conv_desc, _nhwc, _run_conv
from .resnet import (FrozenBatchNorm2d, _BLOCK_FN, _BottleneckFn, _MaxPool, _bottleneck_eager, _frozen_image, _relu_mask,
                     _stem_wgrad, avgpool2x2, avgpool2x2_bwd, conv_norm_forward)


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
        dy = _relu_mask(g.contiguous(), a)
        gw9 = _stem_wgrad(s2d, dy, 4 * Cin, [(t // 3 - 1, t % 3 - 1) for t in range(9)]).view(Cout, 4 * Cin, 3, 3)
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
            return _BottleneckFn.apply(x, self.stride, int(len(pairs) == 4), pooled, getattr(self, "input_is_relu", False),
                                       *[c.weight for c, _ in pairs], *aff)
        convs = [functools.partial(conv_norm_forward, c, c.weight, n, stride, (c.weight.shape[-1] - 1) // 2)
                 for (c, n), stride in zip(pairs, (1, self.stride, 1, 1))]
        shortcut = (lambda t: t) if self.downsample is None else (lambda t: convs[3](self.downsample[0](t)))
        return _bottleneck_eager(x, convs[:3], self.conv3.weight, shortcut)


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
                pack = lambda: _pack_stem(w0 * scale.view(-1, 1, 1, 1))
                wf = pack() if w0.requires_grad else _frozen_image(c[0], w0, c[1], pack)
                a = _stem_conv(s2d, wf, shift, w0.shape[0])
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
