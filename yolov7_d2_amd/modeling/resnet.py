"""detectron2's ResNet-50 (`build_resnet_backbone`, BasicStem + BottleneckBlock, FrozenBatchNorm2d) on the MI355X kernels -
the backbone of BASELINE.json configs 4 / 5 (configs/coco/detr/detr_256_6_6_torchvision.yaml:7-10,
configs/coco/sparseinst/Base-SparseInst.yaml:8).  detectron2 is NOT vendored in the reference and not installed here:
module structure, state_dict keys (`stem.conv1.weight`, `stem.conv1.norm.{weight,bias,running_mean,running_var}`,
`res3.0.shortcut.weight`, `res3.0.conv2.norm.*` ...) and semantics are restated from d2 upstream (parity unpinned: the
CPU restatement is oracle/resnet_oracle.py).

How it runs:
  * every Conv2d + FrozenBatchNorm2d pair is ONE implicit-GEMM launch (torch.ops.mi355.conv2d): the frozen affine
    (scale = w / sqrt(var + 1e-5), shift = b - mean * scale) is folded into the packed weight image and the conv bias -
    a frozen norm has no statistics pass at all;
  * the 7x7 stride-2 stem conv (3 -> 64) is a 4x4 conv over the 2x2 space-to-depth image: the Focus packer of the YOLOX
    stem (mi_focus_pack: fp32 NCHW -> bf16 [N, H/2, W/2, 12+4]) followed by a 16-tap conv with the 7x7 weights scattered
    into an 8x8 kernel (row / column -1 are zero) - no 3-channel implicit GEMM with 13/16 of the k-chunk wasted;
  * ReLU / residual add: mi_ew_bf16; MaxPool2d(3, 2, 1): mi_maxpool3x3s2_*;
  * MODEL.BACKBONE.FREEZE_AT (default 2): the stem and res2 run forward-only (no saved activations, no data / weight
    gradients), exactly the layers detectron2 freezes; FREEZE_AT 0 (SparseInst) trains the stem through the 16-tap
    weight-gradient kernel.
Activations are bf16 NCHW tensors in channels_last memory (= NHWC for the kernels).
"""
import ctypes as C
import os

import torch
from torch import nn

from .. import _lib as L
from ..d2shim import BACKBONE_REGISTRY, Backbone, ShapeSpec
from ..ops import WgradBatch, _ConvGeom, _conv_desc, _ld, _nchw, _nhwc, _nhwc_v, _pad_last, _run_conv, wgrad_can_defer


class FrozenBatchNorm2d(nn.Module):
    """detectron2.layers.FrozenBatchNorm2d: four BUFFERS, eps 1e-5, y = x * scale + shift"""

    def __init__(self, num_features, eps=1e-5):
        super().__init__()
        self.num_features, self.eps = num_features, eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features) - eps)

    def affine(self):
        """(scale, shift), fp32 [C].  The four buffers are constants of a training run: the pair is computed once and kept
        until a buffer is written or replaced (five tiny launches per convolution per step otherwise).

        The two tensors are ADDRESS-STABLE: a changed buffer (load_state_dict, or just a version bump - GraphedTrainStep
        restores every buffer with copy_ after its warm-up passes) recomputes INTO them.  Captured graphs hold their
        addresses as launch arguments; replacing the pair would free memory an earlier capture still reads, and the
        allocator hands it to the next tensor (found with two captured shapes and an eager forward in between: the
        second shape's replays read another tensor's bytes as the BatchNorm shift)."""
        bufs = (self.weight, self.bias, self.running_mean, self.running_var)
        key = tuple((t.data_ptr(), t._version) for t in bufs)
        c = self.__dict__.get("_affine")
        if c is None or c[0] != key:
            with torch.no_grad():
                scale = (self.weight.float() * (self.running_var.float() + self.eps).rsqrt()).contiguous()
                shift = (self.bias.float() - self.running_mean.float() * scale).contiguous()
                if c is not None and c[1].device == scale.device and c[1].shape == scale.shape:
                    c[1].copy_(scale)
                    c[2].copy_(shift)
                    scale, shift = c[1], c[2]
            c = self.__dict__["_affine"] = (key, scale, shift)
        return c[1], c[2]


def _nhwc_view(x):
    """bf16 NCHW tensor -> its NHWC image (no copy when x is channels_last)"""
    return x.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()


class _EwAddRelu(torch.autograd.Function):
    """relu(a + b): the tail of a bottleneck block"""

    @staticmethod
    def forward(ctx, a, b):
        y = torch.empty_like(a)
        L.check(L.lib().mi_ew_bf16(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), 7, L.stream_ptr()), "mi_ew_bf16 add+relu")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = g.contiguous()
        out = torch.empty_like(g)
        L.check(L.lib().mi_ew_bf16(g.data_ptr(), y.data_ptr(), out.data_ptr(), g.numel(), 2, L.stream_ptr()), "mi_ew_bf16 relu'")
        return out, out


def _add_relu(a, b):
    return _EwAddRelu.apply(_nhwc_view(a), _nhwc_view(b)).permute(0, 3, 1, 2)


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xh):          # xh bf16 [N,H,W,C] contiguous
        N, H, W, Cc = xh.shape
        y = torch.empty(N, (H + 1) // 2, (W + 1) // 2, Cc, dtype=torch.bfloat16, device=xh.device)
        if not xh.requires_grad:
            L.check(L.lib().mi_maxpool3x3s2_fwd(xh.data_ptr(), Cc, y.data_ptr(), Cc, N, H, W, Cc, L.stream_ptr()), "maxpool fwd")
            return y
        # training through the stem (FREEZE_AT 0): one byte per output element records where its first maximum sits, the
        # backward reads that instead of re-deriving it from x (and x need not be kept)
        code = torch.empty(N, (H + 1) // 2, (W + 1) // 2, Cc, dtype=torch.uint8, device=xh.device)
        L.check(L.lib().mi_maxpool3x3s2_fwd_idx(xh.data_ptr(), Cc, y.data_ptr(), Cc, code.data_ptr(), N, H, W, Cc, L.stream_ptr()),
                "maxpool fwd")
        ctx.save_for_backward(code)
        ctx.in_shape = (N, H, W, Cc)
        return y

    @staticmethod
    def backward(ctx, g):
        (code,) = ctx.saved_tensors
        N, H, W, Cc = ctx.in_shape
        g = g.contiguous()
        dx = torch.empty(N, H, W, Cc, dtype=torch.bfloat16, device=g.device)
        L.check(L.lib().mi_maxpool3x3s2_bwd_idx(code.data_ptr(), g.data_ptr(), Cc, dx.data_ptr(), Cc, 0, N, H, W, Cc,
                                                L.stream_ptr()), "maxpool bwd")
        return dx


class Conv2d(nn.Module):
    """detectron2.layers.Conv2d(..., bias=False, norm=FrozenBatchNorm2d) as the reference's configs build it"""

    def __init__(self, cin, cout, kernel_size, stride=1, padding=0):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, kernel_size, kernel_size))
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")      # c2_msra_fill
        self.norm = FrozenBatchNorm2d(cout)
        self.stride, self.padding = stride, padding

    def forward(self, x, relu=False, add_relu=None):
        """relu=True: the ReLU that follows runs in the convolution's epilogue (MI_CONV_RELU), one launch instead of two.
        The frozen affine is folded into the packed weight image (scale) and the bias (shift).
        add_relu (no-autograd path only): an NCHW tensor of the output's shape; returns relu(bf16(conv + shift) + add_relu) from
        the convolution's epilogue (MI_CONV_ADDRELU): conv3 + shortcut + ReLU of a frozen bottleneck as one launch"""
        return conv_norm_forward(self, self.weight, self.norm, self.stride, self.padding, x, relu, add_relu)


def conv_norm_forward(owner, weight, norm, stride, padding, x, relu=False, add_relu=None):
    """Conv2d.forward for any (OIHW weight, FrozenBatchNorm2d) pair - modeling/resnet_vd.py keeps them in separate modules
    under timm's names.  owner: the module whose __dict__ keeps the frozen layer's packed image"""
    scale, shift = norm.affine()
    if torch.is_grad_enabled() and (weight.requires_grad or x.requires_grad):
        if add_relu is not None:
            raise L.MI355Error("Conv2d.forward(add_relu=...): only on the frozen / no-autograd path")
        return _FoldedConvFn.apply(x, weight, scale, shift, stride, padding, relu)
    g = _ConvGeom(x.shape, weight.shape, stride, padding)
    with torch.no_grad():
        pack = lambda: g.pack(weight, dgrad=False, scale=scale)[0]
        # a TRAINABLE layer run without autograd (evaluation between training steps) is packed per call: its weight may
        # have been updated by a kernel that torch's version counter does not see (mi_adamw_step_multi, the arena SGD),
        # so no key could tell a stale image from a fresh one.  A frozen layer (FREEZE_AT prefix) keeps its image
        wf = pack() if weight.requires_grad else _frozen_image(owner, weight, norm, pack)
        return _folded_forward(g, x, wf, shift, relu, add_relu)[1]


def _frozen_image(owner, weight, norm, pack):
    """the packed image of a FROZEN layer: a constant, made by pack() once and kept in owner.__dict__.  Keyed on the identity
    + write counters of the weight and of the four norm buffers (load_state_dict / .to() change them), not on the address
    of `scale`: a recomputed scale may be handed the freed one's address.  A changed key re-packs INTO the same tensor"""
    norm.affine()
    key = (weight.data_ptr(), weight._version, norm.__dict__["_affine"][0])
    c = owner.__dict__.get("_image")
    if c is None or c[0] != key:
        c = owner.__dict__["_image"] = (key, _same_address(c, pack()))
    return c[1]


def _same_address(cached, new):
    """a re-packed constant image goes INTO the tensor the previous one lived in (captured graphs hold its address; see
    FrozenBatchNorm2d.affine)"""
    if cached is not None and cached[1].device == new.device and cached[1].shape == new.shape and cached[1].dtype == new.dtype:
        cached[1].copy_(new)
        return cached[1]
    return new


def _folded_forward(g, x, wf, shift, relu, add_relu=None):
    xh = g.pad_in(x)
    y = torch.empty(g.N, g.Ho, g.Wo, g.CoutP, dtype=torch.bfloat16, device=x.device)
    b32 = shift
    if g.CoutP != g.Cout:
        b32 = torch.zeros(g.CoutP, dtype=torch.float32, device=x.device)
        b32[: g.Cout] = shift
    ar = None
    if add_relu is not None:
        if g.CoutP != g.Cout or relu:
            raise L.MI355Error("conv + add + ReLU epilogue: channel count must be a multiple of 32 (and no second ReLU)")
        ar = _nhwc_v(add_relu)
    g.fwd(xh, wf, y, bias=b32, relu=relu, add_relu=ar)
    return xh, _nchw(y, g.Cout)


class _FoldedConvFn(torch.autograd.Function):
    """Conv2d + FrozenBatchNorm2d (+ ReLU) of a TRAINABLE layer as one autograd node: y = act(conv(x, W * scale) + shift).
    One pack launch writes the forward and the data-gradient image (the latter is kept for backward), no bias gradient
    (shift is a buffer), the ReLU mask comes from the saved output, gW = scale * gW'."""

    @staticmethod
    def forward(ctx, x, weight, scale, shift, stride, padding, relu):
        g = _ConvGeom(x.shape, weight.shape, stride, padding)
        need_dx = x.requires_grad
        wf, wd = g.pack(weight, dgrad=need_dx, scale=scale)
        xh, y = _folded_forward(g, x, wf, shift, relu)
        ctx.g, ctx.relu = g, relu
        ctx.save_for_backward(xh, wd, scale, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, grad):
        xh, wd, scale, y = ctx.saved_tensors
        g = ctx.g
        dyh = _nhwc(grad)
        if ctx.relu:
            yh = _nhwc(y)
            gm = torch.empty_like(dyh)
            L.check(L.lib().mi_ew_bf16(dyh.data_ptr(), yh.data_ptr(), gm.data_ptr(), dyh.numel(), 2, L.stream_ptr()), "mi_ew_bf16 relu'")
            dyh = gm
        dyh = _pad_last(dyh, g.CoutP)
        dx = gw = None
        if ctx.needs_input_grad[0]:
            full = g.CinP == g.Cin and not (g.k == 1 and g.s == 2)
            dxh = (torch.empty if full else torch.zeros)(g.N, g.H, g.W, g.CinP, dtype=torch.bfloat16, device=xh.device)
            g.dgrad(dyh, wd, dxh)
            dx = _nchw(dxh, g.Cin)
        if ctx.needs_input_grad[1]:
            gw = g.wgrad_scaled(xh, dyh, scale)
        return dx, gw, None, None, None, None, None


class _StemFn(torch.autograd.Function):
    """trainable stem (MODEL.BACKBONE.FREEZE_AT 0, configs/coco/sparseinst/Base-SparseInst.yaml:7): forward as
    BasicStem.forward; backward = max-pool routing, ReLU mask and the weight gradient of the 16-tap conv (wgrad kernel,
    NT = 16) mapped back from the 4x4 space-to-depth layout to the 7x7 OIHW gradient.  The input image needs no gradient."""

    @staticmethod
    def forward(ctx, s2d, w7, scale, shift):
        N, Hh, Wh, _ = s2d.shape
        Cout, Cin = w7.shape[0], w7.shape[1]
        wf = _pack_w7(w7 * scale.view(-1, 1, 1, 1))
        a = torch.empty(N, Hh, Wh, Cout, dtype=torch.bfloat16, device=s2d.device)
        _run_conv(_conv_desc(s2d.data_ptr(), 16, N, Hh, Wh, wf, 16, a.data_ptr(), Cout, Hh, Wh, Cout, Cout, _STEM_TAPS,
                             bias=shift.float().contiguous(), flags=L.MI_CONV_RELU),
                  "mi_conv2d (7x7 stem as 4x4 over space-to-depth, ReLU in the epilogue)")
        out = torch.empty(N, (Hh + 1) // 2, (Wh + 1) // 2, Cout, dtype=torch.bfloat16, device=s2d.device)
        code = torch.empty(N, (Hh + 1) // 2, (Wh + 1) // 2, Cout, dtype=torch.uint8, device=s2d.device)
        L.check(L.lib().mi_maxpool3x3s2_fwd_idx(a.data_ptr(), Cout, out.data_ptr(), Cout, code.data_ptr(), N, Hh, Wh, Cout,
                                                L.stream_ptr()), "maxpool")
        ctx.save_for_backward(s2d, a, scale, code)
        ctx.shape = (Cout, Cin)
        return out

    @staticmethod
    def backward(ctx, g):
        s2d, a, scale, code = ctx.saved_tensors
        Cout, Cin = ctx.shape
        N, Hh, Wh, _ = s2d.shape
        g = g.contiguous()
        da = torch.empty_like(a)
        lib = L.lib()
        L.check(lib.mi_maxpool3x3s2_bwd_idx(code.data_ptr(), g.data_ptr(), Cout, da.data_ptr(), Cout, 0, N, Hh, Wh, Cout,
                                            L.stream_ptr()), "maxpool bwd")
        dy = torch.empty_like(a)
        L.check(lib.mi_ew_bf16(da.data_ptr(), a.data_ptr(), dy.data_ptr(), a.numel(), 2, L.stream_ptr()), "relu bwd")
        gw4 = _stem_wgrad(s2d, dy, 4 * Cin, [(dy_, dx_) for dy_, dx_, _ in _STEM_TAPS])
        # [Cout][(px*2+py)*Cin + c][Ay][Ax] -> 8x8 kernel rows R = 2 Ay + py -> drop the zero row / column -> 7x7
        g8 = gw4.view(Cout, 2, 2, Cin, 4, 4).permute(0, 3, 4, 2, 5, 1).reshape(Cout, Cin, 8, 8)
        gw7 = g8[:, :, 1:, 1:] * scale.view(-1, 1, 1, 1)
        dshift = dy.float().sum((0, 1, 2)) if ctx.needs_input_grad[3] else None     # (a FrozenBN shift has none)
        return None, gw7, None, dshift


_STEM_TAPS = [(ay - 2, ax - 2, ay * 4 + ax) for ay in range(4) for ax in range(4)]


def _stem_wgrad(s2d, dy, cin, taps):
    """weight gradient of a stride-1 stem convolution over the space-to-depth image: s2d bf16 [N, Hh, Wh, 16] (its first
    `cin` channels are real), dy bf16 [N, Hh, Wh, Cout], taps [(dy, dx)] (1, 9 or 16 of them) -> fp32 [Cout, cin, len(taps)].
    The mapping back to the 7x7 / 3x3 OIHW gradient stays with the caller"""
    N, Hh, Wh, _ = s2d.shape
    Cout = dy.shape[-1]
    gw = torch.empty(Cout, cin, len(taps), dtype=torch.float32, device=dy.device)
    d = L.mi_wgrad_desc()
    d.x, d.dy, d.gw = s2d.data_ptr(), dy.data_ptr(), gw.data_ptr()
    d.ldx, d.ldy, d.N, d.H, d.W, d.outH, d.outW, d.stride = 16, Cout, N, Hh, Wh, Hh, Wh, 1
    d.Cin, d.Cout, d.CinPad, d.CoutPad, d.ntaps = cin, Cout, 16, Cout, len(taps)
    for t, (dy_, dx_) in enumerate(taps):
        d.tap_dy[t], d.tap_dx[t] = dy_, dx_
    need = L.lib().mi_conv2d_wgrad_plan(C.byref(d))
    L.check(need, "mi_conv2d_wgrad_plan (stem)")
    ws = torch.empty(max(int(need), 16), dtype=torch.uint8, device=dy.device)
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
    L.check(L.lib().mi_conv2d_wgrad(C.byref(d), L.stream_ptr()), "mi_conv2d_wgrad (stem)")
    return gw


def _w7_to_w4(w7s):
    """7x7 kernel -> 8x8 with a zero first row / column -> [Cout][q = py + 2 px][c] x 4x4 taps (ay, ax in -2..1)"""
    Cout, Cin = w7s.shape[:2]
    w8 = w7s.new_zeros(Cout, Cin, 8, 8)
    w8[:, :, 1:, 1:] = w7s
    return w8.view(Cout, Cin, 4, 2, 4, 2).permute(0, 5, 3, 1, 2, 4).reshape(Cout, 4 * Cin, 4, 4)   # ch = (px*2+py)*Cin+c


def _pack_w7(w7s):
    """the (scaled) 7x7 stem weight -> the forward image of its 16-tap form"""
    Cout, Cin = w7s.shape[:2]
    w4 = _w7_to_w4(w7s).contiguous()
    wf = torch.empty(16 * 16 * Cout, dtype=torch.bfloat16, device=w7s.device)
    L.check(L.lib().mi_pack_conv_weight(w4.data_ptr(), Cout, 4 * Cin, 4, 4, wf.data_ptr(), 16, Cout, None, 0, 0, L.stream_ptr()),
            "mi_pack_conv_weight (stem)")
    return wf


class BasicStem(nn.Module):
    def __init__(self, cin=3, cout=64):
        super().__init__()
        self.conv1 = Conv2d(cin, cout, 7, stride=2, padding=3)
        self.out_channels = cout

    def forward(self, x):
        """x: fp32 NCHW image (already normalised).  7x7 s2 conv + frozen norm + ReLU + max-pool."""
        w7 = self.conv1.weight
        scale, shift = self.conv1.norm.affine()
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
        if w7.requires_grad and torch.is_grad_enabled():
            return _StemFn.apply(s2d, w7, scale, shift).permute(0, 3, 1, 2)
        with torch.no_grad():       # frozen stem (FREEZE_AT >= 1): the packed image is a constant, kept across steps
            Cout = w7.shape[0]
            # (a TRAINABLE stem run without autograd is packed per call: kernels that update weights bypass torch's
            #  version counter, see conv_norm_forward)
            pack = lambda: _pack_w7(w7 * scale.view(-1, 1, 1, 1))
            wf = pack() if w7.requires_grad else _frozen_image(self, w7, self.conv1.norm, pack)
            Hh, Wh = He // 2, We // 2
            a = torch.empty(N, Hh, Wh, Cout, dtype=torch.bfloat16, device=x.device)
            _run_conv(_conv_desc(s2d.data_ptr(), 16, N, Hh, Wh, wf, 16, a.data_ptr(), Cout, Hh, Wh, Cout, Cout, _STEM_TAPS,
                                 bias=shift, flags=L.MI_CONV_RELU), "mi_conv2d (7x7 stem as 4x4 over space-to-depth)")
            out = torch.empty(N, (Hh + 1) // 2, (Wh + 1) // 2, Cout, dtype=torch.bfloat16, device=x.device)
            L.check(L.lib().mi_maxpool3x3s2_fwd(a.data_ptr(), Cout, out.data_ptr(), Cout, N, Hh, Wh, Cout, L.stream_ptr()),
                    "maxpool fwd")
            return out.permute(0, 3, 1, 2)


def _BLOCK_FN():
    """MI_RESNET_BLOCK_FN=0: every convolution of a trainable bottleneck block is its own autograd node again (A/B switch)"""
    return os.environ.get("MI_RESNET_BLOCK_FN", "1") != "0"


def _EPI_FUSE():
    """MI_RESNET_EPI_FUSE (default 1 since round 4; 0 restores the three elementwise passes per block): the block's conv3 +
    shortcut + ReLU and the two ReLU backward masks run in convolution epilogues (MI_CONV_ADDRELU / MI_CONV_RELUMASK, the tile
    kernel's EPI 2 instantiations).  First device run + same-call A/B in round 4 (profiles/r04_epi_fuse_ab.txt): DETR-R50
    bs 4 213-216 -> 218.6-219.5 images/s, SparseInst bs 8 353-371 -> 379-382; forward output identical, gradients within one
    bf16 ulp at tensor scale where the masked data gradients change kernel family
    (tests/test_gpu_resnet.py::test_bottleneck_epilogue_fusions_equal_the_elementwise_passes)."""
    return os.environ.get("MI_RESNET_EPI_FUSE", "1") == "1"


def _relu_mask(g, a):
    """g * (a > 0) (bf16, same shape)"""
    out = torch.empty_like(g)
    L.check(L.lib().mi_ew_bf16(g.data_ptr(), a.data_ptr(), out.data_ptr(), g.numel(), 2, L.stream_ptr()), "mi_ew_bf16 relu'")
    return out


# Gradients that leave a bottleneck's backward ALREADY multiplied by the ReLU mask of the tensor they belong to (the block's
# input is the previous block's ReLU output: the last data gradient into it applies (x > 0) in its epilogue, MI_CONV_ACCUM |
# MI_CONV_RELUMASK), so that the previous block's backward skips its own mask pass - a read-read-write of the block's largest
# map, 13 launches per DETR-R50 step.  Keyed by (address, autograd graph task): an entry is only believed inside the backward
# pass that made it.  Correct for any consumer: the producer of a ReLU output multiplies its out-gradient by that mask anyway,
# and the mask is idempotent; a gradient that autograd summed from several consumers is a new tensor and is masked as before.
_PREMASKED = {}


def _premask_note(t):
    task = torch._C._current_graph_task_id()
    for k in [k for k, v in _PREMASKED.items() if v != task]:
        del _PREMASKED[k]
    _PREMASKED[t.data_ptr()] = task


def _premask_take(t):
    return _PREMASKED.pop(t.data_ptr(), None) == torch._C._current_graph_task_id()


def _MASK_FUSE():
    """MI_RESNET_MASK_FUSE=0: every block masks its own out-gradient with a separate pass (round 5's form; A/B, tests)"""
    return os.environ.get("MI_RESNET_MASK_FUSE", "1") == "1"


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


class _BottleneckFn(torch.autograd.Function):
    """A trainable bottleneck (conv1 1x1 - conv2 3x3 of stride s2 - conv3 1x1, FrozenBN folded, + shortcut, ReLU) as ONE
    autograd node: detectron2's BottleneckBlock and the ResNet-vd block (modeling/resnet_vd.py).  The shortcut is
      ssc 0:               the block input itself (identity block);
      ssc s, not pooled:   a 1x1 convolution of stride s on the input (d2: s = the block's stride; vd layer1.0: s = 1);
      ssc 1, pooled:       a 1x1 stride-1 convolution on xp = avgpool2x2(input) (vd, stride-2 blocks).
    What the per-convolution nodes cannot do: the block input's gradient is the sum of two paths - autograd materialised both
    and added them (a three-tensor pass over the block's largest map, and a full zero fill under the stride-2 shortcut's data
    gradient, which writes only the even pixels); here the second path ACCUMULATES into the first in the convolution's epilogue
    (MI_CONV_ACCUM): identity blocks add conv1's data gradient into the (masked) output gradient, shortcut blocks add the
    shortcut's data gradient into conv1's.  The pooled shortcut's data gradient is a quarter-size map that
    mi_avgpool2x2s2_bwd adds into conv1's - a pass over every pixel of the block input, so the input's ReLU mask is taken there
    (and noted for the previous block) for stride-2 blocks too, which the strided convolution's accumulate, visiting only the
    even pixels, cannot do.  Same kernels, same roundings as the separate nodes (bf16 + bf16 -> bf16)."""

    @staticmethod
    def forward(ctx, x, s2, ssc, pooled, in_relu, *rest):
        n = 4 if ssc else 3
        ws, aff = rest[:n], rest[n:]
        scales, shifts = aff[0::2], aff[1::2]
        need_dx = x.requires_grad
        N, Cin, H, W = x.shape
        bc = ws[0].shape[0]
        g1 = _ConvGeom((N, Cin, H, W), ws[0].shape, 1, 0)
        g2 = _ConvGeom((N, bc, H, W), ws[1].shape, s2, 1)
        g3 = _ConvGeom((N, bc, g2.Ho, g2.Wo), ws[2].shape, 1, 0)
        Hp, Wp = ((H + 1) // 2, (W + 1) // 2) if pooled else (H, W)
        gs = _ConvGeom((N, Cin, Hp, Wp), ws[3].shape, ssc, 0) if ssc else None
        geoms = [g1, g2, g3] + ([gs] if ssc else [])
        for g in geoms:
            if g.CinP != g.Cin or g.CoutP != g.Cout:
                raise L.MI355Error("ResNet bottleneck: channel counts must be multiples of 32")
        if (ssc and (gs.Ho, gs.Wo) != (g2.Ho, g2.Wo)) or (not ssc and (s2 != 1 or Cin != ws[2].shape[0])):
            raise L.MI355Error("ResNet bottleneck: the shortcut's map does not match conv3's")
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
        xp = avgpool2x2(xh) if pooled else None
        sc = run(gs, xp if pooled else xh, 3, False) if ssc else xh
        ctx.epi = _EPI_FUSE()
        if ctx.epi:
            y = run(g3, a2, 2, False, add_relu=sc)            # relu(bf16(conv3 + shift) + shortcut) in conv3's epilogue
        else:
            o = run(g3, a2, 2, False)
            y = torch.empty_like(o)
            L.check(L.lib().mi_ew_bf16(o.data_ptr(), sc.data_ptr(), y.data_ptr(), o.numel(), 7, L.stream_ptr()), "mi_ew_bf16 add+relu")
        ctx.geoms, ctx.pooled, ctx.in_relu = geoms, bool(pooled), bool(in_relu)
        ctx.params = ws
        ctx.save_for_backward(xh, a1, a2, y, xp, *[im[1] for im in imgs], *scales)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        n = len(ctx.geoms)
        xh, a1, a2, y, xp = ctx.saved_tensors[:5]
        wds, scales = ctx.saved_tensors[5:5 + n], ctx.saved_tensors[5 + n:]
        g1, g2, g3 = ctx.geoms[:3]
        gs = ctx.geoms[3] if n == 4 else None
        gyh = _nhwc(gy)
        if _premask_take(gyh):
            gm = gyh                        # the next block's backward masked it in its last pass (and owns no other use of it)
        else:
            gm = _relu_mask(gyh, y)         # (a fresh tensor: identity blocks accumulate the input gradient into it)
        gws = [None] * n
        # the block's three or four weight gradients as ONE grouped launch (ops.WgradBatch), issued below - before the input
        # gradient is accumulated INTO gm, which two of the jobs read
        df = wgrad_can_defer(*ctx.params)
        owner = lambda i: ctx.params[i] if df else None
        gws[2] = g3.wgrad_scaled(a2, gm, scales[2], defer=df, owner=owner(2))
        da2 = torch.empty_like(a2)
        if ctx.epi:
            g3.dgrad(gm, wds[2], da2, relu_mask=a2)
        else:
            g3.dgrad(gm, wds[2], da2)
            da2 = _relu_mask(da2, a2)
        gws[1] = g2.wgrad_scaled(a1, da2, scales[1], defer=df, owner=owner(1))
        da1 = torch.empty_like(a1)
        if ctx.epi:
            g2.dgrad(da2, wds[1], da1, relu_mask=a1)
        else:
            g2.dgrad(da2, wds[1], da1)
            da1 = _relu_mask(da1, a1)
        gws[0] = g1.wgrad_scaled(xh, da1, scales[0], defer=df, owner=owner(0))
        if gs is not None:
            gws[3] = gs.wgrad_scaled(xp if ctx.pooled else xh, gm, scales[3], defer=df, owner=owner(3))
        if df:
            WgradBatch.flush()
        dx = None
        if ctx.needs_input_grad[0]:
            # the block input is a ReLU output (the backbones set input_is_relu): its mask goes into the LAST pass over its
            # gradient - the pool's backward, or the last data gradient's epilogue (not the stride-2 shortcut's, whose
            # accumulate visits only the even pixels)
            fuse = ctx.in_relu and _MASK_FUSE() and (ctx.pooled or (ctx.epi and (gs is None or gs.s == 1)))
            mask = xh if fuse else None
            if gs is None:
                dxh = gm
                g1.dgrad(da1, wds[0], dxh, accum=True, relu_mask=mask)
            else:
                dxh = torch.empty_like(xh)
                g1.dgrad(da1, wds[0], dxh)
                if ctx.pooled:
                    dp = torch.empty_like(xp)
                    gs.dgrad(gm, wds[3], dp)
                    avgpool2x2_bwd(dp, dxh, accumulate=True, mask=mask)
                else:
                    gs.dgrad(gm, wds[3], dxh, accum=True, relu_mask=mask)
            if fuse:
                _premask_note(dxh)
            dx = dxh.permute(0, 3, 1, 2)
        return (dx, None, None, None, None, *gws, *([None] * (2 * n)))


def _bottleneck_eager(x, convs, w3, shortcut):
    """A bottleneck as per-convolution launches / autograd nodes: conv1 + ReLU, conv2 + ReLU, shortcut(x), conv3 + shortcut
    + ReLU.  convs: conv1 .. conv3 as callables (input, relu=False, add_relu=None) - detectron2-shaped blocks pass their
    Conv2d MODULES, whose forward hooks the tests use to read every convolution's output; w3: conv3's weight"""
    out = convs[1](convs[0](x, relu=True), relu=True)
    return _conv3_add_relu(convs[2], w3, out, shortcut(x))


def _conv3_add_relu(conv3, w3, out, sc):
    """relu(conv3(out) + sc).  Without autograd (a frozen block under FREEZE_AT, inference) the add + ReLU run in conv3's
    epilogue, as _BottleneckFn does for the trainable blocks - the separate pass was a read-read-write of the block's
    largest map (3 x 73 us per DETR-R50 step for res2 at 800 x 1333)"""
    autograd = torch.is_grad_enabled() and (out.requires_grad or sc.requires_grad or w3.requires_grad)
    if not autograd and _EPI_FUSE() and w3.shape[0] % 32 == 0:
        return conv3(out, add_relu=sc)
    return _add_relu(conv3(out), sc)


class BottleneckBlock(nn.Module):
    def __init__(self, cin, cout, bottleneck_channels, stride=1, stride_in_1x1=False):
        super().__init__()
        self.shortcut = Conv2d(cin, cout, 1, stride=stride) if cin != cout else None
        s1, s3 = (stride, 1) if stride_in_1x1 else (1, stride)
        self.conv1 = Conv2d(cin, bottleneck_channels, 1, stride=s1)
        self.conv2 = Conv2d(bottleneck_channels, bottleneck_channels, 3, stride=s3, padding=1)
        self.conv3 = Conv2d(bottleneck_channels, cout, 1)
        self.stride = stride

    def forward(self, x):
        convs = [self.conv1, self.conv2, self.conv3] + ([self.shortcut] if self.shortcut is not None else [])
        if (_BLOCK_FN() and torch.is_grad_enabled() and all(c.weight.requires_grad for c in convs) and self.conv1.stride == 1):
            aff = [t for c in convs for t in c.norm.affine()]
            return _BottleneckFn.apply(x, self.conv2.stride, self.shortcut.stride if self.shortcut is not None else 0, False,
                                       getattr(self, "input_is_relu", False), *[c.weight for c in convs], *aff)
        return _bottleneck_eager(x, convs[:3], self.conv3.weight, self.shortcut if self.shortcut is not None else (lambda t: t))


def _DEFORM_KEEP_COL():
    """MI_DEFORM_KEEP_COL (default 1): a DeformConv keeps its sampled columns for the backward pass (9x its input, read once
    by the weight gradient); 0 samples them again there - one more mi_deform_im2col per layer, nothing kept
    (profiles/deform_conv_probe.txt has both)"""
    return os.environ.get("MI_DEFORM_KEEP_COL", "1") != "0"


def _offset_operand(offset, N, Ho, Wo):
    """offset [N, 18, Ho, Wo] -> (tensor to keep alive, pixel stride): read IN PLACE when it is the channel slice of a bf16
    NHWC map (what mi355::conv2d returns for 18 outputs: rows of 32), a padded NHWC copy otherwise"""
    if tuple(offset.shape) != (N, 18, Ho, Wo):
        raise L.MI355Error(f"DeformConv: offset {tuple(offset.shape)} is not [N, 18, Ho, Wo] = {(N, 18, Ho, Wo)}")
    if offset.dtype == torch.bfloat16:
        sn, sc, sh, sw = offset.stride()
        if sc == 1 and sw >= 18 and (Ho == 1 or sh == Wo * sw) and (N == 1 or sn == Ho * Wo * sw):
            return offset, sw
    return _pad_last(_nhwc(offset.detach()), 32), 32


def _deform_cols(xh, off, ldoff, Ho, Wo, stride):
    """sampled im2col: bf16 [N, Ho, Wo, 9 * C], tap-major, the C channels of a tap contiguous"""
    N, H, W, Cc = xh.shape
    col = torch.empty(N, Ho, Wo, 9 * Cc, dtype=torch.bfloat16, device=xh.device)
    L.check(L.lib().mi_deform_im2col(xh.data_ptr(), _ld(xh), off.data_ptr(), ldoff, col.data_ptr(), N, H, W, Cc, stride, 1, 1,
                                     L.stream_ptr()), "mi_deform_im2col")
    return col


def _deform_geom(x_shape, w_shape, stride):
    """the 1x1 convolution over the sampled columns: [N, 9 * C, Ho, Wo] -> [N, Cout, Ho, Wo]"""
    N, Cin, H, W = x_shape
    Cout, cw, kh, kw = w_shape
    if (cw, kh, kw) != (Cin, 3, 3) or stride not in (1, 2) or Cin % 32 or Cout % 32:
        raise L.MI355Error(f"DeformConv: weight {tuple(w_shape)} on {Cin} channels, stride {stride} (served: 3x3, stride 1 or 2, "
                           "padding 1, dilation 1, one group, channel counts in multiples of 32)")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return _ConvGeom((N, 9 * Cin, Ho, Wo), (Cout, 9 * Cin, 1, 1), 1, 0)


def _tap_major(weight):
    """[Cout, C, 3, 3] -> [Cout, 9 * C, 1, 1] in the columns' order (tap-major, channels inside a tap)"""
    return weight.detach().permute(0, 2, 3, 1).reshape(weight.shape[0], -1, 1, 1)


class _DeformConvFn(torch.autograd.Function):
    """DeformConv + FrozenBatchNorm2d (+ ReLU) as one autograd node over (x, offset, weight): sampled im2col, then the
    1x1 route of the convolution kernels with the folded scale / shift / ReLU in its epilogue (as _FoldedConvFn).
    Backward: dcol = 1x1 data gradient, gW = weight gradient on (col, dy) permuted back to OIHW, mi_deform_col2im for
    d_offset and the fp32 dx sum, one pass to bf16 dx that also applies the input's ReLU mask (x_is_relu)."""

    @staticmethod
    def forward(ctx, x, offset, weight, scale, shift, stride, relu, x_is_relu):
        g = _deform_geom(x.shape, weight.shape, stride)
        xh = _nhwc_v(x)
        off, ldoff = _offset_operand(offset, g.N, g.H, g.W)
        col = _deform_cols(xh, off, ldoff, g.H, g.W, stride)
        wf, wd = g.pack(_tap_major(weight), dgrad=True, scale=scale)
        y = torch.empty(g.N, g.Ho, g.Wo, g.CoutP, dtype=torch.bfloat16, device=x.device)
        g.fwd(col, wf, y, bias=shift, relu=relu)
        ctx.g, ctx.relu, ctx.stride, ctx.ldoff, ctx.x_is_relu = g, relu, stride, ldoff, x_is_relu
        ctx.save_for_backward(xh, off, wd, scale, y if relu else None, col if _DEFORM_KEEP_COL() else None)
        return _nchw(y, g.Cout)

    @staticmethod
    def backward(ctx, grad):
        xh, off, wd, scale, y, col = ctx.saved_tensors
        g, stride = ctx.g, ctx.stride
        N, H, W, Cc = xh.shape
        lib, sp = L.lib(), L.stream_ptr()
        dyh = _nhwc(grad)
        if ctx.relu:
            dyh = _relu_mask(dyh, y)
        if col is None:
            col = _deform_cols(xh, off, ctx.ldoff, g.H, g.W, stride)
        gw = None
        if ctx.needs_input_grad[2]:
            gw9 = g.wgrad_scaled(col, dyh, scale)
            gw = gw9.view(g.Cout, 3, 3, Cc).permute(0, 3, 1, 2).contiguous()
        dx = doff = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dcol = torch.empty_like(col)
            g.dgrad(dyh, wd, dcol)
            # (zeroed by a kernel: a memset node in a captured step serialises the graph's branches,
            #  profiles/r04_graph_memset_finding.txt)
            # the fp32 sum and, behind it, max |dcol|: col2im rounds its addends to a grid derived from that maximum, so that
            # the float atomics give the same bits in any order (a bf16 backward pass amplifies one differing bit to its
            # rounding-noise floor within a few layers: eager and captured steps would part ways)
            n32 = N * H * W * Cc
            buf = torch.empty(n32 + 4, dtype=torch.float32, device=xh.device)
            dx32, gmax = buf[:n32], buf[n32:]
            L.check(lib.mi_deform_zero_f32(buf.data_ptr(), buf.numel(), sp), "mi_deform_zero_f32")
            L.check(lib.mi_deform_absmax(dcol.data_ptr(), dcol.numel(), gmax.data_ptr(), sp), "mi_deform_absmax")
            doffh = torch.empty(N, g.H, g.W, 32, dtype=torch.bfloat16, device=xh.device)
            L.check(lib.mi_deform_col2im(dcol.data_ptr(), xh.data_ptr(), _ld(xh), off.data_ptr(), ctx.ldoff, dx32.data_ptr(),
                                         doffh.data_ptr(), gmax.data_ptr(), N, H, W, Cc, stride, 1, 1, sp), "mi_deform_col2im")
            if ctx.needs_input_grad[1]:
                doff = _nchw(doffh, 18)
            if ctx.needs_input_grad[0]:
                dxh = torch.empty(N, H, W, Cc, dtype=torch.bfloat16, device=xh.device)
                mask = xh if ctx.x_is_relu else None
                L.check(lib.mi_deform_dx_finish(dx32.data_ptr(), L.ptr(mask), _ld(xh) if mask is not None else 0, dxh.data_ptr(), Cc,
                                                N * H * W, Cc, sp), "mi_deform_dx_finish")
                dx = dxh.permute(0, 3, 1, 2)
        return dx, doff, gw, None, None, None, None, None


class DeformConv(nn.Module):
    """detectron2.layers.DeformConv(cin, cout, 3, stride, padding=1, bias=False, norm=FrozenBatchNorm2d): unmodulated, one
    deformable group, groups 1.  forward(x, offset): offset [N, 18, Ho, Wo], channel 2t / 2t + 1 = row / column offset of tap
    t = i * 3 + j.  The operator is csrc/deform_conv.hip."""

    def __init__(self, cin, cout, stride=1):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, 3, 3))
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")      # c2_msra_fill (DeformBottleneckBlock)
        self.norm = FrozenBatchNorm2d(cout)
        self.stride, self.padding = stride, 1

    def forward(self, x, offset, relu=False, x_is_relu=False):
        """relu: the ReLU that follows runs in the GEMM's epilogue.  x_is_relu: x is a ReLU output - its mask is applied to
        the data gradient in the pass that rounds it to bf16 (x's producer may mask again - the block's conv1 does, its
        output also feeds conv2_offset and autograd sums the two gradients into a new tensor; the mask is idempotent)"""
        if not x.is_cuda:
            raise L.MI355Error("DeformConv: the MI355X path needs device tensors (no CPU fallback)")
        scale, shift = self.norm.affine()
        weight = self.weight
        grad_on = torch.is_grad_enabled() and (weight.requires_grad or x.requires_grad or offset.requires_grad)
        if grad_on:
            return _DeformConvFn.apply(x, offset, weight, scale, shift, self.stride, relu, x_is_relu)
        # no autograd (evaluation, a frozen stage): nothing saved; a frozen layer's packed image is a constant (Conv2d.forward)
        with torch.no_grad():
            g = _deform_geom(x.shape, weight.shape, self.stride)
            pack = lambda: g.pack(_tap_major(weight), dgrad=False, scale=scale)[0]
            wf = pack() if weight.requires_grad else _frozen_image(self, weight, self.norm, pack)
            xh = _nhwc_v(x)
            off, ldoff = _offset_operand(offset, g.N, g.H, g.W)
            col = _deform_cols(xh, off, ldoff, g.H, g.W, self.stride)
            y = torch.empty(g.N, g.Ho, g.Wo, g.CoutP, dtype=torch.bfloat16, device=x.device)
            g.fwd(col, wf, y, bias=shift, relu=relu)
            return _nchw(y, g.Cout)


class DeformBottleneckBlock(nn.Module):
    """detectron2 resnet.py DeformBottleneckBlock (deform_modulated False, one deformable group): conv1 1x1 + ReLU,
    conv2_offset = plain 3x3 convolution with bias and no norm (18 outputs, the 3x3's stride, zero-initialised), conv2 =
    DeformConv + norm + ReLU, conv3 1x1 + shortcut + ReLU.  Every convolution is its own autograd node."""

    def __init__(self, cin, cout, bottleneck_channels, stride=1, stride_in_1x1=False):
        super().__init__()
        self.shortcut = Conv2d(cin, cout, 1, stride=stride) if cin != cout else None
        s1, s3 = (stride, 1) if stride_in_1x1 else (1, stride)
        self.conv1 = Conv2d(cin, bottleneck_channels, 1, stride=s1)
        self.conv2_offset = nn.Conv2d(bottleneck_channels, 18, 3, stride=s3, padding=1)
        self.conv2 = DeformConv(bottleneck_channels, bottleneck_channels, stride=s3)
        self.conv3 = Conv2d(bottleneck_channels, cout, 1)
        nn.init.constant_(self.conv2_offset.weight, 0)
        nn.init.constant_(self.conv2_offset.bias, 0)
        self.stride = stride

    def forward(self, x):
        if not x.is_cuda:
            raise L.MI355Error("DeformBottleneckBlock: the MI355X path needs device tensors (no CPU fallback)")
        out = self.conv1(x, relu=True)
        po = self.conv2_offset
        offset = torch.ops.mi355.conv2d(out, po.weight, po.bias, po.stride[0], 1)
        out = self.conv2(out, offset, relu=True, x_is_relu=True)
        sc = self.shortcut(x) if self.shortcut is not None else x
        return _conv3_add_relu(self.conv3, self.conv3.weight, out, sc)


class ResNet(Backbone):
    def __init__(self, depth=50, out_features=("res5",), freeze_at=2, stride_in_1x1=False, deform_on_per_stage=(False,) * 4):
        """deform_on_per_stage (res2 .. res5): every block of a true stage is a DeformBottleneckBlock (d2's make_stage)"""
        super().__init__()
        if len(deform_on_per_stage) != 4:
            raise ValueError(f"ResNet: deform_on_per_stage {deform_on_per_stage} must have one entry per stage res2 .. res5")
        blocks = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}[depth]
        self.stem = BasicStem(3, 64)
        self._out_features = list(out_features)
        self._shapes = {"stem": ShapeSpec(channels=64, stride=4)}
        cin, bc, cout, stride = 64, 64, 256, 4
        self.stage_names = []
        for i, nb in enumerate(blocks):
            name = f"res{i + 2}"
            first = 1 if i == 0 else 2
            block = DeformBottleneckBlock if deform_on_per_stage[i] else BottleneckBlock
            stage = nn.Sequential(*[block(cin if k == 0 else cout, cout, bc, stride=first if k == 0 else 1,
                                          stride_in_1x1=stride_in_1x1) for k in range(nb)])
            for blk in stage:
                blk.input_is_relu = True    # every block's input is a ReLU output (the stem's max-pooled ReLU, the previous block)
            self.add_module(name, stage)
            self.stage_names.append(name)
            stride *= first
            self._shapes[name] = ShapeSpec(channels=cout, stride=stride)
            cin, bc, cout = cout, bc * 2, cout * 2
        self.freeze(freeze_at)

    def freeze(self, freeze_at):
        """detectron2 ResNet.freeze: 1 = stem, 2 = stem + res2, ..."""
        if freeze_at >= 1:
            for p in self.stem.parameters():
                p.requires_grad = False
        for idx, name in enumerate(self.stage_names, start=2):
            if freeze_at >= idx:
                for p in getattr(self, name).parameters():
                    p.requires_grad = False
        return self

    def forward(self, x):
        if not x.is_cuda:
            raise L.MI355Error("ResNet: the MI355X path needs device tensors (no CPU fallback)")
        outs = {}
        x = self.stem(x)
        if "stem" in self._out_features:
            outs["stem"] = x
        for name in self.stage_names:
            x = getattr(self, name)(x)
            if name in self._out_features:
                outs[name] = x
        return outs

    def output_shape(self):
        return {k: self._shapes[k] for k in self._out_features}

    def stage_modules(self):
        """res2 .. res5 in forward order: single-tensor outputs that cut the backward into stages
        (graph_step.GraphedTrainStep's data-parallel overlap)"""
        return [getattr(self, n) for n in self.stage_names]

    @property
    def size_divisibility(self):
        return 0


@BACKBONE_REGISTRY.register()
def build_resnet_backbone(cfg, input_shape=None):
    r = cfg.MODEL.RESNETS
    if r.NORM != "FrozenBN":
        raise NotImplementedError("build_resnet_backbone: MODEL.RESNETS.NORM FrozenBN (the reference's DETR / SparseInst configs)")
    deform = [bool(d) for d in r.get("DEFORM_ON_PER_STAGE", [False] * 4)]
    if any(deform):
        if r.get("DEFORM_MODULATED", False):
            raise NotImplementedError("build_resnet_backbone: MODEL.RESNETS.DEFORM_MODULATED True (the modulated form is not "
                                      "served: csrc/deform_conv.hip is detectron2's unmodulated DeformConv)")
        if r.get("DEFORM_NUM_GROUPS", 1) != 1:
            raise NotImplementedError(f"build_resnet_backbone: MODEL.RESNETS.DEFORM_NUM_GROUPS {r.get('DEFORM_NUM_GROUPS')} "
                                      "(served: one deformable group)")
    return ResNet(depth=r.DEPTH, out_features=r.OUT_FEATURES, freeze_at=cfg.MODEL.BACKBONE.FREEZE_AT,
                  stride_in_1x1=r.STRIDE_IN_1X1, deform_on_per_stage=deform)
