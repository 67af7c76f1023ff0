"""TEST INFRASTRUCTURE: an fp32 nn.Module restatement of detectron2's RegNet (modeling/backbone/regnet.py upstream: SimpleStem,
ResBottleneckBlock / BottleneckTransform, AnyStage, AnyNet / RegNet with generate_regnet_parameters and
adjust_block_compatibility) on nn.BatchNorm2d and F.conv2d(groups), carrying d2's state_dict names.  It shares no code with
yolov7_d2_amd/modeling/regnet.py: tests/test_regnet_builder.py compares the two trees' names and shapes, tests/test_gpu_regnet.py
their numbers.

`quant`: optional emulation of the product's bf16 storage - applied where the product stores a map: the network input, every
raw convolution output and every layer / block output (oracle/resnet_oracle.forward's `quant` in spirit); the weights are
rounded as the packed images are.  The restatement with quant against itself without measures the floor bf16 storage leaves."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

TYPES = {
    "RegNetX_200MF": dict(stem_width=32, w_a=36.44, w_0=24, w_m=2.49, group_width=8, depth=13),
    "RegNetX_400MF": dict(stem_width=32, w_a=24.48, w_0=24, w_m=2.54, group_width=16, depth=22),
    "RegNetX_600MF": dict(stem_width=32, w_a=36.97, w_0=48, w_m=2.24, group_width=24, depth=16),
}
# computed with the width rule below on the CPU
EXPECTED = {
    "RegNetX_200MF": dict(widths=[24, 56, 152, 368], depths=[1, 1, 4, 7], group_width=8),
    "RegNetX_400MF": dict(widths=[32, 64, 160, 384], depths=[1, 2, 7, 12], group_width=16),
    "RegNetX_600MF": dict(widths=[48, 96, 240, 528], depths=[1, 3, 5, 7], group_width=24),
}


def bf16(t):
    """storage rounding: fp32 -> bf16 -> fp32, gradient passed straight through (the product's gradients are stored in bf16 as
    well, but each is a separate tensor of its own: the floor measured here is the forward's)"""
    return t + (t.to(torch.bfloat16).float() - t).detach()


def widths_and_depths(w_a, w_0, w_m, d, q=8):
    ws_cont = np.arange(d) * w_a + w_0
    ks = np.round(np.log(ws_cont / w_0) / np.log(w_m))
    ws_all = np.round(np.divide(w_0 * np.power(w_m, ks), q)).astype(int) * q
    ws, ds = np.unique(ws_all, return_counts=True)
    return ws.tolist(), ds.tolist()


def compatible(ws, bs, gs):
    vs = [int(max(1, w * b)) for w, b in zip(ws, bs)]
    gs = [int(min(g, v)) for g, v in zip(gs, vs)]
    ms = [np.lcm(g, b) if b > 1 else g for g, b in zip(gs, bs)]
    vs = [max(m, int(round(v / m) * m)) for v, m in zip(vs, ms)]
    return [int(v / b) for v, b in zip(vs, bs)], bs, gs


class _Q:
    """carries the storage emulation into the modules"""
    fn = None


def _q(t, owner):
    return owner.q.fn(t) if owner.q.fn is not None else t


def _conv(m, x, owner):
    w = _q(m.weight, owner)
    return _q(F.conv2d(x, w, None, m.stride, m.padding, 1, m.groups), owner)


class Stem(nn.Module):
    def __init__(self, w_in, w_out, q):
        super().__init__()
        self.q = q
        self.conv = nn.Conv2d(w_in, w_out, 3, stride=2, padding=1, bias=False)
        self.bn = nn.BatchNorm2d(w_out)

    def forward(self, x):
        return _q(F.relu(self.bn(_conv(self.conv, x, self))), self)


class Transform(nn.Module):
    def __init__(self, w_in, w_out, stride, group_w, q):
        super().__init__()
        self.q = q
        w_b = w_out                                   # bottleneck ratio 1.0
        self.a = nn.Conv2d(w_in, w_b, 1, bias=False)
        self.a_bn = nn.BatchNorm2d(w_b)
        self.b = nn.Conv2d(w_b, w_b, 3, stride=stride, padding=1, groups=w_b // group_w, bias=False)
        self.b_bn = nn.BatchNorm2d(w_b)
        self.c = nn.Conv2d(w_b, w_out, 1, bias=False)
        self.c_bn = nn.BatchNorm2d(w_out)

    def forward(self, x):
        x = _q(F.relu(self.a_bn(_conv(self.a, x, self))), self)
        x = _q(F.relu(self.b_bn(_conv(self.b, x, self))), self)
        return self.c_bn(_conv(self.c, x, self))      # (the tail stores after the add and the ReLU)


class Block(nn.Module):
    def __init__(self, w_in, w_out, stride, group_w, q):
        super().__init__()
        self.q = q
        self.proj, self.bn = None, None
        if w_in != w_out or stride != 1:
            self.proj = nn.Conv2d(w_in, w_out, 1, stride=stride, bias=False)
            self.bn = nn.BatchNorm2d(w_out)
        self.f = Transform(w_in, w_out, stride, group_w, q)

    def forward(self, x):
        x_p = self.bn(_conv(self.proj, x, self)) if self.proj is not None else x
        return _q(F.relu(x_p + self.f(x)), self)


class Stage(nn.Module):
    def __init__(self, w_in, w_out, stride, d, group_w, q):
        super().__init__()
        for i in range(d):
            self.add_module("b%d" % (i + 1), Block(w_in, w_out, stride, group_w, q))
            stride, w_in = 1, w_out

    def forward(self, x):
        for b in self.children():
            x = b(x)
        return x


class RegNetRef(nn.Module):
    def __init__(self, kind, out_features=("s2", "s3", "s4")):
        super().__init__()
        a = TYPES[kind]
        ws, ds = widths_and_depths(a["w_a"], a["w_0"], a["w_m"], a["depth"])
        ws, _, gs = compatible(ws, [1.0] * len(ws), [a["group_width"]] * len(ws))
        self.widths, self.depths, self.group_widths = ws, ds, gs
        self.q = _Q()
        self.out_features = list(out_features)
        self.stem = Stem(3, a["stem_width"], self.q)
        prev = a["stem_width"]
        self.names = []
        for i, (d, w, g) in enumerate(zip(ds, ws, gs)):
            self.add_module("s%d" % (i + 1), Stage(prev, w, 2, d, g, self.q))
            self.names.append("s%d" % (i + 1))
            prev = w
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(mean=0.0, std=float(np.sqrt(2.0 / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels))))

    def forward(self, x, quant=None):
        self.q.fn = quant
        try:
            x = x if quant is None else quant(x)
            out = {}
            x = self.stem(x)
            if "stem" in self.out_features:
                out["stem"] = x
            for n in self.names:
                x = getattr(self, n)(x)
                if n in self.out_features:
                    out[n] = x
            return out
        finally:
            self.q.fn = None


def block(w_in, w_out, stride, group_w):
    """one ResBottleneckBlock of the restatement, d2's init; forward(x, quant=None)"""
    q = _Q()
    b = Block(w_in, w_out, stride, group_w, q)
    for m in b.modules():
        if isinstance(m, nn.Conv2d):
            m.weight.data.normal_(mean=0.0, std=float(np.sqrt(2.0 / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels))))
    return b


def run_block(b, x, quant=None):
    b.q.fn = quant
    try:
        return b(x if quant is None else quant(x))
    finally:
        b.q.fn = None
