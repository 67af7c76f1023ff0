"""Test support: an fp32 torch restatement of the reference's ResNet-vd (yolov7/modeling/backbone/resnetvd.py with
stem_type "deep", stem_width 32, avg_down True, bottleneck blocks, a frozen norm) from nn.Conv2d, the frozen affine,
F.avg_pool2d(2, 2, ceil_mode=True, count_include_pad=False) and F.max_pool2d(3, 2, 1), under the reference's key names.
tests/test_resnetvd_ref.py pins it to the reference's own class; the GPU tests compare the HIP modules with it.

`quant` (default: identity) is applied where the HIP path stores bf16: the folded weight image and every map."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn


def bf(t):
    return t.to(torch.bfloat16).float()


def quant_bf16(t):
    """bf16 storage with a straight-through gradient"""
    return t + (bf(t) - t).detach()


class FrozenNorm(nn.Module):
    def __init__(self, c, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.register_buffer("weight", torch.ones(c))
        self.register_buffer("bias", torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c) - eps)

    def affine(self):
        scale = self.weight * (self.running_var + self.eps).rsqrt()
        return scale, self.bias - self.running_mean * scale

    def forward(self, x):
        scale, shift = self.affine()
        return x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)


class AvgPool(nn.Module):
    def forward(self, x):
        return F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False)


def conv_norm(conv, norm, x, q=None):
    """conv + frozen affine; with q: the folded form the HIP path computes, q(conv(x, q(W * scale)) + shift)"""
    if q is None:
        return norm(conv(x))
    scale, shift = norm.affine()
    return q(F.conv2d(x, q(conv.weight * scale.view(-1, 1, 1, 1)), shift, conv.stride, conv.padding))


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = FrozenNorm(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = FrozenNorm(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = FrozenNorm(planes * 4)
        self.downsample = downsample

    def forward(self, x, q=None):
        qq = q or (lambda t: t)
        o = qq(F.relu(conv_norm(self.conv1, self.bn1, x, q)))
        o = qq(F.relu(conv_norm(self.conv2, self.bn2, o, q)))
        o = conv_norm(self.conv3, self.bn3, o, q)
        sc = x
        if self.downsample is not None:
            sc = conv_norm(self.downsample[1], self.downsample[2], qq(self.downsample[0](x)), q)
        return qq(F.relu(o + sc))


def downsample_avg(cin, cout, stride):
    return nn.Sequential(AvgPool() if stride != 1 else nn.Identity(), nn.Conv2d(cin, cout, 1, bias=False), FrozenNorm(cout))


class ResNetVDRef(nn.Module):
    def __init__(self, layers=(3, 4, 6, 3), stem_width=32, zero_init_last_bn=True):
        super().__init__()
        inplanes = 2 * stem_width
        self.conv1 = nn.Sequential(
            nn.Conv2d(3, stem_width, 3, stride=2, padding=1, bias=False), FrozenNorm(stem_width), nn.ReLU(),
            nn.Conv2d(stem_width, stem_width, 3, padding=1, bias=False), FrozenNorm(stem_width), nn.ReLU(),
            nn.Conv2d(stem_width, inplanes, 3, padding=1, bias=False))
        self.bn1 = FrozenNorm(inplanes)
        for i, (planes, nb) in enumerate(zip((64, 128, 256, 512), layers)):
            stride = 1 if i == 0 else 2
            blocks = []
            for k in range(nb):
                down = downsample_avg(inplanes, planes * 4, stride) if k == 0 and (stride != 1 or inplanes != planes * 4) else None
                blocks.append(Bottleneck(inplanes, planes, stride if k == 0 else 1, down))
                inplanes = planes * 4
            self.add_module(f"layer{i + 1}", nn.Sequential(*blocks))
        if zero_init_last_bn:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.zeros_(m.bn3.weight)

    def stem(self, x, q=None):
        qq = q or (lambda t: t)
        c = self.conv1
        x = qq(x)
        x = qq(F.relu(conv_norm(c[0], c[1], x, q)))
        x = qq(F.relu(conv_norm(c[3], c[4], x, q)))
        x = qq(F.relu(conv_norm(c[6], self.bn1, x, q)))
        return F.max_pool2d(x, 3, 2, 1)

    def forward(self, x, q=None):
        x = self.stem(x, q)
        outs = {}
        for i in range(4):
            for blk in getattr(self, f"layer{i + 1}"):
                x = blk(x, q)
            if i:
                outs[f"res{i + 2}"] = x
        return outs


def random_state(shapes, seed):
    """weights and norm buffers for a {key: shape} table, drawn from numpy.random.RandomState(seed) in sorted key order:
    convolutions N(0, 2 / fan_in) (ReLU-preserving), norm buffers near the identity (scales near 1) so that activations stay
    alive through 16 blocks"""
    rs = np.random.RandomState(seed)
    sd = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        if len(shp) == 4:
            v = rs.standard_normal(shp) * (2.0 / (shp[1] * shp[2] * shp[3])) ** 0.5
        elif k.endswith("running_var") or k.endswith(".weight"):
            v = rs.uniform(0.9, 1.1, shp)
        else:
            v = rs.standard_normal(shp) * 0.05
        sd[k] = torch.from_numpy(np.asarray(v, np.float32))
    return sd


# tests/golden/resnetvd.npz (tools/gen_resnetvd_golden.py): the gradients recorded for the depth-50 net; the three large
# ones are stored as every STEP-th element of the flattened tensor (a prime step: no alignment with the tensor's axes)
GOLDEN_GRADS = {"conv1.0.weight": 1, "conv1.6.weight": 1, "layer2.0.downsample.1.weight": 7, "layer4.0.conv2.weight": 131,
                "layer4.2.conv3.weight": 61}
GOLDEN_SEED, GOLDEN_LAYERS = 50, (3, 4, 6, 3)


def golden_cotangents(shapes):
    """the fixed random cotangents of the golden's loss sum(out * cotangent): bf16-exact values, regenerated (not stored)"""
    rs = np.random.RandomState(2)
    return {k: bf(torch.from_numpy(rs.standard_normal(tuple(shapes[k])).astype(np.float32))) for k in ("res3", "res4", "res5")}


# ---------------------------------------------------------------------------------------------- the reference's own class
class TimmBottleneck(nn.Module):
    """timm.models.resnet.Bottleneck (timm is not installed) restated from the reference's own DeformableBottleneck
    (resnetvd.py:23-117): the same layout without the offset branch, conv2 an ordinary 3x3 convolution"""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, cardinality=1, base_width=64, reduce_first=1, dilation=1,
                 first_dilation=None, act_layer=nn.ReLU, norm_layer=nn.BatchNorm2d, attn_layer=None, aa_layer=None,
                 drop_block=None, drop_path=None):
        super().__init__()
        import math
        width = int(math.floor(planes * (base_width / 64)) * cardinality)
        first_planes = width // reduce_first
        outplanes = planes * self.expansion
        first_dilation = first_dilation or dilation
        self.conv1 = nn.Conv2d(inplanes, first_planes, kernel_size=1, bias=False)
        self.bn1 = norm_layer(first_planes)
        self.act1 = act_layer(inplace=True)
        self.conv2 = nn.Conv2d(first_planes, width, kernel_size=3, stride=stride, padding=first_dilation, dilation=first_dilation,
                               groups=cardinality, bias=False)
        self.bn2 = norm_layer(width)
        self.act2 = act_layer(inplace=True)
        self.conv3 = nn.Conv2d(width, outplanes, kernel_size=1, bias=False)
        self.bn3 = norm_layer(outplanes)
        self.act3 = act_layer(inplace=True)
        self.downsample = downsample
        self.stride = stride
        self.dilation = dilation

    def zero_init_last_bn(self):
        nn.init.zeros_(self.bn3.weight)

    def forward(self, x):
        shortcut = x
        x = self.act1(self.bn1(self.conv1(x)))
        x = self.act2(self.bn2(self.conv2(x)))
        x = self.bn3(self.conv3(x))
        if self.downsample is not None:
            shortcut = self.downsample(shortcut)
        x += shortcut
        return self.act3(x)


def load_reference():
    """the reference's resnetvd.py loaded by path, the way oracle/ref_loader.py loads files; the names it imports from
    detectron2 and timm (neither installed) are stubbed, timm's Bottleneck by the restatement above"""
    import importlib
    import sys
    import types
    import ref_loader
    ref_loader.load()                      # detectron2 stubs + the yolov7 namespace packages
    d2l = sys.modules["detectron2.layers"]
    for name, val in (("FrozenBatchNorm2d", FrozenNorm), ("NaiveSyncBatchNorm", nn.BatchNorm2d), ("DeformConv", nn.Conv2d)):
        if not hasattr(d2l, name):
            setattr(d2l, name, val)

    def stub(name, **attrs):
        m = sys.modules.get(name)
        if m is None:
            m = sys.modules[name] = types.ModuleType(name)
            m.__path__ = []
        for k, v in attrs.items():
            if not hasattr(m, k):
                setattr(m, k, v)
        return m
    stub("timm")
    stub("timm.models")
    stub("timm.models.resnet", BasicBlock=type("BasicBlock", (nn.Module,), {"expansion": 1}), Bottleneck=TimmBottleneck)
    stub("timm.models.layers", DropBlock2d=nn.Identity, DropPath=nn.Identity, AvgPool2dSame=nn.AvgPool2d)
    return importlib.import_module("yolov7.modeling.backbone.resnetvd")


def build_reference(layers):
    """the reference's own ResNet as its builder constructs it (resnetvd.py:542-549), for any `layers`"""
    return load_reference().ResNet(["bottleneck"] * 4, list(layers), stem_type="deep", stem_width=32, avg_down=True, norm_layer=FrozenNorm)
