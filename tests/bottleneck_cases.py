"""The bottleneck blocks whose outputs tests/golden/bottleneck_parent_record.npz holds, as they were computed by the commit
before the d2 and the vd block came to share one autograd node: shared by tests/test_gpu_bottleneck_record.py and
tools/record_bottleneck_outputs.py, so that both build identical tensors.

Every case: N = 2, the smallest channel counts the blocks accept (32 / 64, bottleneck width 32), input_is_relu set, the
input a ReLU output (half of it zero), frozen-norm buffers drawn away from the identity, everything from one CPU generator.
The d2 odd map (11 x 19) exercises the strided shortcut's accumulate over the even pixels only, the vd odd map ceil-mode
pooling.  The two stacks - [projection block, identity block] through ONE backward - are where the identity block's masked
input gradient (_premask_note) meets the _premask_take of the block before it."""
import hashlib
import os

import numpy as np
import torch
from torch import nn

from yolov7_d2_amd.modeling import resnet as R
from yolov7_d2_amd.modeling import resnet_vd as RV

DEV = "cuda"
RECORD = "bottleneck_parent_record.npz"
N, BC = 2, 32
# name -> (family, [(cin, cout, stride) per block], H, W)
CASES = {
    "d2_identity": ("d2", [(64, 64, 1)], 11, 19),
    "d2_shortcut_s1": ("d2", [(32, 64, 1)], 11, 19),
    "d2_shortcut_s2": ("d2", [(32, 64, 2)], 11, 19),
    "vd_identity": ("vd", [(64, 64, 1)], 12, 20),
    "vd_proj_s1": ("vd", [(32, 64, 1)], 12, 20),
    "vd_pooled_s2": ("vd", [(32, 64, 2)], 11, 19),
    "d2_stack": ("d2", [(32, 64, 2), (64, 64, 1)], 11, 19),
    "vd_stack": ("vd", [(32, 64, 2), (64, 64, 1)], 11, 19),
}
GROUPED = ("1", "0")        # MI_WGRAD_LAYER_GROUP: the block's weight gradients as one grouped launch / one launch each


class _VD(RV.BottleneckVD):
    expansion = 2           # 32 -> 64: the smallest output width (the reference's blocks have 4)


def _block(family, cin, cout, stride):
    if family == "d2":
        return R.BottleneckBlock(cin, cout, BC, stride=stride)
    assert cout == BC * _VD.expansion
    return _VD(cin, BC, stride, RV._downsample_avg(cin, cout, stride) if (stride != 1 or cin != cout) else None)


def build(name):
    """(nn.Sequential of the case's blocks on the device, x, gy): every value drawn from a CPU generator seeded by the name"""
    family, blocks, H, W = CASES[name]
    g = torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"))
    net = nn.Sequential(*[_block(family, *b) for b in blocks])
    with torch.no_grad():
        for blk in net:
            blk.input_is_relu = True
        for k, p in net.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
        for k, b in net.named_buffers():
            if k.endswith(("running_var", ".weight")):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
            else:
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
    cl = lambda t: t.to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last)
    x = cl(torch.randn(N, blocks[0][0], H, W, generator=g).clamp(min=0))
    s = blocks[0][2]
    gy = cl(torch.randn(N, blocks[-1][1], (H - 1) // s + 1, (W - 1) // s + 1, generator=g))
    return net.to(DEV), x, gy


def _raw(t):
    """the tensor's bits on the host: bf16 as int16, fp32 as int32, NCHW order"""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def run(name, grouped):
    """forward + one backward of the case under the default switches and MI_WGRAD_LAYER_GROUP=grouped:
    {"out", "dx", "gw_<parameter name>"...: raw bits}"""
    prev = os.environ.get("MI_WGRAD_LAYER_GROUP")
    os.environ["MI_WGRAD_LAYER_GROUP"] = grouped
    try:
        net, x, gy = build(name)
        xi = x.clone().requires_grad_(True)
        out = net(xi)
        out.backward(gy)
        torch.cuda.synchronize()
    finally:
        if prev is None:
            del os.environ["MI_WGRAD_LAYER_GROUP"]
        else:
            os.environ["MI_WGRAD_LAYER_GROUP"] = prev
    res = {"out": _raw(out), "dx": _raw(xi.grad)}
    for k, p in net.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        res["gw_" + k] = _raw(p.grad)
    return res


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def record_of(name, grouped, res):
    """what the record keeps of one run: every tensor's SHA-256, and under the default (grouped) setting the tensors
    themselves - the file stays under the size a committed file may have, and a difference can still be located"""
    rec = {f"{name}/g{grouped}/sha256/{k}": digest(v) for k, v in res.items()}
    if grouped == "1":
        rec.update({f"{name}/g{grouped}/bits/{k}": v for k, v in res.items()})
    return rec
