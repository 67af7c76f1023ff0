"""GPU (-m gpu): the ResNet-vd backbone (modeling/resnet_vd.py, csrc/resnetvd_ops.hip) - the shortcut's average pool bit
for bit against torch, BottleneckVD and the deep stem against the fp32 restatement tests/resnetvd_ref.py (pinned to the
reference's own class by tests/test_resnetvd_ref.py), the depth-50 network against tests/golden/resnetvd.npz (the
reference's outputs and gradients), and SparseInst on this backbone, eager and captured."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnetvd_ref as V
import yolov7_d2_amd as M
from yolov7_d2_amd import _lib as L
from yolov7_d2_amd.modeling import resnet_vd as RV

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ pool kernels
# (N, H, W, C, channels of the tensor the input / the gradient destination is a slice of, first channel of the slice)
POOL_SHAPES = [(2, 8, 12, 64, 64, 0), (2, 7, 9, 64, 96, 16), (1, 1, 1, 8, 8, 0), (1, 5, 2, 72, 72, 0)]


def _grid(shape, gen):
    """bf16 values k / 64, |k| <= 256: every fp32 sum of up to five of them (and of quarters of them) is exact"""
    return (torch.randint(-256, 257, shape, generator=gen).float() / 64).to(torch.bfloat16)


def _pool_ref(x):            # x: fp32 NHWC -> fp32 NHWC
    return F.avg_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1)


@pytest.mark.parametrize("N,H,W,C,Cw,c0", POOL_SHAPES)
def test_avgpool_forward_equals_torch_bit_for_bit(N, H, W, C, Cw, c0):
    gen = torch.Generator().manual_seed(H * 100 + W)
    wide = _grid((N, H, W, Cw), gen).to(DEV)
    x = wide[..., c0: c0 + C]                       # ldx = Cw > C for the sliced case
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    ywide = torch.full((N, Ho, Wo, Cw), 7.0, dtype=torch.bfloat16, device=DEV)
    L.check(L.lib().mi_avgpool2x2s2_fwd(x.data_ptr(), Cw, ywide[..., c0:].data_ptr(), Cw, N, H, W, C, L.stream_ptr()), "fwd")
    ref = _pool_ref(x.float().cpu()).to(torch.bfloat16)
    assert torch.equal(_bits(ywide[..., c0: c0 + C].cpu()), _bits(ref))
    keep = torch.ones(Cw, dtype=torch.bool)
    keep[c0: c0 + C] = False
    assert bool((ywide.cpu()[..., keep] == 7.0).all())          # nothing outside the [N, Ho, Wo, C] region is written
    assert torch.equal(_bits(RV.avgpool2x2(x).cpu()), _bits(ref))   # the module's wrapper (dense output) on the same view


@pytest.mark.parametrize("form", ["plain", "accumulate", "accumulate_mask"])
@pytest.mark.parametrize("N,H,W,C,Cw,c0", POOL_SHAPES)
def test_avgpool_backward_equals_torch_bit_for_bit(N, H, W, C, Cw, c0, form):
    gen = torch.Generator().manual_seed(H * 100 + W + 7)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    dy = _grid((N, Ho, Wo, C), gen)
    pre = _grid((N, H, W, Cw), gen)                  # what the destination holds before the pass
    mask = _grid((N, H, W, C), gen)
    mask[torch.rand(mask.shape, generator=gen) < 0.3] = 0       # zeros, negatives and positives
    assert bool((mask == 0).any()) or mask.numel() <= 8
    xr = torch.zeros(N, H, W, C, requires_grad=True)
    _pool_ref(xr).backward(dy.float())
    want = xr.grad.clone()                           # dy[iy / 2][ix / 2] / count, exact in fp32
    if form != "plain":
        want = want + pre[..., c0: c0 + C].float()
    want = want.to(torch.bfloat16)                   # the one rounding
    if form == "accumulate_mask":
        want = torch.where(mask.float() > 0, want, torch.zeros_like(want))
    dxw = pre.clone().to(DEV)
    dyd, md = dy.to(DEV), mask.to(DEV)
    L.check(L.lib().mi_avgpool2x2s2_bwd(dyd.data_ptr(), C, dxw[..., c0:].data_ptr(), Cw, md.data_ptr() if form == "accumulate_mask" else None,
                                        C, 0 if form == "plain" else 1, N, H, W, C, L.stream_ptr()), "bwd")
    got = dxw.cpu()
    assert torch.equal(_bits(got[..., c0: c0 + C]), _bits(want))
    keep = torch.ones(Cw, dtype=torch.bool)
    keep[c0: c0 + C] = False
    assert torch.equal(_bits(got[..., keep]), _bits(pre[..., keep]))     # outside the [N, H, W, C] region: untouched
    if form == "accumulate_mask":                    # = the unmasked pass followed by mi_ew_bf16 op 2
        d2 = pre[..., c0: c0 + C].contiguous().to(DEV)
        L.check(L.lib().mi_avgpool2x2s2_bwd(dyd.data_ptr(), C, d2.data_ptr(), C, None, 0, 1, N, H, W, C, L.stream_ptr()), "bwd")
        out = torch.empty_like(d2)
        L.check(L.lib().mi_ew_bf16(d2.data_ptr(), md.data_ptr(), out.data_ptr(), d2.numel(), 2, L.stream_ptr()), "relu'")
        assert torch.equal(_bits(out.cpu()), _bits(got[..., c0: c0 + C]))


# ------------------------------------------------------------------------------------------------ BottleneckVD
BLOCK_CASES = [(64, 256, 64, 1, 14, 18), (256, 512, 128, 2, 14, 18), (256, 512, 128, 2, 15, 17), (512, 512, 128, 1, 8, 8)]
BLOCK_IDS = ["proj_s1", "pool_even", "pool_odd", "identity"]


def _block_pair(cin, cout, bc, stride, seed=5):
    """(HIP block on the device, fp32 restatement) with the same random weights and norm buffers"""
    proj = stride != 1 or cin != cout
    ref = V.Bottleneck(cin, bc, stride, V.downsample_avg(cin, cout, stride) if proj else None)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in ref.state_dict().items():
        if v.dim() == 4:
            sd[k] = V.bf(torch.randn(v.shape, generator=g) * (2.0 / (v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5)
        elif k.endswith(("running_var", ".weight")):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
    ref.load_state_dict(sd)
    blk = RV.BottleneckVD(cin, bc, stride, RV._downsample_avg(cin, cout, stride) if proj else None)
    blk.load_state_dict(sd)
    return blk.to(DEV), ref, g


@pytest.mark.parametrize("cin,cout,bc,stride,H,W", BLOCK_CASES, ids=BLOCK_IDS)
def test_bottleneck_vd_fwd_bwd(cin, cout, bc, stride, H, W):
    """output, input gradient and the three or four weight gradients against fp32 torch with bf16-rounded storage - the
    bounds of test_gpu_resnet.py::test_bottleneck_block_fwd_bwd (the d2 block on the same kernels)"""
    blk, ref, g = _block_pair(cin, cout, bc, stride)
    x = V.bf(torch.randn(2, cin, H, W, generator=g))
    xr = x.clone().requires_grad_(True)
    want = ref(xr, V.quant_bf16)
    go = V.bf(torch.randn(want.shape, generator=g))
    want.backward(go)
    xd = x.to(DEV).to(torch.bfloat16).requires_grad_(True)
    out = blk(xd)
    assert out.shape == want.shape
    e = {"out": _rel(out, want)}
    out.backward(go.to(DEV).to(out.dtype))
    e["dx"] = _rel(xd.grad, xr.grad)
    rp = dict(ref.named_parameters())
    for n, p in blk.named_parameters():
        e[n] = _rel(p.grad, rp[n].grad)
    print("BottleneckVD", (cin, cout, bc, stride, H, W), {k: round(v, 5) for k, v in e.items()})
    assert len(e) == (6 if blk.downsample is not None else 5)
    assert e["out"] < 1e-2, e
    assert max(v for k, v in e.items() if k != "out") < 3e-2, e


@pytest.mark.parametrize("cin,cout,bc,stride,H,W", BLOCK_CASES, ids=BLOCK_IDS)
def test_bottleneck_vd_as_one_node_equals_the_per_module_composition(cin, cout, bc, stride, H, W, monkeypatch):
    """resnet._BottleneckFn (the node the vd block shares with the d2 block) against conv-by-conv autograd nodes (+ the
    pool's own node and autograd's additions): same kernels and roundings -> identical output and weight
    gradients, the input gradient within the 4e-3 of the d2 block's test"""
    monkeypatch.setenv("MI_WGRAD_LAYER_GROUP", "0")     # one launch per weight gradient on both sides
    monkeypatch.setenv("MI_RESNET_EPI_FUSE", "0")       # (the node structure is under test)
    blk, _, g = _block_pair(cin, cout, bc, stride)
    x = torch.randn(2, cin, H, W, generator=g).to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    go = torch.randn(2, cout, Ho, Wo, generator=g).to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last)
    res = []
    for flag in ("1", "0"):
        monkeypatch.setenv("MI_RESNET_BLOCK_FN", flag)
        blk.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        out = blk(xi)
        assert (type(out.grad_fn).__name__ == "_BottleneckFnBackward") == (flag == "1")
        out.backward(go)
        res.append([out.detach().float(), xi.grad.float()] + [p.grad.float().clone() for p in blk.parameters()])
    for i, (a, b) in enumerate(zip(*res)):
        if i == 1:
            assert _rel(a, b) < 4e-3
        else:
            assert torch.equal(a, b), (i, float((a - b).abs().max()))


@pytest.mark.parametrize("cin,cout,bc,stride,H,W", BLOCK_CASES, ids=BLOCK_IDS)
def test_bottleneck_vd_mask_fused_backward_equals_unfused_then_relu_mask(cin, cout, bc, stride, H, W, monkeypatch):
    """input_is_relu: the block input's ReLU mask taken in the last pass over its gradient (the pool's backward for the
    stride-2 blocks) == the unfused backward followed by mi_ew_bf16 op 2, bit for bit"""
    blk, _, g = _block_pair(cin, cout, bc, stride)
    blk.input_is_relu = True
    x = torch.relu(torch.randn(2, cin, H, W, generator=g)).to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    go = torch.randn(2, cout, Ho, Wo, generator=g).to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last)
    dxs = []
    for fuse in ("1", "0"):
        monkeypatch.setenv("MI_RESNET_MASK_FUSE", fuse)
        xi = x.clone().requires_grad_(True)
        blk(xi).backward(go)
        dxs.append(xi.grad.permute(0, 2, 3, 1).contiguous())
    xh = x.permute(0, 2, 3, 1).contiguous()
    masked = torch.empty_like(dxs[1])
    L.check(L.lib().mi_ew_bf16(dxs[1].data_ptr(), xh.data_ptr(), masked.data_ptr(), masked.numel(), 2, L.stream_ptr()), "relu'")
    assert float((xh == 0).float().mean()) > 0.3 and not torch.equal(_bits(dxs[1].cpu()), _bits(masked.cpu()))   # the mask bites
    assert torch.equal(_bits(dxs[0].cpu()), _bits(masked.cpu()))


# ------------------------------------------------------------------------------------------------ deep stem
def test_stem_scattered_taps_reproduce_the_shifted_input():
    """a 3x3 weight with a single 1 at (r, s): the stride-2 convolution is the image sampled at (2 oy - 1 + r, 2 ox - 1 + s)"""
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 128, (2, 3, 12, 20), generator=g).float()          # bf16-exact, non-negative (ReLU epilogue)
    s2d = torch.empty(2, 6, 10, 16, dtype=torch.bfloat16, device=DEV)
    xd = img.to(DEV).contiguous()
    L.check(L.lib().mi_focus_pack(xd.data_ptr(), 2, 12, 20, s2d.data_ptr(), 16, L.stream_ptr()), "mi_focus_pack")
    zero = torch.zeros(32, device=DEV)
    for r in range(3):
        for s in range(3):
            w = torch.zeros(32, 3, 3, 3)
            for c in range(3):
                w[c, c, r, s] = 1
            out = RV._stem_conv(s2d, RV._pack_stem(w.to(DEV)), zero, 32).float().cpu()
            pad = F.pad(img, (1, 1, 1, 1))
            want = pad[:, :, r: r + 12: 2, s: s + 20: 2].permute(0, 2, 3, 1)
            assert torch.equal(out[..., :3], want), (r, s)
            assert float(out[..., 3:].abs().max()) == 0


@pytest.mark.parametrize("H,W", [(32, 48), (31, 45)])
def test_deep_stem_forward_and_weight_gradients(H, W):
    """three 3x3 convolutions (the first as 2x2 taps over the space-to-depth image) with their frozen affines + ReLU in the
    epilogues + MaxPool(3, 2, 1), and the three weight gradients (the first in the 9-tap form mapped back to 3x3), against
    the restatement on bf16-rounded storage; the terms of test_trainable_stem_forward_and_weight_gradient_match_torch"""
    ref = V.ResNetVDRef((1, 1, 1, 1))
    shapes = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    sd = V.random_state(shapes, seed=H)
    g = torch.Generator().manual_seed(H)
    for k in sd:                                   # norm buffers well away from the identity: the fold is under test
        if sd[k].dim() == 1:
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g) if k.endswith(("running_var", ".weight")) else 0.1 * torch.randn(sd[k].shape, generator=g)
    ref.load_state_dict(sd)
    net = RV.ResNetVD((1, 1, 1, 1))
    net.load_state_dict(sd)
    net.to(DEV).train()
    x = torch.randn(2, 3, H, W, generator=g)
    out = net.stem(x.to(DEV))
    want = ref.stem(x, V.quant_bf16)
    assert tuple(out.shape) == tuple(want.shape) == (2, 64, ((H + 1) // 2 + 1) // 2, ((W + 1) // 2 + 1) // 2)
    go = V.bf(torch.randn(want.shape, generator=g))
    want.backward(go)
    out.backward(go.to(DEV).to(out.dtype))
    e = _rel(out, want)
    print("deep stem", (H, W), "forward rel", round(e, 5))
    assert e < 1e-2
    for name, mine, theirs in (("conv1.0", net.conv1[0], ref.conv1[0]), ("conv1.3", net.conv1[3], ref.conv1[3]),
                               ("conv1.6", net.conv1[6], ref.conv1[6])):
        ga, gb = mine.weight.grad.float().cpu(), theirs.weight.grad
        cos = float((ga * gb).sum() / (ga.norm() * gb.norm()))
        ratio = float(ga.norm() / gb.norm())
        print("deep stem", (H, W), name, "cos", round(cos, 5), "norm ratio", round(ratio, 5))
        assert cos > 0.995 and abs(ratio - 1.0) < 0.01, (name, cos, ratio)


# ------------------------------------------------------------------------------------------------ whole backbone
def test_resnet50_vd_against_the_reference_golden(golden_dir):
    """depth 50 on the golden's 64 x 96 image: the reference's fp32 outputs within test_resnet50_forward_and_gradients' per-map
    bound, its five recorded gradients within that test's bounds for its own net (last block < 0.25, all < 0.7: the bf16
    noise floor of a 16-block network - the restatement's own bf16 emulation sits at 0.057 / 0.36 on this golden).
    Measured on the MI355X: outputs 8.1e-3 / 7.8e-3 / 7.7e-3; gradients conv1.0 0.355, conv1.6 0.245, layer2.0.downsample.1 0.250,
    layer4.0.conv2 0.153, layer4.2.conv3 0.059"""
    z = np.load(os.path.join(golden_dir, "resnetvd.npz"))
    net = RV.ResNetVD(V.GOLDEN_LAYERS)
    net.load_state_dict(V.random_state({k: tuple(v.shape) for k, v in net.state_dict().items()}, V.GOLDEN_SEED))
    net.to(DEV).train()
    out = net(torch.from_numpy(z["image"]).to(DEV))
    assert list(out) == ["res3", "res4", "res5"]
    cot = V.golden_cotangents({k: tuple(v.shape) for k, v in out.items()})
    for k in out:
        e = _rel(out[k], torch.from_numpy(z["out/" + k]))
        print("resnet50-vd", k, tuple(out[k].shape), "rel", round(e, 5))
        assert e < 3e-2, (k, e)
    sum((out[k].float() * cot[k].to(DEV)).sum() for k in out).backward()
    params = dict(net.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values())
    rels = {k: _rel(params[k].grad.flatten()[::step], torch.from_numpy(z["grad/" + k])) for k, step in V.GOLDEN_GRADS.items()}
    print("resnet50-vd weight-gradient rel L2:", {k: round(v, 4) for k, v in rels.items()})
    assert rels["layer4.2.conv3.weight"] < 0.25, rels
    assert max(rels.values()) < 0.7, rels


# ------------------------------------------------------------------------------------------------ SparseInst on ResNet-vd
def _si_inputs(seed, sizes, counts=None):
    """batched_inputs of the SparseInst meta-arch: uint8-valued images + bitmask instances (rectangles)"""
    from yolov7_d2_amd.d2shim import Instances
    gen = torch.Generator().manual_seed(seed)
    out = []
    for k, (h, w) in enumerate(sizes):
        n = counts[k] if counts is not None else int(torch.randint(1, 6, (1,), generator=gen))
        masks = torch.zeros(n, h, w)
        for j in range(n):
            y0, x0 = int(torch.randint(0, h - 40, (1,), generator=gen)), int(torch.randint(0, w - 40, (1,), generator=gen))
            hh, ww = int(torch.randint(24, min(96, h - y0), (1,), generator=gen)), int(torch.randint(24, min(96, w - x0), (1,), generator=gen))
            masks[j, y0: y0 + hh, x0: x0 + ww] = 1
        inst = Instances((h, w), gt_classes=torch.randint(0, 80, (n,), generator=gen), gt_masks=masks)
        out.append(dict(image=torch.randint(0, 256, (3, h, w), generator=gen).float(), instances=inst, height=h, width=w))
    return out


def _vd_model():
    torch.manual_seed(0)
    cfg = M.sparse_inst_r50_giam_cfg(device=DEV)
    cfg.MODEL.BACKBONE.NAME = "build_resnet_vd_backbone"
    model = M.build_model(cfg)
    with torch.no_grad():          # a fresh ResNet-vd has every bn3.weight zeroed: give the residual branches something to do
        for blk in (b for st in model.backbone.stage_modules() for b in st):
            blk.bn3.weight.fill_(0.5)
    return model.train()


def test_sparseinst_vd_eager_step_trains_every_backbone_parameter():
    model = _vd_model()
    losses = model(_si_inputs(1, ((192, 224), (160, 200))))
    assert losses and all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
    sum(losses.values()).backward()
    missing = [n for n, p in model.backbone.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing and len(list(model.backbone.parameters())) == 3 + 16 * 3 + 4
    assert all(float(p.grad.abs().max()) > 0 for p in model.backbone.parameters())


def test_sparseinst_vd_captured_step_equals_eager_across_two_shapes():
    """GraphedTrainStep on the vd backbone, the shapes and the tolerance of
    test_sparseinst_device_half_never_reads_the_host_and_is_captured: capture at one padded shape, an eager forward, a
    capture at a second shape, then replays of both - every step's losses equal the eager model's (the frozen affines and
    the step's other constants must keep their addresses between captures: FrozenBatchNorm2d.affine)"""
    from yolov7_d2_amd.graph_step import GraphedTrainStep
    from yolov7_d2_amd.optim import MultiTensorAdamW
    eager = _vd_model()
    graphed = copy.deepcopy(eager)
    mk = lambda m: MultiTensorAdamW([p for p in m.parameters() if p.requires_grad], lr=5e-5, weight_decay=0.05)
    oe, og = mk(eager), mk(graphed)
    a1, a2 = _si_inputs(1, ((192, 224), (160, 200))), _si_inputs(3, ((170, 224), (192, 200)))
    b1, b2 = _si_inputs(2, ((128, 160), (120, 150)), counts=(3, 1)), _si_inputs(4, ((100, 160), (128, 140)), counts=(2, 0))
    assert eager.batch_key(a1) == eager.batch_key(a2) != eager.batch_key(b1) == eager.batch_key(b2)
    step = GraphedTrainStep(graphed, og)
    try:
        for it, b in enumerate((a1, b1, a2, b2)):
            if it == 1:
                with torch.no_grad():
                    graphed(a2)                       # an eager forward between the two captures
            losses = eager(b)
            oe.zero_grad(set_to_none=True)
            sum(losses.values()).backward()
            oe.step()
            out = step(b)
            assert len(step.graphs) == min(it + 1, 2)
            for k, v in losses.items():
                torch.testing.assert_close(out[k].float(), v.detach().float(), rtol=3e-3, atol=3e-3, msg=f"step {it} {k}")
        torch.cuda.synchronize()
    finally:
        step.close()
