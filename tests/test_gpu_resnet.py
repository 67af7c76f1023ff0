"""GPU (-m gpu): detectron2-shaped ResNet-50 (modeling/resnet.py) against the CPU restatement oracle/resnet_oracle.py -
7x7 stem as 4x4 over space-to-depth (even and odd image sizes), frozen norms folded into the conv, max-pool, all four
stages forward, and the gradients of the trainable stages (FREEZE_AT 2) with respect to weights and the res2 output."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_oracle as R
from yolov7_d2_amd.modeling.resnet import ResNet, _MaxPool

pytestmark = pytest.mark.gpu


def _bf(t):
    return t.to(torch.bfloat16).float()


def _rel(a, b):
    return float((a.detach().float().cpu() - b.detach().float().cpu()).norm() / (b.detach().float().cpu().norm() + 1e-12))


def test_maxpool_fwd_bwd_matches_torch():
    g = torch.Generator().manual_seed(1)
    for (N, C, H, W) in ((2, 64, 17, 22), (1, 32, 8, 8)):
        x = _bf(torch.randn(N, C, H, W, generator=g)).round(decimals=1)      # coarse values: ties exercise the first-max rule
        x = _bf(x)
        xr = x.clone().requires_grad_(True)
        ref = F.max_pool2d(xr, 3, 2, 1)
        go = _bf(torch.randn(ref.shape, generator=g))
        ref.backward(go)
        xd = x.permute(0, 2, 3, 1).contiguous().cuda().to(torch.bfloat16).requires_grad_(True)
        y = _MaxPool.apply(xd)
        assert torch.equal(y.float().cpu().permute(0, 3, 1, 2), ref.detach())
        y.backward(go.permute(0, 2, 3, 1).contiguous().cuda().to(torch.bfloat16))
        np.testing.assert_allclose(xd.grad.float().cpu().permute(0, 3, 1, 2).numpy(), _bf(xr.grad).numpy(), rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("H,W", [(64, 96), (75, 101)])
def test_resnet50_forward_and_gradients(H, W):
    sd = R.init_state_dict(50, seed=0)
    m = ResNet(50, ("res2", "res3", "res4", "res5"), freeze_at=2)
    m.load_state_dict(sd)
    m.cuda().train()
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(3))
    out = m(x.cuda())
    q = lambda t: t + (_bf(t) - t).detach()
    osd = {k: v.clone() for k, v in sd.items()}
    train_keys = [k for k in osd if k.endswith(".weight") and ".norm." not in k and k.startswith(("res3", "res4", "res5"))]
    for k in train_keys:
        osd[k].requires_grad_(True)
    ref = R.forward(osd, x, quant=q)
    for k in ("res2", "res3", "res4", "res5"):
        assert out[k].shape == ref[k].shape, (k, out[k].shape, ref[k].shape)
        e = _rel(out[k], ref[k])
        print(k, tuple(ref[k].shape), "rel", e)
        assert e < 3e-2, (k, e)
    go = _bf(torch.randn(ref["res5"].shape, generator=torch.Generator().manual_seed(4)))
    ref["res5"].backward(go)
    out["res5"].backward(go.cuda().to(out["res5"].dtype))
    assert m.stem.conv1.weight.grad is None and m.res2[0].conv1.weight.grad is None      # frozen
    rels = {k: _rel(dict(m.named_parameters())[k].grad, osd[k].grad) for k in train_keys}
    print("weight-gradient rel L2 by stage:", {st: round(max(v for k, v in rels.items() if k.startswith(st)), 3)
                                               for st in ("res3", "res4", "res5")})
    # bf16 storage noise flips ReLU gates and compounds through the 13 trainable blocks: the oracle's OWN two bf16
    # emulations of this network and input differ by 0.14-0.16 (res5.2), 0.35-0.48 (res4), 0.46-0.52 (res3) in these
    # weight gradients (measured on the CPU).  The whole-network check is therefore a noise-floor bound; the per-block
    # test below is the tight check of every backward kernel path (1x1 / 3x3 stride 1 / 2, shortcut, add + ReLU).
    assert max(v for k, v in rels.items() if k.startswith("res5.2")) < 0.25
    assert max(rels.values()) < 0.7


def test_resnet50_gradients_with_the_forward_state_pinned(monkeypatch):
    """the tight whole-network check (what tests/test_gpu_parity_bench.py does for YOLOX): every conv output of the
    trainable stages (res3 .. res5, FREEZE_AT 2) that the HIP network produced is forced into the oracle's forward
    (teacher forcing: same ReLU gates, same operands), then the oracle's autograd from the same output gradient must give
    the HIP weight gradients - cosine >= 0.999 and relative L2 <= 0.05 on every one of the 42 trainable conv weights.  The
    un-forced comparison above can only bound the bf16 noise floor (< 0.7)."""
    from yolov7_d2_amd.modeling.resnet import Conv2d
    # the per-convolution modules are hooked for their outputs: run the blocks as per-convolution autograd nodes (the
    # one-node form is tied to this one by test_bottleneck_as_one_node_equals_per_convolution_nodes)
    monkeypatch.setenv("MI_RESNET_BLOCK_FN", "0")
    sd = R.init_state_dict(50, seed=0)
    m = ResNet(50, ("res2", "res3", "res4", "res5"), freeze_at=2)
    m.load_state_dict(sd)
    m.cuda().train()
    caps = {}
    for name, mod in m.named_modules():
        if isinstance(mod, Conv2d) and name.startswith(("res3", "res4", "res5")):
            mod.register_forward_hook(lambda mod, inp, out, name=name: caps.__setitem__(name, out.detach().float().cpu()))
    x = torch.randn(2, 3, 96, 128, generator=torch.Generator().manual_seed(3))
    out = m(x.cuda())
    q = lambda t: t + (_bf(t) - t).detach()
    osd = {k: v.clone() for k, v in sd.items()}
    train_keys = [k for k in osd if k.endswith(".weight") and ".norm." not in k and k.startswith(("res3", "res4", "res5"))]
    assert len(train_keys) == 42 and len(caps) == 42     # 13 blocks x 3 convs + 3 shortcuts
    for k in train_keys:
        osd[k].requires_grad_(True)
    ref = R.forward(osd, None, quant=q, force=caps, start=("res3", out["res2"].detach().float().cpu()))
    for k in ("res3", "res4", "res5"):
        assert _rel(out[k], ref[k]) < 1e-3, (k, _rel(out[k], ref[k]))     # forced: only the last add + ReLU differs in rounding
    go = _bf(torch.randn(ref["res5"].shape, generator=torch.Generator().manual_seed(4)))
    ref["res5"].backward(go)
    out["res5"].backward(go.cuda().to(out["res5"].dtype))
    bad = []
    for k in train_keys:
        a, b = dict(m.named_parameters())[k].grad.float().cpu().flatten(), osd[k].grad.flatten()
        cos = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))
        rel = float((a - b).norm() / (b.norm() + 1e-30))
        if cos < 0.999 or rel > 0.05:
            bad.append((k, round(cos, 5), round(rel, 4)))
    assert not bad, bad[:8]


@pytest.mark.parametrize("cin,cout,bc,stride", [(256, 512, 128, 2), (512, 512, 128, 1)], ids=["shortcut_s2", "identity"])
def test_bottleneck_block_fwd_bwd(cin, cout, bc, stride):
    """one BottleneckBlock (1x1 -> 3x3 (stride) -> 1x1, frozen norms folded, 1x1 stride-2 shortcut, add + ReLU): output,
    input gradient and the four weight gradients against fp32 torch with bf16-rounded storage"""
    from yolov7_d2_amd.modeling.resnet import BottleneckBlock
    g = torch.Generator().manual_seed(5)
    blk = BottleneckBlock(cin, cout, bc, stride=stride)
    sd = {}
    for n, mod in (("shortcut", blk.shortcut), ("conv1", blk.conv1), ("conv2", blk.conv2), ("conv3", blk.conv3)):
        if mod is None:
            continue
        co, ci, k, _ = mod.weight.shape
        sd[n + ".weight"] = _bf(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
        sd[n + ".norm.weight"] = 0.5 + torch.rand(co, generator=g)
        sd[n + ".norm.bias"] = torch.randn(co, generator=g) * 0.1
        sd[n + ".norm.running_mean"] = torch.randn(co, generator=g) * 0.1
        sd[n + ".norm.running_var"] = 0.5 + torch.rand(co, generator=g)
    blk.load_state_dict(sd)
    blk.cuda()
    x = _bf(torch.randn(2, cin, 20, 26, generator=g))
    q = lambda t: t + (_bf(t) - t).detach()
    osd = {k: v.clone().requires_grad_(k.endswith(".weight") and ".norm." not in k) for k, v in sd.items()}

    def cn(p, t, s_, pad):
        scale = osd[p + ".norm.weight"] * (osd[p + ".norm.running_var"] + 1e-5).rsqrt()
        shift = osd[p + ".norm.bias"] - osd[p + ".norm.running_mean"] * scale
        return q(F.conv2d(t, q(osd[p + ".weight"] * scale.view(-1, 1, 1, 1)), shift, s_, pad))
    xr = x.clone().requires_grad_(True)
    o = q(F.relu(cn("conv1", xr, 1, 0)))
    o = q(F.relu(cn("conv2", o, stride, 1)))
    o = cn("conv3", o, 1, 0)
    sc = cn("shortcut", xr, stride, 0) if blk.shortcut is not None else xr
    ref = q(F.relu(o + sc))
    go = _bf(torch.randn(ref.shape, generator=g))
    ref.backward(go)
    xd = x.cuda().to(torch.bfloat16).requires_grad_(True)
    out = blk(xd)
    assert _rel(out, ref) < 1e-2
    out.backward(go.cuda().to(out.dtype))
    assert _rel(xd.grad, xr.grad) < 3e-2
    for n, p in blk.named_parameters():
        assert _rel(p.grad, osd[n].grad) < 3e-2, (n, _rel(p.grad, osd[n].grad))


@pytest.mark.parametrize("H,W", [(64, 96), (75, 101)])
def test_trainable_stem_forward_and_weight_gradient_match_torch(H, W):
    """BasicStem with FREEZE_AT 0 (SparseInst: configs/coco/sparseinst/Base-SparseInst.yaml): 7x7 stride-2 conv (as a 4x4
    conv over the space-to-depth image) + frozen affine + ReLU + MaxPool(3, 2, 1) with recorded first-maximum positions,
    and its backward - max-pool routing, ReLU mask, the 16-tap weight gradient mapped back to 7x7 - against torch fp32 on
    the same bf16-rounded operands"""
    from yolov7_d2_amd.modeling.resnet import BasicStem
    g = torch.Generator().manual_seed(H)
    torch.manual_seed(H)                 # (the stem's weights come from the global generator: the case must not depend on test order)
    stem = BasicStem(3, 64).cuda()
    with torch.no_grad():
        stem.conv1.norm.weight.copy_(0.5 + torch.rand(64, generator=g))
        stem.conv1.norm.bias.copy_(0.1 * torch.randn(64, generator=g))
        stem.conv1.norm.running_mean.copy_(0.1 * torch.randn(64, generator=g))
        stem.conv1.norm.running_var.copy_(0.5 + torch.rand(64, generator=g))
    x = torch.randn(2, 3, H, W, generator=g)
    out = stem(x.cuda())
    go = _bf(torch.randn(out.shape, generator=g))
    out.backward(go.cuda().to(out.dtype))
    scale, shift = (t.detach().float().cpu() for t in stem.conv1.norm.affine())
    w = stem.conv1.weight.detach().float().cpu().clone().requires_grad_(True)
    ref = F.max_pool2d(F.relu(F.conv2d(_bf(x), w * scale.view(-1, 1, 1, 1), shift, stride=2, padding=3)), 3, 2, 1)
    ref.backward(go)
    assert _rel(out, ref) < 1e-2
    ga, gb = stem.conv1.weight.grad.float().cpu(), w.grad
    # bf16 weights / activations on our side only (ReLU decisions of near-zero pre-activations may differ): measured cos 0.997
    cos = float((ga * gb).sum() / (ga.norm() * gb.norm()))
    assert cos > 0.995 and abs(float(ga.norm() / gb.norm()) - 1.0) < 0.01, (cos, float(ga.norm() / gb.norm()))
    per_cout = (ga * gb).sum((1, 2, 3)) / (gb * gb).sum((1, 2, 3))
    assert float((per_cout - 1).abs().max()) < 0.05       # (the frozen scale is applied per output channel)


@pytest.mark.parametrize("cin,cout,k,stride,bias", [(64, 64, 1, 1, True), (64, 64, 3, 1, True), (128, 128, 3, 2, True),
                                                    (256, 256, 3, 1, True), (64, 48, 3, 1, False)])
def test_conv2d_relu_epilogue_equals_conv_then_relu(cin, cout, k, stride, bias):
    """MI_CONV_RELU: the fused launch must give bit-identical outputs and gradients to conv2d followed by the separate ReLU
    pass (same convolution kernel, the clamp applied to the fp32 value before the single bf16 rounding)"""
    from yolov7_d2_amd.modeling.sparseinst import relu as ew_relu
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, cin, 20, 28, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).cuda()
    b = torch.randn(cout, generator=g).cuda() * 0.1 if bias else None
    dy = torch.randn(2, cout, (20 + 2 * (k // 2) - k) // stride + 1, (28 + 2 * (k // 2) - k) // stride + 1, generator=g)
    dy = dy.to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
    outs = []
    for fused in (True, False):
        xi, wi = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        bi = b.clone().requires_grad_(True) if bias else None
        if fused:
            y = torch.ops.mi355.conv2d_relu(xi, wi, bi, stride, k // 2)
        else:
            y = ew_relu(torch.ops.mi355.conv2d(xi, wi, bi, stride, k // 2))
        y.backward(dy)
        outs.append((y.detach().float(), xi.grad.float(), wi.grad.float(), bi.grad.float() if bias else None))
    assert (outs[0][0] > 0).float().mean().item() > 0.2
    for a, r in zip(*outs):
        if a is not None:
            assert torch.equal(a, r)


@pytest.mark.parametrize("cin,cout,bc,stride,xgrad", [(256, 512, 128, 2, True), (512, 512, 128, 1, True), (256, 256, 64, 1, True),
                                                      (256, 512, 128, 2, False)],
                         ids=["shortcut_s2", "identity", "identity_64", "shortcut_s2_no_dx"])
def test_bottleneck_as_one_node_equals_per_convolution_nodes(cin, cout, bc, stride, xgrad, monkeypatch):
    """_BottleneckFn (the second path of the input gradient accumulated in the convolution epilogue, MI_CONV_ACCUM) against the
    per-convolution autograd nodes + autograd's own additions: same kernels and roundings -> identical output and weight gradients, the input gradient to a bf16 rounding"""
    from yolov7_d2_amd.modeling.resnet import BottleneckBlock
    monkeypatch.setenv("MI_WGRAD_LAYER_GROUP", "0")     # one launch per weight gradient on both sides (the grouped form picks other split counts)
    torch.manual_seed(3)
    blk = BottleneckBlock(cin, cout, bc, stride=stride).cuda()
    for m in blk.modules():
        if hasattr(m, "running_var"):
            m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.1); m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, cin, 24, 36, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
    go = torch.randn(2, cout, 24 // stride, 36 // stride, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
    res = []
    monkeypatch.setenv("MI_RESNET_EPI_FUSE", "0")     # (the node structure is under test: the epilogue fusions have their own)
    for flag in ("1", "0"):
        monkeypatch.setenv("MI_RESNET_BLOCK_FN", flag)
        blk.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(xgrad)
        out = blk(xi)
        out.backward(go)
        res.append([out.detach().float()] + ([xi.grad.float()] if xgrad else []) + [p.grad.float().clone() for p in blk.parameters()])
    for i, (a, b) in enumerate(zip(*res)):
        if xgrad and i == 1:      # the input gradient: one rounding may move (accumulate-in-epilogue vs a separate bf16 add)
            assert _rel(a, b) < 4e-3
        else:
            assert torch.equal(a, b), (i, float((a - b).abs().max()))


@pytest.mark.parametrize("cin,cout,bc,stride", [(256, 512, 128, 2), (512, 512, 128, 1)], ids=["shortcut_s2", "identity"])
def test_bottleneck_grouped_weight_gradients_equal_single_launches(cin, cout, bc, stride, monkeypatch):
    """ops.WgradBatch inside _BottleneckFn.backward: the block's three or four weight gradients as ONE grouped launch, issued
    before the input gradient is accumulated into the tensor two of the jobs read - equal to the one-launch-per-layer form to
    the split-K summation order, input gradient and output bit for bit"""
    from yolov7_d2_amd.modeling.resnet import BottleneckBlock
    from yolov7_d2_amd.ops import WgradBatch
    res = []
    for grouped in ("0", "1"):
        monkeypatch.setenv("MI_WGRAD_LAYER_GROUP", grouped)
        torch.manual_seed(3)
        blk = BottleneckBlock(cin, cout, bc, stride=stride).cuda()
        for m in blk.modules():
            if hasattr(m, "running_var"):
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.1); m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
        g = torch.Generator().manual_seed(9)
        x = torch.randn(2, cin, 24, 36, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        go = torch.randn(2, cout, 24 // stride, 36 // stride, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
        n0 = dict(WgradBatch.stats)
        y = blk(x)
        y.backward(go)
        torch.cuda.synchronize()
        assert WgradBatch.stats["flushes"] - n0["flushes"] == int(grouped) and not WgradBatch.pending
        res.append((y.detach().float(), x.grad.float(), {k: p.grad.float() for k, p in blk.named_parameters() if p.grad is not None}))
    (y0, dx0, g0), (y1, dx1, g1) = res
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1) and set(g0) == set(g1) and len(g0) >= 3
    for k in g0:
        scale = float(g0[k].abs().max()) + 1e-30
        assert float((g0[k] - g1[k]).abs().max()) <= 2e-5 * scale, (k, float((g0[k] - g1[k]).abs().max()), scale)


@pytest.mark.parametrize("k,stride,cin,cout", [(1, 1, 64, 256), (3, 2, 128, 128), (1, 2, 256, 512)])
def test_folded_frozen_norm_conv_equals_the_explicit_fold(k, stride, cin, cout):
    """Conv2d + FrozenBatchNorm2d with the scale folded INSIDE the pack kernel (mi_pack_conv_weight_scaled) and the weight
    gradient rescaled by mi_scale_rows_f32, against the explicit form built here (torch `weight * scale`, mi355::conv2d with
    its ReLU epilogue, autograd's mul backward): the same fp32 products and roundings -> identical output, input gradient
    and weight gradient"""
    from yolov7_d2_amd.modeling.resnet import Conv2d
    torch.manual_seed(5)
    m = Conv2d(cin, cout, k, stride=stride, padding=k // 2).cuda()
    m.norm.weight.uniform_(0.5, 1.5); m.norm.bias.normal_(0, 0.1); m.norm.running_mean.normal_(0, 0.1); m.norm.running_var.uniform_(0.5, 1.5)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, cin, 20, 28, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
    go = torch.randn(2, cout, (20 - 1) // stride + 1, (28 - 1) // stride + 1, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
    res = []
    scale, shift = m.norm.affine()
    for folded in (True, False):
        m.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        if folded:
            out = m(xi, relu=True)
        else:
            out = torch.ops.mi355.conv2d_relu(xi, m.weight * scale.view(-1, 1, 1, 1), shift, stride, k // 2)
        out.backward(go)
        res.append((out.detach().float(), xi.grad.float(), m.weight.grad.float().clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b), float((a - b).abs().max())


def test_trainable_layer_without_autograd_never_reuses_a_packed_image():
    """Evaluation between training steps: a TRAINABLE Conv2d run under no_grad must see a weight update that bypasses torch's
    version counter (mi_adamw_step_multi and the arena SGD write through raw pointers) - its packed image is never cached;
    a FROZEN layer's is (the same tensor object always; re-packed in place when its buffers or weight are written through torch)."""
    from yolov7_d2_amd.modeling.resnet import Conv2d
    if not hasattr(torch.autograd, "_unsafe_preserve_version_counter"):
        pytest.skip("no torch.autograd._unsafe_preserve_version_counter in this torch")
    torch.manual_seed(1)
    m = Conv2d(64, 64, 3, padding=1).cuda()
    x = torch.randn(2, 64, 16, 24).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y1 = m(x).float().clone()
        with torch.autograd._unsafe_preserve_version_counter(m.weight):
            m.weight.mul_(2.0)                                   # what an optimizer kernel does: no version bump
        y2 = m(x).float().clone()
        shift = m.norm.affine()[1].view(1, -1, 1, 1)
        assert _rel(y2 - shift, 2.0 * (y1 - shift)) < 1e-2
        assert "_image" not in m.__dict__
        m.weight.requires_grad_(False)                           # frozen: cached, and refreshed when written through torch
        y3 = m(x).float().clone()
        assert "_image" in m.__dict__ and torch.equal(y3, y2)
        img = m.__dict__["_image"][1]
        assert m(x) is not None and m.__dict__["_image"][1] is img
        old = img.clone()
        m.weight.mul_(0.5)
        y4 = m(x).float()
        # re-packed INTO the same tensor (captured graphs hold its address: tests/test_frozen_constants.py), new contents
        assert m.__dict__["_image"][1] is img and not torch.equal(img, old) and _rel(y4 - shift, y1 - shift) < 1e-2


@pytest.mark.parametrize("cin,cout,bc,stride", [(256, 512, 128, 2), (512, 512, 128, 1), (256, 256, 64, 1)], ids=["shortcut_s2", "identity", "identity_64"])
def test_bottleneck_epilogue_fusions_equal_the_elementwise_passes(cin, cout, bc, stride, monkeypatch):
    """MI_RESNET_EPI_FUSE=1 (the default since round 4): conv3 + shortcut + ReLU in conv3's epilogue and the two ReLU masks in
    the data-gradient epilogues, against the elementwise passes they replace.  The epilogues themselves round exactly like
    the passes (forward output identical; the stride-2 block, whose convolutions stay on the tile kernel either way,
    identical throughout - first device run, round 4).  In the stride-1 blocks the masked data gradients move from the
    streaming 1x1 / weight-stationary 3x3 kernels to the tile kernel's EPI 2 instantiation, which sums the K products in
    another order: fp32 rounding, i.e. one bf16 ulp on a small fraction of the gradient elements (the bound
    test_gpu_conv3x3_ws.py holds the two kernel families to) - measured at the scale of the tensor, because the block
    input's gradient is the sum of two paths and where they cancel one ulp of a path is several of the sum."""
    from yolov7_d2_amd.modeling.resnet import BottleneckBlock
    torch.manual_seed(3)
    blk = BottleneckBlock(cin, cout, bc, stride=stride).cuda()
    for m in blk.modules():
        if hasattr(m, "running_var"):
            m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.1); m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, cin, 24, 36, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
    go = torch.randn(2, cout, 24 // stride, 36 // stride, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
    res = []
    for flag in ("1", "0"):
        monkeypatch.setenv("MI_RESNET_EPI_FUSE", flag)
        blk.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        out = blk(xi)
        out.backward(go)
        res.append([out.detach().float(), xi.grad.float()] + [p.grad.float().clone() for p in blk.parameters()])
    assert torch.equal(res[0][0], res[1][0])                       # forward: the same roundings in every block type
    for i, (a, b) in enumerate(zip(*res)):
        if stride == 2:
            assert torch.equal(a, b), (i, float((a - b).abs().max()))
            continue
        if i == 1:
            d = (a - b).abs()
            bound = 2.0 ** -7 * torch.maximum(torch.maximum(a.abs(), b.abs()), b.pow(2).mean().sqrt().expand_as(b))
            assert bool((d <= bound).all()), float((d / bound).max())
            assert float((d > 0).float().mean()) < 0.05
        elif i > 1:                                                 # fp32 weight gradients: sums of those bf16 values
            assert float((a - b).norm() / b.norm().clamp(min=1e-12)) < 2e-3, i


def test_weight_images_one_launch_equals_the_per_layer_packs():
    """ops.WeightImages (the captured steps' ONE pack launch per step, mi_pack_conv_weights_batch with the folded per-Cout
    factor in the job): record three layers through their ordinary pack calls - a 3x3 conv with a folded FrozenBatchNorm
    scale, a plain 1x1 conv, a row block of an attention in-projection - freeze, change the parameters the way an optimizer
    kernel does, run(): every image equals a fresh single-layer pack of the new values bit for bit; a weight that is not
    parameter-backed and a layer that was not recorded are served by their own launch."""
    from yolov7_d2_amd import ops
    g = torch.Generator().manual_seed(11)
    w3 = torch.nn.Parameter(torch.randn(72, 64, 3, 3, generator=g).cuda())          # Cout 72 -> padded to 96
    w1 = torch.nn.Parameter(torch.randn(256, 64, 1, 1, generator=g).cuda())
    wi = torch.nn.Parameter(torch.randn(3 * 256, 256, generator=g).cuda())
    late = torch.nn.Parameter(torch.randn(64, 64, 1, 1, generator=g).cuda())
    scale = (0.5 + torch.rand(72, generator=g)).cuda()
    reg = ops.WeightImages([w3, w1, wi, late])

    def packs():
        a = ops.pack_images(w3.detach(), 72, 64, 3, 3, 64, 96, 96, 64, True, True, scale)
        b = ops.pack_images(w1.detach(), 256, 64, 1, 1, 64, 256, 256, 64, True, False, None)
        c = ops.pack_images(wi.detach()[256:512], 256, 256, 1, 1, 256, 256, 256, 256)
        return a, b, c

    fresh = lambda: [tuple(None if t is None else t.clone() for t in p) for p in packs()]
    ops.WeightImages.active = reg
    try:
        rec = packs()                                                   # recording pass: own launches + registration
        reg.freeze()
        assert reg.launch[0] == 3 and reg.launch[2] == 9
        with torch.no_grad():
            for p in (w3, w1, wi):
                p.mul_(1.7).add_(0.01)
        reg.run()
        hit = packs()                                                   # no launch: the registered tensors themselves
        for r, h in zip(rec, hit):
            assert all(x is y for x, y in zip(r, h))
        other = ops.pack_images((w1.detach() * 2.0), 256, 64, 1, 1, 64, 256, 256, 64)       # a temporary: never registered
        assert other[0] is not rec[1][0]
        unrec = ops.pack_images(late.detach(), 64, 64, 1, 1, 64, 64, 64, 64)                 # after freeze: own launch
        assert len(reg.images) == 3
    finally:
        ops.WeightImages.active = None
    want = fresh()
    torch.cuda.synchronize()
    for h, w in zip(hit, want):
        for x, y in zip(h, w):
            assert (x is None) == (y is None)
            if x is not None:
                assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    ref = ops.pack_images(late.detach(), 64, 64, 1, 1, 64, 64, 64, 64)
    assert torch.equal(unrec[0].view(torch.int16), ref[0].view(torch.int16))


def test_frozen_bottleneck_add_relu_in_the_conv_epilogue_equals_the_separate_pass(monkeypatch):
    """a frozen BottleneckBlock (the FREEZE_AT prefix; every block at inference): conv3 + shortcut + ReLU from conv3's epilogue
    (MI_CONV_ADDRELU) against the separate add + ReLU pass (MI_RESNET_EPI_FUSE=0) - same roundings, bit for bit"""
    from yolov7_d2_amd.modeling.resnet import BottleneckBlock
    outs = []
    for fuse in ("0", "1"):
        monkeypatch.setenv("MI_RESNET_EPI_FUSE", fuse)
        for cin, cout, bc, stride in ((64, 256, 64, 1), (256, 256, 64, 1), (256, 512, 128, 2)):
            torch.manual_seed(5)
            blk = BottleneckBlock(cin, cout, bc, stride=stride).cuda()
            for m in blk.modules():
                if hasattr(m, "running_var"):
                    m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.1); m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
            for p in blk.parameters():
                p.requires_grad = False
            g = torch.Generator().manual_seed(7)
            x = torch.randn(2, cin, 40, 56, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
            y = blk(x)
            torch.cuda.synchronize()
            assert tuple(y.shape) == (2, cout, 40 // stride, 56 // stride)
            outs.append(y.float().cpu())
    n = len(outs) // 2
    for a, b in zip(outs[:n], outs[n:]):
        assert torch.equal(a, b) and float(a.abs().max()) > 0


def test_relu_mask_of_block_inputs_in_the_last_data_gradient_equals_the_separate_pass(monkeypatch):
    """round 6: a bottleneck whose input is a ReLU output (every block of the ResNet) applies that ReLU's mask to its input
    gradient in the epilogue of the last data gradient (MI_CONV_ACCUM | MI_CONV_RELUMASK: streaming kernel MODE 6 / tile kernel)
    and the previous block skips its own mask pass - against the separate pass per block (MI_RESNET_MASK_FUSE=0): every
    parameter gradient bit for bit, the chain's input gradient wherever the input is positive (where it is zero its producer
    masks it anyway)"""
    from yolov7_d2_amd.modeling.resnet import BottleneckBlock
    from yolov7_d2_amd import modeling
    res = []
    for fuse in ("0", "1"):
        monkeypatch.setenv("MI_RESNET_MASK_FUSE", fuse)
        torch.manual_seed(21)
        chain = torch.nn.Sequential(BottleneckBlock(64, 256, 64, stride=1), BottleneckBlock(256, 256, 64), BottleneckBlock(256, 256, 64),
                                    BottleneckBlock(256, 512, 128, stride=2), BottleneckBlock(512, 512, 128)).cuda()
        for blk in chain:
            blk.input_is_relu = True
            for m in blk.modules():
                if hasattr(m, "running_var"):
                    m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.1); m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
        g = torch.Generator().manual_seed(13)
        x = torch.randn(2, 64, 32, 64, generator=g).clamp(min=0).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        go = torch.randn(2, 512, 16, 32, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
        y = chain(x)
        y.backward(go)
        torch.cuda.synchronize()
        res.append((y.detach().float(), (x.grad.float() * (x.detach() > 0)), {k: p.grad.float() for k, p in chain.named_parameters() if p.grad is not None}))
    (y0, dx0, g0), (y1, dx1, g1) = res
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1) and float(dx0.abs().max()) > 0
    assert set(g0) == set(g1) and len(g0) == 17
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    from yolov7_d2_amd.modeling.resnet import _PREMASKED
    assert len(_PREMASKED) <= 1          # (the chain input's entry: nothing consumed it; dropped by the next pass)
