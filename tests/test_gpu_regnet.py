"""GPU (-m gpu): the RegNet module tree (yolov7_d2_amd/modeling/regnet.py) against the independent fp32 restatement of
tests/regnet_ref.py - single blocks (identity, projection, odd map, every group width), RegNetX_200MF as a whole in train and
eval mode - and DETR on that backbone, eager against captured.

Bounds.  Activations are stored in bf16 and the norms use batch statistics, so the product differs from an fp32 network by
storage round-off that the normalisation amplifies.  Every quantity q is measured as rel(q) = |got - ref|_2 / |ref|_2 against
the fp32 restatement (the worst member of a class of quantities); the FLOOR is the same figure for the restatement itself with
bf16 storage emulated (regnet_ref.bf16 wherever the product stores a map, weights rounded as the packed images are) against
itself in fp32.  Each bound is twice the larger of the two: bf16 round-off moves by about that much between seeds and shapes.
Measured on an MI355X (product / floor) beside each constant below.

On each block case the fused tail (one rounding) must also be no further from the restatement than the composition from the
existing launches (mi_bn_act_fwd(act 0) on the projection, mi_bn_act_fwd(act 0, res) on c, mi_ew_bf16 ReLU: three roundings)
on the same raw convolution outputs and statistics."""
import copy
import ctypes as C

import pytest
import torch

import regnet_ref as R
import yolov7_d2_amd as M
from yolov7_d2_amd import _lib as L
from yolov7_d2_amd.config import add_yolo_config, get_cfg
from yolov7_d2_amd.d2shim import Boxes, Instances
from yolov7_d2_amd.modeling import regnet as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# (w_in, w_out, stride, group width, H, W), batch 2
BLOCKS = [(64, 64, 1, 16, 14, 18),       # identity
          (32, 64, 2, 16, 15, 17),       # projection, odd map
          (24, 56, 2, 8, 14, 18),
          (48, 96, 2, 24, 8, 8)]
CLASSES = ("out", "dx", "conv_grad", "bn_weight_grad", "bn_bias_grad", "running_mean", "running_var")
# per block case and class: (bound, product, floor); bound = 2 x max(product, floor), figures measured on an MI355X
BLOCK_BOUNDS = [
    {   # (64, 64, 1, 16, 14, 18); tail against the restatement: fused 0.004396, composed 0.004396
        "out": (0.0088, 0.0044, 0.00439),
        "dx": (0.13, 0.0646, 0.0645),
        "conv_grad": (0.147, 0.0733, 0.0733),
        "bn_weight_grad": (0.145, 0.0722, 0.0716),
        "bn_bias_grad": (0.171, 0.0854, 0.0853),
        "running_mean": (0.00556, 0.00278, 0.00278),
        "running_var": (0.000292, 0.000146, 0.000146),
    },
    {   # (32, 64, 2, 16, 15, 17); tail against the restatement: fused 0.004717, composed 0.004833
        "out": (0.00944, 0.00472, 0.00472),
        "dx": (0.141, 0.0701, 0.07),
        "conv_grad": (0.161, 0.08, 0.0799),
        "bn_weight_grad": (0.146, 0.0729, 0.0729),
        "bn_bias_grad": (0.191, 0.0955, 0.0954),
        "running_mean": (0.00442, 0.00221, 0.00221),
        "running_var": (0.000263, 0.000131, 0.000131),
    },
    {   # (24, 56, 2, 8, 14, 18); tail against the restatement: fused 0.004714, composed 0.004946
        "out": (0.00943, 0.00471, 0.00471),
        "dx": (0.177, 0.0881, 0.0879),
        "conv_grad": (0.224, 0.112, 0.112),
        "bn_weight_grad": (0.206, 0.102, 0.103),
        "bn_bias_grad": (0.31, 0.155, 0.154),
        "running_mean": (0.00485, 0.00242, 0.00242),
        "running_var": (0.00023, 0.000115, 0.000115),
    },
    {   # (48, 96, 2, 24, 8, 8); tail against the restatement: fused 0.004618, composed 0.004786
        "out": (0.00924, 0.00462, 0.00462),
        "dx": (0.222, 0.111, 0.11),
        "conv_grad": (0.222, 0.111, 0.111),
        "bn_weight_grad": (0.258, 0.129, 0.129),
        "bn_bias_grad": (0.227, 0.113, 0.113),
        "running_mean": (0.00512, 0.00256, 0.00256),
        "running_var": (0.000403, 0.000201, 0.000201),
    },
]
# RegNetX_200MF at 2 x 3 x 64 x 96, per quantity (parameter gradients: the worst of the class): (bound, product, floor).  The
# gradients of the whole network sit above 100 % on BOTH sides: s4 normalises over 12 samples per channel and every ReLU whose
# argument changes sign under storage round-off flips a whole gradient entry, 13 blocks deep - the blocks above are the sharp check
NET_BOUNDS = {
    "s2": (0.0222, 0.0111, 0.0111),
    "s3": (0.0706, 0.0353, 0.0353),
    "s4": (0.504, 0.252, 0.252),
    "conv_grad": (2.75, 1.37, 1.37),
    "bn_weight_grad": (3.22, 1.61, 1.55),
    "bn_bias_grad": (3.55, 1.71, 1.77),
    "eval_s2": (0.00851, 0.00425, 0.00425),
    "eval_s3": (0.00834, 0.00417, 0.00417),
    "eval_s4": (0.00935, 0.00466, 0.00467),
}


def rel(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return float((got - ref).norm() / ref.norm().clamp(min=1e-30))


def _bf(t):
    return t.to(BF).float()


def _klass(name):
    if name.endswith("running_mean") or name.endswith("running_var"):
        return name.rsplit(".", 1)[1]
    if "bn" in name.rsplit(".", 2)[-2]:
        return "bn_weight_grad" if name.endswith("weight") else "bn_bias_grad"
    return "conv_grad"


def _randomise_norms(mod, g):
    """d2's init leaves every norm at (1, 0): give the affine parameters something to differentiate"""
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
            m.bias.data.copy_(0.2 * torch.randn(m.bias.shape, generator=g))


def _ref_step(ref, run, x, douts, quant):
    """one train-mode step of (a copy of) the restatement -> {quantity: tensor}"""
    ref = copy.deepcopy(ref).train()
    x = x.clone().requires_grad_(True)
    outs = run(ref, x, quant)
    loss = sum((outs[k] * douts[k]).sum() for k in outs)
    loss.backward()
    q = {"out." + k: v.detach() for k, v in outs.items()}
    q["dx"] = x.grad
    for n, p in ref.named_parameters():
        q[n] = p.grad
    for n, b in ref.named_buffers():
        if not n.endswith("num_batches_tracked"):
            q[n] = b.clone()
    return q


def _worst(got, ref):
    """class -> worst relative error over the quantities of that class"""
    w = {}
    for n, r in ref.items():
        k = n if n.startswith("out") or n == "dx" else _klass(n)
        k = "out" if k.startswith("out") else k
        w[k] = max(w.get(k, 0.0), rel(got[n], r))
    return w


def block_case(i):
    """-> (product errors, floor) by class, and the tail comparison (fused, composed) for block case i"""
    w_in, w_out, stride, gw, H, W = BLOCKS[i]
    g = torch.Generator().manual_seed(100 + i)
    torch.manual_seed(100 + i)                      # (d2's init draws the convolution weights from the global generator)
    ref = R.block(w_in, w_out, stride, gw)
    _randomise_norms(ref, g)
    x = _bf(torch.randn(2, w_in, H, W, generator=g))
    run = lambda m, xx, quant: {"y": R.run_block(m, xx, quant)}
    with torch.no_grad():
        shape = run(copy.deepcopy(ref), x, None)["y"].shape
    douts = {"y": _bf(torch.randn(shape, generator=g))}
    want = _ref_step(ref, run, x, douts, None)
    floor = _worst(_ref_step(ref, run, x, douts, R.bf16), want)
    blk = P.ResBottleneckBlock(w_in, w_out, stride, {"bot_mul": 1.0, "group_w": gw, "se_r": 0.0}).to(DEV)
    blk.load_state_dict(ref.state_dict())
    blk.train()
    xd = x.to(DEV).to(BF).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = blk(xd)
    assert out.dtype == BF and tuple(out.shape) == tuple(shape)
    out.backward(douts["y"].to(DEV).to(BF))
    torch.cuda.synchronize()
    got = {"out.y": out, "dx": xd.grad}
    for n, p in blk.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        got[n] = p.grad
    for n, b in blk.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(b) == 1, n
        else:
            got[n] = b
    err = _worst(got, want)
    return err, floor, tail_comparison(blk, xd.detach(), want["out.y"])


def tail_comparison(blk, x, ref_out):
    """the block's tail from the same raw convolution outputs and statistics: one fused launch against the composition from the
    existing launches; -> (fused error, composed error) against the restatement's block output"""
    lib, sp = L.lib(), L.stream_ptr()
    f = blk.f
    with torch.no_grad():
        state = copy.deepcopy(blk.state_dict())
        h = P._layer(P._layer(x, f.a, f.a_bn, True), f.b, f.b_bn, True)
        blk.load_state_dict(state)                  # (the two layers above advanced their running statistics)
        cc = P._Conv(h, f.c.weight, 1, 1, False, True)
        cp = P._Conv(x, blk.proj.weight, blk.stride, 1, False, True) if blk.proj is not None else None
        Cc, npix = cc.Cout, cc.npix
        new = lambda: torch.empty(x.shape[0], cc.Ho, cc.Wo, Cc, dtype=BF, device=DEV)
        fused, t1, t2, comp = new(), new(), new(), new()
        d = L.mi_bn_relu_desc()
        keep = [P._fill_fwd(d.n1, cc, f.c_bn, True)]
        d.n1.running_mean = d.n1.running_var = d.n1.num_batches_tracked = None
        xh = P._nhwc_v(x)
        if cp is not None:
            keep.append(P._fill_fwd(d.n2, cp, blk.bn, True))
            d.n2.running_mean = d.n2.running_var = d.n2.num_batches_tracked = None
        else:
            d.res, d.ldres = xh.data_ptr(), P._ld(xh)
        d.a, d.lda, d.npix, d.C, d.relu = fused.data_ptr(), Cc, npix, Cc, 1
        L.check(lib.mi_bn_relu_fwd(C.byref(d), sp), "mi_bn_relu_fwd")

        def bn_act(cv, bn, res, ldres, out):
            st = torch.empty(4, Cc, dtype=torch.float32, device=DEV)
            L.check(lib.mi_bn_act_fwd(cv.y.data_ptr(), Cc, cv.acc.data_ptr(), L.MI_BN_SLOTS, npix, bn.weight.data_ptr(),
                                      bn.bias.data_ptr(), bn.eps, 0.0, None, None, None, st[0].data_ptr(), st[1].data_ptr(),
                                      st[2].data_ptr(), st[3].data_ptr(), res, ldres, out.data_ptr(), Cc, npix, Cc, 0, sp), "mi_bn_act_fwd")
        if cp is not None:
            bn_act(cp, blk.bn, None, 0, t1)
            bn_act(cc, f.c_bn, t1.data_ptr(), Cc, t2)
        else:
            bn_act(cc, f.c_bn, xh.data_ptr(), P._ld(xh), t2)
        L.check(lib.mi_ew_bf16(t2.data_ptr(), None, comp.data_ptr(), t2.numel(), 1, sp), "mi_ew_bf16 relu")
        torch.cuda.synchronize()
        nchw = lambda t: t.permute(0, 3, 1, 2)
        return rel(nchw(fused), ref_out), rel(nchw(comp), ref_out)


@pytest.mark.parametrize("i", range(len(BLOCKS)), ids=["%d-%d-s%d-g%d-%dx%d" % b for b in BLOCKS])
def test_block_against_the_restatement(i):
    err, floor, (fused, comp) = block_case(i)
    print("block", BLOCKS[i], "product", err, "floor", floor, "tail fused / composed", fused, comp)
    assert set(err) == set(CLASSES)
    for k in CLASSES:
        assert err[k] <= BLOCK_BOUNDS[i][k][0], (k, err[k], floor[k], BLOCK_BOUNDS[i][k])
    assert fused <= comp, (fused, comp)


# ---------------------------------------------------------------------------------------------------------------- network
def _net_cfg(kind):
    cfg = add_yolo_config(get_cfg())
    cfg.MODEL.DEVICE = DEV
    cfg.MODEL.BACKBONE.NAME = "build_regnet_backbone"
    cfg.MODEL.REGNETS.TYPE = kind
    return cfg


def network_case():
    g = torch.Generator().manual_seed(7)
    torch.manual_seed(7)
    ref = R.RegNetRef("RegNetX_200MF")
    _randomise_norms(ref, g)
    x = _bf(torch.randn(2, 3, 64, 96, generator=g))
    run = lambda m, xx, quant: m(xx, quant)
    with torch.no_grad():
        shapes = {k: v.shape for k, v in copy.deepcopy(ref)(x).items()}
    douts = {k: _bf(torch.randn(s, generator=g)) for k, s in shapes.items()}
    want = _ref_step(ref, run, x, douts, None)
    fl = _ref_step(ref, run, x, douts, R.bf16)
    bb = M.build_backbone(_net_cfg("RegNetX_200MF")).to(DEV)
    bb.load_state_dict(ref.state_dict())
    bb.train()
    outs = bb(x.to(DEV))
    assert list(outs) == ["s2", "s3", "s4"]
    sum((outs[k].float() * douts[k].to(DEV)).sum() for k in outs).backward()
    torch.cuda.synchronize()
    err, floor = {}, {}
    for k in outs:
        err[k], floor[k] = rel(outs[k], want["out." + k]), rel(fl["out." + k], want["out." + k])
    for n, p in bb.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        k = _klass(n)
        err[k] = max(err.get(k, 0.0), rel(p.grad, want[n]))
        floor[k] = max(floor.get(k, 0.0), rel(fl[n], want[n]))
    # eval mode, the same state_dict on both sides
    ref_e = copy.deepcopy(ref).eval()
    bb.load_state_dict(ref.state_dict())
    bb.eval()
    with torch.no_grad():
        we, fe, ge = ref_e(x), ref_e(x, R.bf16), bb(x.to(DEV))
    for k in we:
        err["eval_" + k], floor["eval_" + k] = rel(ge[k], we[k]), rel(fe[k], we[k])
    return err, floor


def test_network_against_the_restatement():
    err, floor = network_case()
    print("RegNetX_200MF 2x3x64x96: product", err, "floor", floor)
    assert set(err) == set(NET_BOUNDS)
    for k, b in NET_BOUNDS.items():
        assert err[k] <= b[0], (k, err[k], floor[k], b)


# ------------------------------------------------------------------------------------------------------------------- DETR
def _batch(seed, sizes, counts):
    g = torch.Generator().manual_seed(seed)
    out = []
    for (h, w), n in zip(sizes, counts):
        wh = 16 + torch.rand(n, 2, generator=g) * 96
        xy = torch.rand(n, 2, generator=g) * (torch.tensor([w, h]) - wh).clamp(min=1)
        inst = Instances((h, w), gt_boxes=Boxes(torch.cat([xy, xy + wh], 1)), gt_classes=torch.randint(0, 80, (n,), generator=g))
        out.append(dict(image=torch.randint(0, 256, (3, h, w), generator=g).float().to(DEV), instances=inst))
    return out


def _detr():
    """the small configuration of tests/test_gpu_detr_graph.py (2 + 2 layers, 30 queries) on RegNetX_200MF"""
    cfg = M.detr_r50_cfg(device=DEV)
    cfg.MODEL.BACKBONE.NAME = "build_regnet_backbone"
    cfg.MODEL.REGNETS.TYPE = "RegNetX_200MF"
    cfg.MODEL.DETR.ENC_LAYERS, cfg.MODEL.DETR.DEC_LAYERS, cfg.MODEL.DETR.NUM_OBJECT_QUERIES = 2, 2, 30
    cfg.MODEL.DETR.DROPOUT = 0.0
    torch.manual_seed(11)
    model = M.build_model(cfg)
    model.train()
    return model


def test_detr_on_regnet_captured_step_equals_eager_step():
    from yolov7_d2_amd.graph_step import GraphedTrainStep
    batches = [_batch(1, ((256, 320), (224, 288)), (3, 2)), _batch(2, ((256, 320), (256, 256)), (1, 5)),
               _batch(3, ((320, 384), (300, 360)), (4, 4)), _batch(4, ((310, 384), (320, 350)), (2, 3))]     # two padded shapes
    eager = _detr()
    graphed = _detr()
    graphed.load_state_dict(eager.state_dict())
    opt = lambda m: torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-4, capturable=True)
    oe, og = opt(eager), opt(graphed)
    step = GraphedTrainStep(graphed, og)
    try:
        for it, b in enumerate(batches):
            # the eager step takes the route the captured one takes - prepare_batch + forward_prepared, module by module: forward()
            # itself divides by the host's box count where the prepared route multiplies by the device's 1 / count, one ulp apart
            # whenever the count is no power of two (6 boxes in the second batch) whatever the backbone
            losses = eager.forward_prepared(eager.prepare_batch(b))
            total = losses["total"] if "total" in losses else sum(v for k, v in losses.items() if k in eager.criterion.weight_dict)
            oe.zero_grad(set_to_none=True)
            total.backward()
            if it == 0:
                for n, p in eager.detr.backbone[0].backbone.named_parameters():
                    assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
            oe.step()
            out = step(b)
            for k, v in losses.items():
                assert torch.equal(out[k].float(), v.detach().float()), (it, k, float(out[k]), float(v.detach()))
        assert len(step.graphs) == 2
        torch.cuda.synchronize()
        be, bg = dict(eager.named_buffers()), dict(graphed.named_buffers())
        n = 0
        for k, v in be.items():
            if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
                assert torch.equal(v, bg[k]), k
                n += 1
                if k.endswith("num_batches_tracked"):
                    assert int(v) == len(batches), (k, int(v))
        assert n == 3 * 44          # RegNetX_200MF: the stem's norm, 13 blocks x 3 and 4 projection norms; three buffers each
    finally:
        step.close()
