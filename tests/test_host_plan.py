import os
"""CPU: host logic of the product (plan builder: buffer layout, concat slices, gradient fan-in flags, dgrad parity
classes, weight packing) checked by interpreting the symbolic plan with torch ops (tests/plan_interp.py) against
the fp32 oracle.  Storage is bf16 like the product's, so tolerances are the bf16 ones stated in SURVEY §8c."""
import numpy as np
import pytest
import torch

import yolox_oracle as O
from plan_interp import Interp

import yolov7_d2_amd as M
from yolov7_d2_amd import _lib as L
from yolov7_d2_amd.modeling.yolox import _PlanState
from yolov7_d2_amd.params import ParamArena


def _model(seed=0):
    cfg = M.yolox_s_cfg(device="cpu")
    model = M.build_model(cfg)
    sd = O.init_state_dict(0.33, 0.5, 80, seed=seed)
    model.load_state_dict(sd)
    model.params = ParamArena(model, "cpu")
    return model, sd


@pytest.mark.parametrize("fuse_bn_bwd", ["0", "1"])
def test_plan_step_matches_oracle(monkeypatch, fuse_bn_bwd):
    # "1": the BatchNorm-backward sums are taken by the data-gradient convs (MI_CONV_BNBWD) wherever the latest writer
    # of a layer's output gradient is such a conv; the remaining layers keep their BN_BWD_REDUCE command
    monkeypatch.setenv("MI_FUSE_BN_BWD", fuse_bn_bwd)
    model, sd = _model()
    B, H, W = 2, 64, 96
    imgs, labels = O.synth_batch(B, H, W, seed=11, max_gt=4)
    ps = _PlanState(model, B, H, W, True, materialize=False)
    b = ps.builder
    ps.image.copy_(imgs)
    ps.labels.copy_(labels)
    # fp32 storage: isolates the host logic (wiring, flags, packing, tap tables) from bf16 storage noise, which
    # the oracle's own bf16 emulation shows to be ~50% on single-step gradients of this random-init network
    # (gradient condition number ~500 w.r.t. per-layer relative perturbations; see DESIGN.md "Precision").
    nfused = sum(c.tag.endswith("+bnred") for c in b.bwd)
    nred = sum(c.op == L.OP["BN_BWD_REDUCE"] for c in b.bwd)
    assert (nfused, nred) == ((71, 21) if fuse_bn_bwd == "1" else (0, 74))
    it = Interp(b, torch.float32)
    it.run(b.prologue + b.fwd)
    out = it.raw(ps.loss["out"]).view(torch.float32)[:8].clone()
    # oracle
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    res = O.train_step_losses(sd, imgs, labels)
    ref = torch.tensor([float(x) for x in res[:4]])
    np.testing.assert_allclose(out[:4].numpy(), ref.numpy(), rtol=1e-4, atol=1e-4)
    # backward with detectron2's sum-of-dict weights
    it.raw(ps.loss["gw"]).view(torch.float32)[:4] = 1.0
    it.run(b.bwd)
    (res[0] + res[1] + res[2] + res[3]).backward()
    bad = []
    for name, p in model.named_parameters():
        g = model.params.grad_of(p).detach().float()
        r = sd[name].grad
        denom = float(r.norm()) + 1e-6
        rel = float((g - r).norm()) / denom
        if rel > 2e-3:
            bad.append((name, rel, float(r.norm())))
    assert not bad, bad[:10]
    # BN running statistics were updated through the plan
    rm = model.state_dict()["backbone.stem.conv.bn.running_mean"]
    np.testing.assert_allclose(rm.numpy(), sd["backbone.stem.conv.bn.running_mean"].detach().numpy(), rtol=1e-4, atol=1e-4)
    assert int(model.state_dict()["head.stems.2.bn.num_batches_tracked"]) == 1


def test_plan_step_with_l1_loss_matches_oracle():
    """the step plan with head.use_l1 on (what YOLOX.forward builds once update_iter() has passed
    INPUT.MOSAIC_AND_MIXUP.DISABLE_AT_ITER): five losses and every parameter gradient, detectron2 summing the loss dict
    including l1_loss"""
    model, sd = _model(seed=2)
    B, H, W = 2, 64, 96
    imgs, labels = O.synth_batch(B, H, W, seed=9, max_gt=4)
    ps = _PlanState(model, B, H, W, True, materialize=False, use_l1=True)
    b = ps.builder
    ps.image.copy_(imgs)
    ps.labels.copy_(labels)
    it = Interp(b, torch.float32)
    it.run(b.prologue + b.fwd)
    out = it.raw(ps.loss["out"]).view(torch.float32)[:8].clone()
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    res = O.train_step_losses(sd, imgs, labels, use_l1=True)
    assert float(res[4]) > 0.1
    np.testing.assert_allclose(out[:5].numpy(), np.array([float(x) for x in res[:5]]), rtol=1e-4, atol=1e-4)
    it.raw(ps.loss["gw"]).view(torch.float32)[:5] = 1.0
    it.run(b.bwd)
    (res[0] + res[1] + res[2] + res[3] + res[4]).backward()
    bad = []
    for name, p in model.named_parameters():
        g = model.params.grad_of(p).detach().float()
        r = sd[name].grad
        rel = float((g - r).norm()) / (float(r.norm()) + 1e-6)
        if rel > 2e-3:
            bad.append((name, rel))
    assert not bad, bad[:10]


def test_plan_step_depthwise_backbone_matches_oracle():
    """MODEL.DARKNET.DEPTH_WISE True: the backbone's 3x3 convs become DWConv (depthwise 3x3 + pointwise) - built from the
    config key, same state_dict keys as the reference, the plan (DWCONV_FWD / DGRAD / WGRAD commands between the usual
    BatchNorm passes) interpreted on the CPU against the oracle: losses and every parameter gradient"""
    cfg = M.yolox_s_cfg(device="cpu")
    cfg.MODEL.DARKNET.DEPTH_WISE = True
    model = M.build_model(cfg)
    sd = O.init_state_dict(0.33, 0.5, 80, seed=3, depthwise=True)
    model.load_state_dict(sd)          # strict: the DWConv keys (dconv.conv / dconv.bn / pconv.conv / pconv.bn) line up
    model.params = ParamArena(model, "cpu")
    B, H, W = 2, 64, 96
    imgs, labels = O.synth_batch(B, H, W, seed=12, max_gt=4)
    ps = _PlanState(model, B, H, W, True, materialize=False)
    b = ps.builder
    ops = [L.OPS[c.op] for c in b.fwd + b.bwd]
    assert ops.count("DWCONV_FWD") == 12 and ops.count("DWCONV_WGRAD") == 12 and ops.count("DWCONV_DGRAD") == 12   # 4 stage stems + 8 bottlenecks
    ps.image.copy_(imgs)
    ps.labels.copy_(labels)
    it = Interp(b, torch.float32)
    it.run(b.prologue + b.fwd)
    out = it.raw(ps.loss["out"]).view(torch.float32)[:8].clone()
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    res = O.train_step_losses(sd, imgs, labels, depthwise=True)
    np.testing.assert_allclose(out[:4].numpy(), np.array([float(x) for x in res[:4]]), rtol=1e-4, atol=1e-4)
    it.raw(ps.loss["gw"]).view(torch.float32)[:4] = 1.0
    it.run(b.bwd)
    (res[0] + res[1] + res[2] + res[3]).backward()
    bad = []
    for name, p in model.named_parameters():
        g = model.params.grad_of(p).detach().float()
        r = sd[name].grad
        rel = float((g - r).norm()) / (float(r.norm()) + 1e-6)
        if rel > 2e-3:
            bad.append((name, rel))
    assert not bad, bad[:10]
    # the materialised (dry-run) plan knows the depthwise weight gradients' place in the flat gradient arena
    from yolov7_d2_amd.plan import Plan
    from yolov7_d2_amd.parallel import grad_write_ranges
    plan = Plan(b, dry_run=True)
    covered = np.zeros(model.params.total, dtype=bool)
    for rs in grad_write_ranges(plan, model.params.grad):
        for (b0, b1) in rs:
            covered[b0 // 4: b1 // 4] = True
    for name, p, off, cnt in model.params.entries:
        assert covered[off: off + cnt].all(), name


def test_eval_plan_matches_oracle():
    model, sd = _model(seed=3)
    model.eval()
    B, H, W = 1, 64, 64
    imgs, _ = O.synth_batch(B, H, W, seed=5)
    ps = _PlanState(model, B, H, W, False, materialize=False)
    b = ps.builder
    assert not b.bwd
    ps.image.copy_(imgs)
    it = Interp(b)   # bf16 storage, like the product
    it.run(b.prologue + b.fwd)
    got = it.raw(ps.preds_buf).view(torch.float32)[: B * ps.A * 85].view(B, ps.A, 85)
    with torch.no_grad():
        net = O.Net(sd, 0.33, 0.5, 80, training=False)
        raw, hw = net.forward_raw(imgs)
        ref = O.decode_eval(raw, O.make_anchors(hw))
    np.testing.assert_allclose(got[..., :4].numpy(), ref[..., :4].numpy(), rtol=5e-2, atol=0.5)
    np.testing.assert_allclose(got[..., 4:].numpy(), ref[..., 4:].numpy(), rtol=5e-2, atol=5e-3)


def test_gradient_fanin_flags_and_buffers():
    model, _ = _model()
    ps = _PlanState(model, 2, 64, 64, True, materialize=False)
    b = ps.builder
    tags = [c.tag for c in b.bwd]
    # the loss gradient comes first, the stem's weight gradient last; the image never gets a gradient
    assert tags[0] == "bn_acc_zero.bwd" and tags[1] == "loss.bwd" and "backbone.stem.conv" in tags[-1]
    assert not any(t.startswith("backbone.stem.conv.dgrad") for t in tags)
    # stride-2 data gradients are 4 parity-class launches
    assert sum(t.startswith("backbone.dark3.0.dgrad") for t in tags) == 4
    # no NHWC tensor is copied for a concat: there is no COPY command at all
    from yolov7_d2_amd import _lib as L
    assert all(c.op != L.OP["COPY"] for c in b.fwd + b.bwd)
    n_conv = sum(c.op == L.OP["CONV"] for c in b.fwd)
    # 83 convolutions in YOLOX-s; reg_preds + obj_preds of a level run as ONE 5-channel convolution
    # (round 6: their parameters lie back to back in the arena, YOLOXHead.arena_adjacent): 83 - 3
    fused_head = os.environ.get("MI_HEAD_FUSE_REGOBJ", "1") != "0"
    assert n_conv == (80 if fused_head else 83)
    assert (sum("obj_preds" in t for t in tags) == 0) == fused_head and sum(t.startswith("head.reg_preds") for t in tags) > 0


def test_lane_scheduling_invariants():
    """Plan._group_lanes' pure part (plan.schedule_lanes) on the real YOLOX-s step plan: every parallel region (head
    stems, head level x branch chains, CSP conv1 / conv2) is scheduled into issue sets that (1) contain every command
    exactly once, (2) keep each lane's order, (3) never put two writers of one tensor into the same set and keep their
    original order, (4) are homogeneous in op, and (5) actually group: the head's 12 3x3 convs per direction come out
    as sets of 6"""
    from yolov7_d2_amd.plan import schedule_lanes, lane_out_key
    model, _ = _model()
    ps = _PlanState(model, 2, 64, 96, True, materialize=False)
    b = ps.builder
    NOP, CONV = L.OP["NOP"], L.OP["CONV"]
    nregions = 0
    sizes = {"fwd": [], "bwd": []}
    for which, cmds in (("fwd", b.fwd), ("bwd", b.bwd)):
        k = 0
        while k < len(cmds):
            if cmds[k].op == NOP and cmds[k].tag.endswith(".begin"):
                e = k + 1
                while not (cmds[e].op == NOP and cmds[e].tag.endswith(".end")):
                    e += 1
                region = cmds[k + 1: e]
                nregions += 1
                order = {id(c): i for i, c in enumerate(region)}
                sets = schedule_lanes(region)
                flat = [c for s_ in sets for c in s_]
                assert sorted(map(id, flat)) == sorted(map(id, region))                       # (1)
                for ln in {c.lane for c in region}:                                            # (2)
                    seq = [order[id(c)] for c in flat if c.lane == ln]
                    assert seq == sorted(seq)
                last = {}
                for si, s_ in enumerate(sets):
                    assert len({c.op for c in s_}) == 1                                        # (4)
                    keys = [lane_out_key(c) for c in s_]
                    assert len(set(keys)) == len(keys)                                         # (3a)
                    for c, kk in zip(s_, keys):
                        if kk in last:
                            assert last[kk][0] < si and last[kk][1] < order[id(c)]             # (3b)
                        last[kk] = (si, order[id(c)])
                    if s_[0].op == CONV and len(s_[0].desc.taps) == 9 and "head" in s_[0].tag:
                        sizes[which].append(len(s_))
                k = e + 1
            else:
                k += 1
    assert nregions == 2 * (2 + 8)           # head stems + head chains + 8 CSP layers, forward and backward
    assert sizes["fwd"] == [6, 6]             # cls/reg conv 0 and conv 1 of the three levels
    # backward: conv-1 data gradients of the 6 chains together; the conv-0 data gradients write the 3 stem gradients
    # twice (cls + reg branch) -> two ordered sets of 3
    assert sorted(sizes["bwd"]) == [3, 3, 6]


def test_wgrad_split_is_opt_in_and_ordered(monkeypatch):
    """MI_WGRAD_SPLIT (default: only under torch.distributed with world_size > 1): the head + neck weight gradients form
    an early group placed after the last head / neck backward command and before any backbone backward command"""
    model, _ = _model()
    b0 = _PlanState(model, 2, 64, 96, True, materialize=False).builder
    assert b0.wgrad_split is False
    monkeypatch.setenv("MI_WGRAD_SPLIT", "1")
    b1 = _PlanState(model, 2, 64, 96, True, materialize=False).builder
    assert b1.wgrad_split is True and b1.wgrad_early_prefixes == ("head.", "neck.")
    tags = [c.tag for c in b1.bwd]
    wg = [i for i, c in enumerate(b1.bwd) if c.op == L.OP["WGRAD"]]
    early = [i for i in wg if tags[i].startswith(("head.", "neck."))]
    late = [i for i in wg if i not in early]
    # 24 + 24 convs, 35 in the backbone (reg_preds + obj_preds as one convolution per level: 48 - 3)
    assert len(early) == (45 if os.environ.get("MI_HEAD_FUSE_REGOBJ", "1") != "0" else 48) and len(late) == 35
    first_backbone = min(i for i, t in enumerate(tags) if t.startswith("backbone."))
    assert max(early) < first_backbone                            # the early group can be issued before the backbone's backward


def test_plan_step_matches_oracle_yolox_l():
    """the same plan builder on YOLOX-l (depth 1.0, width 1.0: 54.2 M parameters, 9/9/9/3-bottleneck CSP stages, up to
    1024 channels): losses and every parameter gradient of the interpreted plan against the fp32 oracle - the host logic
    is not specialised to the YOLOX-s shapes of the benchmark"""
    cfg = M.yolox_s_cfg(device="cpu")
    cfg.MODEL.YOLO.DEPTH_MUL, cfg.MODEL.YOLO.WIDTH_MUL = 1.0, 1.0
    model = M.build_model(cfg)
    sd = O.init_state_dict(1.0, 1.0, 80, seed=0)
    model.load_state_dict(sd)
    model.params = ParamArena(model, "cpu")
    assert sum(p.numel() for p in model.parameters()) == 54208895
    B, H, W = 2, 128, 128
    imgs, labels = O.synth_batch(B, H, W, seed=11, max_gt=4)
    ps = _PlanState(model, B, H, W, True, materialize=False)
    b = ps.builder
    ps.image.copy_(imgs)
    ps.labels.copy_(labels)
    it = Interp(b, torch.float32)
    it.run(b.prologue + b.fwd)
    out = it.raw(ps.loss["out"]).view(torch.float32)[:4].clone()
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    res = O.train_step_losses(sd, imgs, labels, depth=1.0, width=1.0)
    np.testing.assert_allclose(out.numpy(), np.array([float(x.detach()) for x in res[:4]]), rtol=1e-5, atol=1e-5)
    it.raw(ps.loss["gw"]).view(torch.float32)[:4] = 1.0
    it.run(b.bwd)
    (res[0] + res[1] + res[2] + res[3]).backward()
    bad = []
    for name, p in model.named_parameters():
        g, r = model.params.grad_of(p).detach().float(), sd[name].grad
        rel = float((g - r).norm()) / (float(r.norm()) + 1e-6)
        if rel > 3e-3:
            bad.append((name, rel))
    assert not bad, bad[:8]


@pytest.mark.parametrize("split", ["0", "1"])
def test_gradient_buckets_are_complete_before_their_allreduce(monkeypatch, split):
    """data-parallel schedule on the REAL YOLOX-s backward list (materialised against a host arena: grouped conv /
    BatchNorm / weight-gradient launches, job tables and all): every byte of the flat gradient arena is written by some
    backward command, the buckets tile the arena, and each bucket's all-reduce is issued only after the LAST command that
    writes into it - with the split weight-gradient groups the neck + head bucket goes out before the first backbone
    command"""
    from yolov7_d2_amd.plan import Plan
    from yolov7_d2_amd.parallel import GradReducer, grad_write_ranges, plan_buckets
    monkeypatch.setenv("MI_WGRAD_SPLIT", split)
    model, _ = _model()
    ps = _PlanState(model, 2, 64, 96, True, materialize=False)
    plan = Plan(ps.builder, dry_run=True)
    arena = model.params
    writes = grad_write_ranges(plan, arena.grad)
    n = plan.bwd_cmds[1]
    assert len(writes) == n
    # (1) every parameter's gradient is written by some command
    covered = np.zeros(arena.total, dtype=bool)
    for rs in writes:
        for (b0, b1) in rs:
            covered[b0 // 4: b1 // 4] = True
    for name, p, off, cnt in arena.entries:
        assert covered[off: off + cnt].all(), name
    # (2) buckets (the engine's choice for world > 1) tile the arena and are reduced after their last writer
    bounds = None
    if split == "1":
        bounds = [min(o for (nm, p, o, c) in arena.entries if nm.startswith(("head.", "neck.")))]
    buckets = plan_buckets(arena.total, writes, 3, bounds=bounds)
    assert sorted((lo, hi) for lo, hi, _ in buckets)[0][0] == 0
    assert sum(hi - lo for lo, hi, _ in buckets) == arena.total
    segs = GradReducer(arena.grad, buckets).segments(n)
    assert segs[0][0] == 0 and segs[-1][1] == n and all(a[1] == b_[0] for a, b_ in zip(segs, segs[1:]))
    for (c0, c1, bucket) in segs:
        if bucket is None:
            continue
        lo, hi = bucket
        for k, rs in enumerate(writes):
            if any(b0 < hi * 4 and lo * 4 < b1 for (b0, b1) in rs):
                assert k < c1, (bucket, k, c1, plan.bwd_tags[k])
    tags = plan.bwd_tags
    if split == "1":
        first_backbone = min(i for i, t in enumerate(tags) if t.startswith("backbone."))
        assert len(buckets) == 2 and segs[0][1] <= first_backbone and "wgrad_group.early" in tags
    else:
        assert "wgrad_group.early" not in tags and tags[-1] == "wgrad_group"


def test_grouped_launches_of_the_640_plan(monkeypatch):
    """regression guard for the launch structure of the benchmark-sized plan (dry-run, 640x640): the head's level x branch
    chains and the CSP conv1 / conv2 pairs really come out as grouped launches (a group planner that silently falls back
    to one launch per layer costs ~6 % of the step and no other test would notice), and no grouped conv launch exceeds
    the 80 KB LDS footprint that keeps two blocks per CU"""
    import collections
    import ctypes as C
    from yolov7_d2_amd.plan import Plan
    monkeypatch.setenv("MI_BN_IN_CONSUMER", "0")      # (the launch structure WITHOUT the BatchNorm fold; the fold has its own test below)
    model, _ = _model()
    ps = _PlanState(model, 2, 640, 640, True, materialize=False)
    plan = Plan(ps.builder, dry_run=True)
    # (round 6: reg_preds + obj_preds of a level are ONE convolution - YOLOXHead.arena_adjacent -, so the three obj_preds jobs
    #  and their accumulating data gradients no longer form launches of their own; MI_HEAD_FUSE_REGOBJ=0: round 5's structure)
    fh = os.environ.get("MI_HEAD_FUSE_REGOBJ", "1") != "0"
    want = {"fwd": dict(CONV_GROUP=12 if fh else 13, BN_GROUP=11, CONV=43, BN_ACT_FWD=43),
            "bwd": dict(CONV_GROUP=11 if fh else 12, BN_GROUP=11, BN_BWD_FUSED=43, BN_BWD_REDUCE=0, BN_BWD_APPLY=0, WGRAD_GROUP=1,
                        SPLIT_DPREDS_BATCH=0, SPLIT_DPREDS=0, LOSS_BWD_FUSED=1, LOSS_BWD=0, BIAS_GRADS=0)}
    jobs = {"fwd": [2] * 8 + ([3, 6, 6, 6] if fh else [3, 6, 6, 6, 3]),
            "bwd": ([6, 6, 3, 3, 3] if fh else [6, 3, 6, 3, 3, 3]) + [4] * 6}    # + the parity classes of the six stride-2 data gradients
    for which in ("fwd", "bwd"):
        arr, n = plan.fwd_cmds if which == "fwd" else plan.bwd_cmds
        ops = collections.Counter(L.OPS[arr[k].op] for k in range(n))
        for op, cnt in want[which].items():
            assert ops[op] == cnt, (which, op, ops[op], cnt)
        metas = [C.cast(arr[k].p[0], C.POINTER(L.mi_conv_group)).contents for k in range(n) if L.OPS[arr[k].op] == "CONV_GROUP"]
        assert [m.njobs for m in metas] == jobs[which]
        # CSP conv1 + conv2 pairs read one tensor: they leave as ONE streaming 1x1 launch (KC == -1, csrc/conv1x1_stream.h;
        # persistent blocks with an LDS ring, one or two per CU by design) wherever N*H*W is a multiple of its pixel tile
        stream = [m.njobs for m in metas if m.KC == -1]
        assert stream == ([2] * 6 if which == "fwd" else []), (which, stream)
        # the head's 3x3 128 -> 128 towers (six jobs per launch) run on the weight-stationary kernel (KC == -2): one
        # persistent block per CU by design
        ws = [m.njobs for m in metas if m.KC == -2]
        assert ws == ([6, 6] if which == "fwd" else [6, 3, 3]), (which, ws)
        assert all(m.lds_bytes <= 80 * 1024 for m in metas if m.KC > 0)


@pytest.mark.parametrize("depth,width", [(0.33, 0.375), (0.67, 0.75), (1.33, 1.25)], ids=["tiny", "m", "x"])
def test_plan_step_other_widths(depth, width):
    """YOLOX-tiny / -m / -x: channel counts that are not multiples of 32 (24, 48, 80 ...; C/8 not a power of two) - padded
    pixel strides, zero-padded weight images, real-channel BatchNorm - through the same plan builder, interpreted on
    the CPU in fp32 against the oracle: the four losses and every parameter gradient"""
    cfg = M.yolox_s_cfg(device="cpu")
    cfg.MODEL.YOLO.DEPTH_MUL, cfg.MODEL.YOLO.WIDTH_MUL = depth, width
    model = M.build_model(cfg)
    sd = O.init_state_dict(depth, width, 80, seed=1)
    model.load_state_dict(sd)
    model.params = ParamArena(model, "cpu")
    B, H, W = 2, 64, 96
    imgs, labels = O.synth_batch(B, H, W, seed=11, max_gt=4)
    ps = _PlanState(model, B, H, W, True, materialize=False)
    b = ps.builder
    ps.image.copy_(imgs)
    ps.labels.copy_(labels)
    it = Interp(b, torch.float32)
    it.run(b.prologue + b.fwd)
    out = it.raw(ps.loss["out"]).view(torch.float32)[:8].clone()
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    res = O.train_step_losses(sd, imgs, labels, depth=depth, width=width)
    ref = torch.tensor([float(x) for x in res[:4]])
    np.testing.assert_allclose(out[:4].numpy(), ref.numpy(), rtol=1e-3, atol=1e-4)   # few anchors: bf16 weight images move a loss by ~3e-4
    it.raw(ps.loss["gw"]).view(torch.float32)[:4] = 1.0
    it.run(b.bwd)
    (res[0] + res[1] + res[2] + res[3]).backward()
    bad = []
    for name, p in model.named_parameters():
        g = model.params.grad_of(p).detach().float()
        r = sd[name].grad
        rel = float((g - r).norm()) / (float(r.norm()) + 1e-6)
        if rel > 5e-3:   # (a mis-wired slice / pad channel is an O(1) error; fp32 summation order with 12 samples per
            #  channel in the deepest BatchNorm layers is ~1e-3)
            bad.append((name, rel, float(r.norm())))
    assert not bad, bad[:10]


def test_batchnorm_in_the_consumer_pass_of_the_640_plan(monkeypatch):
    """plan.Plan._defer_bn on the benchmark-sized plan (dry run): MI_BN_IN_CONSUMER=1 drops the BN_ACT_FWD job of every layer
    whose first reader is a forward convolution on the streaming 1x1 / weight-stationary 3x3 kernel (never one with a
    residual, never a reader on the tile kernel), the reader's descriptor then reads the RAW conv output and carries the
    device record; launches of one input share the record and exactly one of them writes the activated tensor; `auto` (the
    default) keeps the measured winners only; the builder's symbolic lists are untouched."""
    import collections
    import ctypes as C
    from yolov7_d2_amd.plan import Plan
    model, _ = _model()
    ps = _PlanState(model, 16, 640, 640, True, materialize=False)
    nfwd = len(ps.builder.fwd)
    counts = {}
    for mode in ("0", "auto", "1"):
        monkeypatch.setenv("MI_BN_IN_CONSUMER", mode)
        plan = Plan(ps.builder, dry_run=True)
        assert len(ps.builder.fwd) == nfwd and sum(c.op == L.OP["BN_ACT_FWD"] for c in ps.builder.fwd) == 74
        arr, n = plan.fwd_cmds
        members = plan.cmd_members["fwd"]
        nbn = sum((len(members[k]) if members[k] else 1) for k in range(n) if L.OPS[arr[k].op] in ("BN_ACT_FWD", "BN_GROUP"))
        assert nbn == 74 - len(plan.deferred_bn)
        counts[mode] = len(plan.deferred_bn)
        assert not any(".conv2.bnact" in t and ".m." in t and t.startswith("backbone.dark2") for t in plan.deferred_bn)   # (shortcut: has a residual)
        xf = collections.defaultdict(list)
        for k in range(n):
            ds = plan.cmd_descs["fwd"][k]
            if L.OPS[arr[k].op] == "CONV":
                ds = [ds]
            elif L.OPS[arr[k].op] != "CONV_GROUP":
                continue
            for d in ds:
                if d.xf:
                    assert d.stats_acc and not d.flags and d.xf_C == d.K8 * 8
                    assert L.lib().mi_conv2d_route(C.byref(d)) in (1, 2)
                    xf[(k, d.xf)].append(d.xf_write)
        assert all(sum(w) == 1 for w in xf.values()), xf
        assert len(xf) == len(plan.deferred_bn)
    assert counts["0"] == 0 and counts["1"] >= 35 and 1 <= counts["auto"] <= 10, counts


@pytest.mark.parametrize("env", [{}, {"MI_GROUP_LEVELS": "0"}, {"MI_WGRAD_SPLIT": "1"}, {"MI_BN_IN_CONSUMER": "1"},
                                 {"MI_FUSE_BN_BWD": "1"}, {"MI_BN_FUSED": "0"}, {"MI_BN_FUSED": "1"}],
                         ids=["default", "levels0", "wgrad_split", "bn_in_consumer", "fuse_bn_bwd", "bn_fused0", "bn_fused1"])
def test_materialized_lists_mean_the_builder_lists(monkeypatch, env):
    """the MATERIALISED command lists (lane scheduling, parity groups, BatchNorm in the consumer, fused BatchNorm backward
    pairs, batched prediction splits, the fused loss backward, the staged weight-gradient groups, the weight-pack batch)
    interpreted through their members - Plan.cmd_objs / cmd_members - compute what the builder's lists compute: losses,
    every parameter gradient and the BatchNorm running statistics to fp32 reordering noise.  A reader scheduled before its
    writer, a dropped or doubled member or a lost accumulation shows up as an O(1) error."""
    from yolov7_d2_amd.plan import Plan
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model, _ = _model(seed=4)
    B, H, W = 2, 64, 96
    imgs, labels = O.synth_batch(B, H, W, seed=13, max_gt=4)
    ps = _PlanState(model, B, H, W, True, materialize=False)
    b = ps.builder
    plan = Plan(b, dry_run=True)
    if env.get("MI_BN_IN_CONSUMER") == "1":
        assert len(plan.deferred_bn) >= 20      # (26 at this size; the streaming kernels do not take every small map)
    ps.image.copy_(imgs)
    ps.labels.copy_(labels)
    state0 = [(t, t.clone()) for t in b.tune_restore]
    res = {}
    for form in ("builder", "materialized"):
        for t, v in state0:
            t.copy_(v)
        model.params.grad.zero_()
        it = Interp(b, torch.float32)
        if form == "builder":
            it.run(b.prologue + b.fwd)
        else:
            it.run_materialized(plan, "fwd")
        out = it.raw(ps.loss["out"]).view(torch.float32)[:8].clone()
        it.raw(ps.loss["gw"]).view(torch.float32)[:4] = 1.0
        if form == "builder":
            it.run(b.bwd)
        else:
            it.run_materialized(plan, "bwd")
        res[form] = (out, model.params.grad.clone(), [t.clone() for t, _ in state0])
    (o0, g0, s0), (o1, g1, s1) = res["builder"], res["materialized"]
    np.testing.assert_allclose(o1.numpy(), o0.numpy(), rtol=1e-5, atol=1e-7)
    assert float(o0[6]) > 0
    bad = []
    for name, p, off, cnt in model.params.entries:
        a, r = g1[off: off + cnt], g0[off: off + cnt]
        rel = float((a - r).norm() / (r.norm() + 1e-30))
        if rel > 1e-5:           # (a gradient that is zero - a head level without foreground - must stay zero)
            bad.append((name, rel))
    assert not bad, bad[:8]
    assert sum(float(g0[off: off + cnt].norm()) > 0 for _, _, off, cnt in model.params.entries) > 0.9 * len(model.params.entries)
    for a, r in zip(s1, s0):
        if r.is_floating_point():
            assert float((a - r).norm() / (r.norm() + 1e-30)) <= 1e-5
        else:
            assert torch.equal(a, r)


def test_materialized_lists_cover_every_builder_command():
    """every symbolic command of the builder's lists is a member of exactly one materialised command (the weight packs of
    PACK_W_BATCH and the layers of a WGRAD_GROUP included); the region markers are the only ones dropped"""
    from yolov7_d2_amd.plan import Plan
    model, _ = _model()
    ps = _PlanState(model, 2, 64, 96, True, materialize=False)
    b = ps.builder
    plan = Plan(b, dry_run=True)
    for which, sym in (("fwd", b.prologue + b.fwd), ("bwd", b.bwd)):
        ran = [m for c in plan.cmd_objs[which] for m in Interp.members(c)]
        assert len(ran) == len({id(m) for m in ran})
        want = {id(c) for c in sym if not (L.OPS[c.op] == "NOP" and c.tag.endswith((".begin", ".end")))}
        got = {id(m) for m in ran if not getattr(m.desc, "xf", None)}
        # (a convolution that applies its input's BatchNorm is a copy of its builder command; its BN_ACT_FWD is absorbed)
        xf = [m for m in ran if getattr(m.desc, "xf", None) is not None]
        absorbed = {id(m.desc.xf_bn) for m in xf}
        assert got | absorbed | {id(c) for c in sym if any(c.tag == m.tag and c.op == m.op for m in xf)} == want
    ops = [L.OPS[c.op] for c in plan.cmd_objs["fwd"]]
    k = ops.index("PACK_W_BATCH")
    assert len(plan.cmd_members["fwd"][k]) == sum(c.op == L.OP["PACK_W"] for c in b.prologue)
    k = [L.OPS[c.op] for c in plan.cmd_objs["bwd"]].index("WGRAD_GROUP")
    assert len(plan.cmd_members["bwd"][k]) == sum(c.op == L.OP["WGRAD"] for c in b.bwd)


def _synthetic_case(seed=0):
    """a 2 x 24 x 40 image of a 64-channel concat buffer whose channel slice [16, 48) is the command's output view and
    [48, 64) a view it only reads, and a plausible correct device result: the reference rounded differently by up to one
    bf16 ulp on a few percent of the output's elements"""
    from plan_compare import Layout
    from yolov7_d2_amd.plan import Buf, TRef, _Cmd, _Ptr
    N, H, W, ld = 2, 24, 40, 64
    buf = Buf("neck.cat", N * H * W * ld * 2)
    t = TRef(buf, N, H, W, 32, ld, 16)
    g = torch.Generator().manual_seed(seed)
    ref = torch.randn(N, H, W, ld, generator=g).to(torch.bfloat16)
    got = ref.clone()
    flip = torch.rand(N, H, W, ld, generator=g) < 0.05
    sub = got[..., 16:48].view(torch.int16)
    sub += (flip[..., 16:48] & (torch.rand(N, H, W, 32, generator=g) < 0.5)).to(torch.int16)   # +1 ulp (same sign)
    got[..., 16:48] = sub.view(torch.bfloat16)
    cmd = _Cmd(L.OP["UPSAMPLE_BWD"], p=[_Ptr(TRef(buf, N, H, W, 16, ld, 48)), _Ptr(t)])
    return buf, Layout([cmd]), got, ref


def test_comparator_passes_rounding_noise_and_flags_subtle_damage():
    """tests/plan_compare.py on synthetic bf16 tensors: one-ulp rounding differences pass; a 16 x 16 tile off by 4 ulps,
    one dropped pixel row, one channel scaled by 1.005 (< 1.3 ulps per element) and one byte changed in a sibling concat
    slice the command only reads (or does not name at all) are each flagged, with the buffer and the first bad
    (n, h, w, c)"""
    from plan_compare import Report, compare_buffer

    def run(got):
        rep = Report()
        ok = compare_buffer(buf, got.view(-1).view(torch.uint8), ref.view(-1).view(torch.uint8), lay, rep, tag="t", op="CONV")
        return ok, rep

    buf, lay, got, ref = _synthetic_case()
    ok, rep = run(got)
    assert ok, str(rep)
    # (1) a 16 x 16 pixel tile of one channel group off by 4 ulps
    bad = got.clone()
    v = bad[1, 4:20, 8:24, 24:32].view(torch.int16)
    v += 4
    ok, rep = run(bad)
    assert not ok and rep.fails[0]["kind"] == "bf16" and rep.fails[0]["first"][:3] == (1, 4, 8), str(rep)
    # (2) a dropped pixel row (stale zeros)
    bad = got.clone()
    bad[0, 7, :, 16:48] = 0
    ok, rep = run(bad)
    assert not ok and rep.fails[0]["first"][:2] == (0, 7), str(rep)
    # (3) one channel scaled by 1.005
    bad = got.clone()
    bad[..., 37] = (bad[..., 37].float() * 1.005).to(torch.bfloat16)
    ok, rep = run(bad)
    assert not ok and any(f["kind"] == "bf16-gain" and f["first"] == ("channel", 37) for f in rep.fails), str(rep)
    assert not any(f["kind"] == "bf16" for f in rep.fails)       # (no element is off by more than the ulp bound)
    # (4) one byte of a sibling slice the command reads (channel 50: a one-ulp stray store), (5) of one it does not name
    for ch in (50, 5):
        bad = got.clone()
        bb = bad.view(-1).view(torch.uint8)
        i = ((1 * 24 + 3) * 40 + 5) * 64 * 2 + ch * 2
        bb[i] ^= 1
        ok, rep = run(bad)
        assert not ok and rep.fails[0]["kind"] == "exact" and rep.fails[0]["first"] == (1, 3, 5, ch), str(rep)


def test_comparator_fp32_and_accumulator_rules():
    """fp32 reductions: reordering noise passes, a 3e-5 error (of max|ref|) on one element fails; fp64 slot accumulators are compared
    as sums over their slots (the device spreads a channel over slots, the interpreter adds to slot 0)"""
    from plan_compare import Layout, Report, compare_buffer
    from yolov7_d2_amd.plan import Buf, _Cmd, _Ptr, TRef
    g = torch.Generator().manual_seed(1)
    sc = Buf("backbone.stem.conv.scale", 64 * 4)
    r = torch.randn(64, generator=g)
    noisy = r * (1 + 1e-7 * torch.randn(64, generator=g))
    lay = Layout([])
    rep = Report()
    assert compare_buffer(sc, noisy.view(torch.uint8), r.view(torch.uint8), lay, rep)
    bad = noisy.clone()
    bad[5] += 3e-5 * float(r.abs().max())
    assert not compare_buffer(sc, bad.view(torch.uint8), r.view(torch.uint8), lay, rep) and rep.fails[-1]["first"] == 5
    # accumulators: 4 slots x 32 channels x (sum, sumsq)
    acc = Buf("scratch.bn_acc_fwd", 4 * 32 * 16)
    y = TRef(Buf("y", 64), 1, 1, 1, 32, 32)
    cmd = _Cmd(L.OP["BN_ACT_FWD"], i=[32, 0, 32, 32, 1, 4], p=[_Ptr(y), _Ptr(acc, 0)] + [_Ptr(None)] * 11, l=[1, 1])
    lay = Layout([cmd])
    dev = torch.randn(4, 32, 2, dtype=torch.float64, generator=g)
    ref = torch.zeros_like(dev)
    ref[0] = dev.sum(0)
    rep = Report()
    assert compare_buffer(acc, dev.view(-1).view(torch.uint8), ref.view(-1).view(torch.uint8), lay, rep), str(rep)
    dev[2, 7, 0] += 0.5
    assert not compare_buffer(acc, dev.view(-1).view(torch.uint8), ref.view(-1).view(torch.uint8), lay, rep)
