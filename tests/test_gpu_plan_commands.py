"""GPU (-m gpu): every command of the materialised YOLOX step plan, one at a time, against the plan interpreter run on
the SAME input bytes (teacher forcing): before command k the interpreter's host mirror receives the device's copy of
every arena buffer and tensor the command's members touch; after the launch each of them is compared in full with the
interpreter's result (tests/plan_compare.py: bf16 ulps, fp32 reductions, exact integers / copies / untouched slices),
and every arena / gradient-arena byte outside them must be unchanged.  No decorrelation: the bounds sit at bf16
rounding level at the production shapes, tile choices, split-K and merged launches."""
import ctypes as C
import time

import pytest
import torch

import yolox_oracle as O
from plan_compare import Layout, Report, compare_buffer, _f32_rule
from plan_interp import Interp
import yolov7_d2_amd as M
from yolov7_d2_amd import _lib as L
from yolov7_d2_amd.plan import Buf, Plan, TRef

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu_model(seed=0):
    cfg = M.yolox_s_cfg(device=DEV)
    model = M.build_model(cfg)
    model.load_state_dict(O.init_state_dict(0.33, 0.5, 80, seed=seed))
    return model


def _tensors(c, out):
    """the torch tensors a symbolic command reads or writes"""
    def add(o):
        o = getattr(o, "obj", o)
        if isinstance(o, torch.Tensor) and o.device.type == "cuda":
            out[id(o)] = o
        elif isinstance(o, dict):
            for v in o.values():
                add(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                add(v)
    for q in c.p:
        add(q)
    if c.desc is not None:
        for v in c.desc.__dict__.values():
            add(v)
        bn = getattr(c.desc, "xf_bn", None)
        if bn is not None:
            _tensors(bn, out)
    return out


def _bufs(members, by_id):
    ids = set()
    for m in members:
        ids |= Plan._cmd_bufs(m)
        bn = getattr(m.desc, "xf_bn", None) if m.desc is not None else None
        if bn is not None:
            ids |= Plan._cmd_bufs(bn)
        for j in (getattr(m.desc, "jobs", None) or []) if m.desc is not None else []:
            d = j.get("dst")
            if d is not None and isinstance(d.obj, TRef):
                ids.add(id(d.obj.buf))
    return [by_id[i] for i in sorted(ids, key=lambda i: by_id[i].offset)]


def _launch(arr, k):
    ptr = C.cast(C.byref(arr, k * C.sizeof(L.mi_cmd)), C.POINTER(L.mi_cmd))
    L.check(L.lib().mi_cmdlist_run(ptr, 1, L.stream_ptr()), "cmd")
    torch.cuda.synchronize()


def _check_step(monkeypatch, B, H, W, training=True, env=None, seed=7, mutate=None):
    """-> (Report, per-command failing tags).  mutate = (which, pick(plan) -> k, fn(desc) -> desc): command k of that list
    runs a modified descriptor and the walk stops after it; the report then also names that command (Report.mutated)"""
    monkeypatch.setenv("MI_BN_FUSED", "1")
    for k_, v in (env or {}).items():
        monkeypatch.setenv(k_, v)
    model = _gpu_model(seed)
    model.train(training)
    ps = model.plan_for(B, H, W, training)
    plan, b = ps.plan, ps.builder
    imgs, labels = O.synth_batch(B, H, W, seed=seed + 10, max_gt=4)
    ps.image.copy_(imgs.to(DEV))
    if training:
        ps.labels.copy_(labels.to(DEV))
        ps.gw().fill_(1.0)
    torch.cuda.synchronize()
    arena = plan.arena
    a0 = arena.data_ptr()
    by_id = {id(bf): bf for bf in b.bufs}
    grad = model.params.grad

    def bview(bf):
        lo = bf.base + bf.offset - a0
        return arena[lo: lo + bf.nbytes]

    it = Interp(b)
    rep = Report()
    flagged = []
    mk = None
    if mutate is not None:
        mk = mutate[1](plan)
        rep.mutated = (plan.fwd_tags if mutate[0] == "fwd" else plan.bwd_tags)[mk]
    for which in (("fwd", "bwd") if training else ("fwd",)):
        arr, n = plan.fwd_cmds if which == "fwd" else plan.bwd_cmds
        tags = plan.fwd_tags if which == "fwd" else plan.bwd_tags
        for k in range(n):
            c = plan.cmd_objs[which][k]
            op = L.OPS[c.op]
            members = Interp.members(c)
            bufs = _bufs(members, by_id)
            tens = {}
            for m in members:
                _tensors(m, tens)
            it.reset()
            for bf in bufs:
                it.mirror(bf, bview(bf).cpu())
            for t in tens.values():
                it.T(t)
            prev, gprev = arena.clone(), grad.clone()
            saved = None
            if mutate is not None and mutate[0] == which and mk == k:
                d2 = mutate[2](L.mi_conv_desc.from_buffer_copy(plan.cmd_descs[which][k]))
                saved = arr[k].p[0]
                arr[k].p[0] = C.addressof(d2)
            _launch(arr, k)
            if saved is not None:
                arr[k].p[0] = saved
            # the fused loss backward stores the fp32 [B][A][5 + ncls] gradient only with MI_LOSS_DPREDS=1: otherwise the
            # buffer is not an output of the launch and must keep its bytes (the interpreter's LOSS_BWD member writes it)
            keep_only = op == "LOSS_BWD_FUSED" and c.p[2].obj is None
            dp0 = it.raw(b.loss["dpreds"]).clone() if keep_only else None
            it.dev_out = {id(bf): bview(bf).cpu() for bf in bufs}
            it.run(members)
            nf = len(rep.fails)
            lay = Layout(members, acc_is_workspace=op == "BN_BWD_FUSED" or (op == "BN_GROUP" and c.i[0] == 3))
            for bf in bufs:
                if keep_only and bf is b.loss["dpreds"]:
                    got = bview(bf).cpu()
                    if not torch.equal(got, dp0[: bf.nbytes]):
                        d_ = (got != dp0[: bf.nbytes]).nonzero()
                        rep.fail(tag=tags[k], op=op, buf=bf.name, kind="untouched", worst=float("inf"), nbad=int(d_.numel()),
                                 first=int(d_[0]))
                    continue
                compare_buffer(bf, bview(bf).cpu(), it.raw(bf), lay, rep, tag=tags[k], op=op, mag=it.mag.get(id(bf)))
            for t in tens.values():
                got, ref = t.detach().cpu(), it.tmap[id(t)][1]
                if torch.equal(got, ref):
                    continue
                if got.is_floating_point():
                    _f32_rule(Buf(f"tensor{tuple(t.shape)}", 0), got.view(-1), ref.view(-1), rep, tags[k], op, lay)
                else:
                    rep.fail(tag=tags[k], op=op, buf=f"tensor{tuple(t.shape)}", kind="exact", worst=float("inf"),
                             nbad=int((got != ref).sum()), first=int((got != ref).view(-1).nonzero()[0]))
            # bytes outside the command's buffers / tensors: unchanged
            diff = arena != prev
            for bf in bufs:
                lo = bf.base + bf.offset - a0
                diff[lo: lo + bf.nbytes] = False
            if bool(diff.any()):
                i = int(diff.nonzero()[0])
                rep.fail(tag=tags[k], op=op, buf="arena", kind="untouched", worst=float("inf"), nbad=int(diff.sum()),
                         first=[bf.name for bf in b.bufs if bf.base + bf.offset - a0 <= i < bf.base + bf.offset - a0 + bf.nbytes])
            gd = grad.view(torch.int32) != gprev.view(torch.int32)
            for t in tens.values():
                if t.untyped_storage().data_ptr() == grad.untyped_storage().data_ptr():
                    o = (t.data_ptr() - grad.data_ptr()) // 4
                    gd[o: o + t.numel()] = False
            if bool(gd.any()):
                rep.fail(tag=tags[k], op=op, buf="grad arena", kind="untouched", worst=float("inf"), nbad=int(gd.sum()),
                         first=int(gd.nonzero()[0]))
            if len(rep.fails) > nf:
                flagged.append(tags[k])
            if saved is not None:
                return rep, flagged
    return rep, flagged


CASES = {
    "bench_16x640x640_bnfused1": (16, 640, 640, True, {"MI_BN_FUSED": "1"}),
    "bench_16x640x640_bnfused0": (16, 640, 640, True, {"MI_BN_FUSED": "0"}),
    "2x96x128": (2, 96, 128, True, {}),
    "4x384x640": (4, 384, 640, True, {}),
    "2x96x128_bn_in_consumer": (2, 96, 128, True, {"MI_BN_IN_CONSUMER": "1"}),
    "2x96x128_fuse_bn_bwd": (2, 96, 128, True, {"MI_FUSE_BN_BWD": "1"}),
    "eval_16x640x640": (16, 640, 640, False, {}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_command_matches_the_interpreter(monkeypatch, case):
    B, H, W, training, env = CASES[case]
    t0 = time.time()
    rep, flagged = _check_step(monkeypatch, B, H, W, training, env)
    print(f"\n[{case}] {time.time() - t0:.1f} s, per-op error distribution:\n{rep.summary()}")
    for f in rep.fails:
        if f.get("bad"):
            print(f["tag"], f["buf"], "bad (n, h, w, c), device, reference:", f["bad"])
    assert not rep.fails, f"{len(flagged)} commands off: {flagged[:10]}\n{rep}"


@pytest.mark.parametrize("mut", ["cout_minus_8", "n_minus_1"])
def test_a_conv_that_writes_less_is_reported(monkeypatch, mut):
    """sensitivity: one CONV command runs a legal descriptor that writes less (Cout - 8 channels, or N - 1 images); the
    comparison must name exactly that command"""
    def pick(plan):
        cands = [k for k, c in enumerate(plan.cmd_objs["fwd"]) if L.OPS[c.op] == "CONV"
                 and getattr(c.desc, "xf", None) is None and not c.desc.flags and c.desc.Cout >= 64 and c.desc.Cout % 32 == 0]
        return cands[len(cands) // 2]

    def fn(d):
        if mut == "cout_minus_8":
            d.Cout -= 8
        else:
            d.N -= 1
        return d
    rep, flagged = _check_step(monkeypatch, 2, 96, 128, True, {}, mutate=("fwd", pick, fn))
    print(f"\n[{mut}] {rep.mutated}:\n{rep}")
    assert flagged == [rep.mutated], flagged
