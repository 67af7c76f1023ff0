#!/usr/bin/env python
"""bench.py — images/sec of the YOLOX-s 640x640 training step (forward + SimOTA/loss + backward +
gradient all-reduce + SGD update), bs=16/GPU, synthetic COCO-shaped data, on N MI355X of one node.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Rank 0 prints ONE JSON line (see BASELINE.json for the metric).  A plain run does only what that line's headline figure
needs: set up, warm up, time the steps, write --dump-outputs, print.  Everything else is measured with

    python bench.py --gpus 1 --steps 20 --warmup 5 --full

after the timed steps, each part in runs of its own.  Its line adds `roofline`, `value_incl_h2d`, `cpu_baseline` (and
`ddp` with --gpus N).  `roofline` describes the dominant
kernel class (the conv / wgrad class with the largest total time per step; since the head / CSP convs are grouped that is the grouped weight gradient), `cpu_baseline` the oracle
(CPU fp32 restatement of the reference path) timed on this box's host cores on a bounded sample.

    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR

also writes what the last timed step computed as DIR/<name>.npy (float32, at most 64 MB), so that two builds run with
the same arguments - identical seeded inputs and weights - can be compared output for output.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def synth_batch_device(B, H, W, seed, device, max_labels=100, num_classes=80, max_gt=20):
    """COCO-shaped synthetic batch: images U{0..255}, n_gt ~ U{1..20}, w,h ~ U[16,272]"""
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (B, 3, H, W), generator=g).float()
    labels = torch.zeros(B, max_labels, 5)
    for b in range(B):
        n = int(torch.randint(1, max_gt + 1, (1,), generator=g))
        wh = 16 + torch.rand(n, 2, generator=g) * (272 - 16)
        cx = wh[:, 0] / 2 + torch.rand(n, generator=g) * (W - wh[:, 0])
        cy = wh[:, 1] / 2 + torch.rand(n, generator=g) * (H - wh[:, 1])
        labels[b, :n, 0] = torch.randint(0, num_classes, (n,), generator=g).float()
        labels[b, :n, 1], labels[b, :n, 2] = cx, cy
        labels[b, :n, 3:5] = wh
    return images.to(device), labels.to(device)


DUMP_BUDGET = 64 << 20     # bytes: --dump-outputs writes at most this much in all


def seeded_sample(t, n, seed):
    """host float32 copy of n elements of t (flattened) at positions fixed by (numel, n, seed), in ascending order; the
    whole of t when it has at most n elements"""
    flat = t.detach().reshape(-1)
    if flat.numel() > n:
        idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(seed))[:n].sort().values
        flat = flat[idx.to(flat.device)]
    return flat.float().cpu()


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy in float32"""
    import numpy as np
    arrs = {k: np.ascontiguousarray(v.detach().float().cpu().numpy() if torch.is_tensor(v) else np.asarray(v, np.float32))
            for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrs.values())
    if total > DUMP_BUDGET:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_BUDGET} byte budget")
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrs.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)


def conv_algorithmic(d):
    """algorithmic bytes / flops of one conv_igemm launch from its descriptor (each tensor touched once)"""
    K = d.K8 * 8
    npix_out = d.N * d.gridH * d.gridW
    in_pix = d.N * d.H * d.W if d.out_stride == 1 else d.N * d.H * d.W  # dgrad-s2 classes read all of dy
    out_bytes = npix_out * d.Cout * (4 if d.flags & 2 else 2) * (2 if d.flags & 1 else 1)
    byt = in_pix * K * 2 + out_bytes + d.ntaps * K * d.CoutPad * 2
    flops = 2.0 * npix_out * d.Cout * K * d.ntaps
    return byt, flops


def _pmc_file():
    """newest committed HBM-traffic CSV (tools/gpu_pmc.sh: separate --pmc FETCH_SIZE / WRITE_SIZE passes of this same
    command, KB units, FETCH_SIZE x2 on gfx950 as MI355X_MICROARCH.md prescribes) and the commit it was taken at"""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic_pmc.csv")))
    if not files:
        return None, None
    path = files[-1]
    meta = path.replace("_hbm_traffic_pmc.csv", "_meta.json")
    commit = None
    if os.path.exists(meta):
        try:
            commit = json.load(open(meta)).get("commit")
        except Exception:
            commit = None
    return path, commit


def pmc_traffic(kernel_class):
    """fallback: HBM bytes per launch of a kernel class from the newest COMMITTED rocprofv3 PMC passes (another box,
    possibly another BatchNorm form: labelled as such in traffic_source); None when absent"""
    import csv
    path, _ = _pmc_file()
    if path is None:
        return None
    live = {}
    for r in csv.DictReader(open(path)):
        live[r["kernel"]] = (float(r["fetch_bytes_per_launch_x2corrected"]), float(r["write_bytes_per_launch"]), int(r["launches"]))
    return class_traffic(kernel_class, live, 0)


def bn_algorithmic(kind, C, npix, res=False, dres=False, dres_acc=False):
    """algorithmic bytes of one BatchNorm pass (bf16, every tensor touched once): fwd reads y (+res) writes a; reduce
    reads da, y; apply reads da, y (+old dres) writes dy (+dres); the fused backward (kind 3) touches what apply touches"""
    e = npix * C * 2
    if kind == 0:
        return e * (2 + int(res))
    if kind == 1:
        return e * 2
    return e * (3 + int(dres) * (1 + int(dres_acc)))


# the three forward / data-gradient convolution kernels (one class each: a template's <KC, BN, ...> instantiations are
# ONE family - round 2 listed them separately and no convolution class ever came out dominant)
CONV_FAMILY = {0: "conv_igemm_kernel (tile implicit GEMM: stride-2 3x3, K > 128 3x3, K = 1024 1x1, prediction convs)",
               1: "c1s_kernel (streaming 1x1, persistent, weights in registers)",
               2: "w3_kernel (weight-stationary 3x3, persistent)"}
# kernel-name substrings of a class in a rocprofv3 trace
PMC_MATCH = {"conv_igemm": ("conv_igemm",), "c1s_kernel": ("c1s_kernel",), "w3_kernel": ("w3_kernel",), "wgrad": ("wgrad",),
             "BN_ACT_FWD": ("bn_act_fwd",), "BN_BWD_REDUCE": ("bn_bwd_reduce",), "BN_BWD_APPLY": ("bn_bwd_apply",),
             "BN_BWD_FUSED": ("bn_bwd_fused",)}


def _pmc_keys(kernel_class):
    for k, v in PMC_MATCH.items():
        if kernel_class.startswith(k):
            return v, ("group" in kernel_class or "grouped" in kernel_class) if kernel_class.startswith("BN_") else None
    return None, None


def live_pmc_traffic(args):
    """HBM bytes per dispatch of every kernel of THIS command on THIS box: two rocprofv3 passes (--pmc FETCH_SIZE, then
    WRITE_SIZE: they do not fit one pass) over a short eager child run of bench.py; KB units, FETCH_SIZE x 2 on gfx950
    (MI355X_MICROARCH.md, HBM section).  -> {kernel name: (fetch bytes, write bytes, dispatches)} or None (no rocprofv3 on
    the box, or a pass failed: the committed CSV is the fallback)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if os.environ.get("MI_BENCH_LIVE_PMC", "1") == "0" or shutil.which("rocprofv3") is None:
        return None
    res = {}
    tmp = tempfile.mkdtemp(prefix="mi_pmc_", dir="/tmp")
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, ctr)
            cmd = ["rocprofv3", "--kernel-trace", "--pmc", ctr, "--output-format", "csv", "-d", out, "-o", "p", "--",
                   sys.executable, os.path.abspath(__file__), "--pmc-child", "--batch", str(args.batch), "--size", str(args.size)]
            r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=240)
            files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return None
            for row in csv.DictReader(open(files[0])):
                if row["Counter_Name"] != ctr:
                    continue
                e = res.setdefault(row["Kernel_Name"], [0.0, 0.0, 0, 0])
                v = float(row["Counter_Value"]) * 1024.0
                if ctr == "FETCH_SIZE":
                    e[0] += 2.0 * v; e[2] += 1
                else:
                    e[1] += v; e[3] += 1
        return {k: (f / max(nf, 1), w / max(nw, 1), max(nf, nw)) for k, (f, w, nf, nw) in res.items()}
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def live_kernel_trace(args):
    """in-graph duration of every dispatch of ONE replayed step on THIS box: rocprofv3 --kernel-trace (no counters) over a
    child run of this file that captures the step into hipGraphs and replays it; a step is cut at the Focus packer, the
    per-dispatch median over the replayed steps is returned in launch order -> ([(kernel name, us)], step span us) or None.
    These are the durations the step actually pays: HIP events around a command replayed alone (plan.time_cmds) carry
    2-3 us per launch that the graph does not (round 4: sum 6.2 ms against a 5.5 ms step)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if os.environ.get("MI_BENCH_LIVE_TRACE", "1") == "0" or shutil.which("rocprofv3") is None:
        return None
    tmp = tempfile.mkdtemp(prefix="mi_trace_", dir="/tmp")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--trace-child", "--batch", str(args.batch), "--size", str(args.size)]
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return None
        rows = sorted(((int(x["Start_Timestamp"]), int(x["End_Timestamp"]), x["Kernel_Name"]) for x in csv.DictReader(open(files[0]))))
        starts = [i for i, x in enumerate(rows) if "focus_pack" in x[2]]
        steps = [rows[a:b] for a, b in zip(starts[:-1], starts[1:])]
        if len(steps) < 4:
            return None
        import collections
        n = collections.Counter(len(x) for x in steps).most_common(1)[0][0]
        steps = [x for x in steps if len(x) == n][-8:]   # (the replayed ones: the eager warm-up steps come first)
        if len(steps) < 3:
            return None
        disp = []
        for i in range(n):
            d = sorted(x[i][1] - x[i][0] for x in steps)
            disp.append((steps[0][i][2], d[len(d) // 2] / 1e3))
        spans = sorted(b[0][0] - a[0][0] for a, b in zip(steps[:-1], steps[1:]))
        return disp, spans[len(spans) // 2] / 1e3
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def trace_to_commands(plan, trace):
    """walk the plan's commands and the traced dispatches of one step in launch order -> {("fwd" | "bwd", k): ms}, the SGD
    launch under ("opt", 0); None when the counts do not add up (then the HIP-event timings stay).  Dispatches per
    command: stream switches 0, the loss forward 4 (cost, dynamic-k, resolve + loss, final), the fused loss backward 2,
    the grouped weight gradient whatever is left (its grids + the split reductions), everything else 1."""
    from yolov7_d2_amd import _lib as L
    disp, _ = trace
    nd = {"STREAM": 0, "NOP": 0, "FORK": 0, "JOIN": 0, "LOSS_FWD": 4, "LOSS_BWD_FUSED": 2}
    farr, fn = plan.fwd_cmds
    barr, bn = plan.bwd_cmds
    fops = [L.OPS[farr[k].op] for k in range(fn)]
    bops = [L.OPS[barr[k].op] for k in range(bn)]
    if "FOCUS" not in fops or bops.count("WGRAD_GROUP") != 1:
        return None
    kf = fops.index("FOCUS")
    order = [("fwd", k, fops[k]) for k in range(kf, fn)] + [("bwd", k, bops[k]) for k in range(bn)] + [("opt", 0, "SGD")] + \
            [("fwd", k, fops[k]) for k in range(kf)]
    fixed = sum(nd.get(op, 1) for _, _, op in order if op != "WGRAD_GROUP")
    nwg = len(disp) - fixed
    if nwg < 1:
        return None
    out, i = {}, 0
    for which, k, op in order:
        n = nwg if op == "WGRAD_GROUP" else nd.get(op, 1)
        out[(which, k)] = sum(d[1] for d in disp[i:i + n]) * 1e-3
        i += n
    return out if i == len(disp) else None


def class_traffic(kernel_class, live, launches_per_step):
    """HBM bytes per launch (= per command) of a class from the live passes"""
    keys, grouped = _pmc_keys(kernel_class)
    if live is None or keys is None:
        return None
    sel = {k: v for k, v in live.items() if any(s in k for s in keys) and (grouped is None or ("group" in k) == grouped)}
    if kernel_class.startswith(("c1s_kernel", "w3_kernel")):
        # the last template argument is the MODE: 3 = the launches that carry their BatchNorm phase
        fused = "BatchNorm/SiLU phase" in kernel_class
        sel = {k: v for k, v in sel.items() if (", 3>(" in k) == fused}
    if not sel:
        return None
    if kernel_class.startswith("wgrad"):   # one command = one dispatch of every weight-gradient grid + the reduce grids
        return int(sum(f + w for f, w, n in sel.values()))
    n = sum(v[2] for v in sel.values())
    return int(sum((f + w) * nn for f, w, nn in sel.values()) / n) if n else None


def roofline_block(plan, iters=5, live=None, trace=None, ms_per_step=None):
    from yolov7_d2_amd import _lib as L
    groups = {}
    in_graph = trace_to_commands(plan, trace) if trace is not None else None
    for which in ("fwd", "bwd"):
        per = None
        if in_graph is None:
            tot, per = plan.time_cmds(which, iters=iters)
        descs = plan.cmd_descs[which]
        arr, n = plan.fwd_cmds if which == "fwd" else plan.bwd_cmds
        for k in range(n):
            op = L.OPS[arr[k].op]
            ms = per[k][1] if in_graph is None else in_graph[(which, k)]
            if op == "CONV":
                d = descs[k]
                name = CONV_FAMILY[L.lib().mi_conv2d_route(C.byref(d))]
                byt, fl = conv_algorithmic(d)
            elif op == "CONV_GROUP":
                meta = C.cast(arr[k].p[0], C.POINTER(L.mi_conv_group)).contents
                name = CONV_FAMILY[{-1: 1, -2: 2}.get(meta.KC, 0)]
                byt = fl = 0
                for d in descs[k]:
                    b1, f1 = conv_algorithmic(d)
                    byt += b1; fl += f1
                fused = getattr(plan.fwd_list[k], "bn_jobs", None) if which == "fwd" else None
                if fused:   # MODE 3: the BatchNorm + SiLU (+ shortcut) pass is the launch's second phase
                    name += " + BatchNorm/SiLU phase"
                    for j in fused:
                        byt += bn_algorithmic(0, j.C, j.npix, bool(j.res))
            elif op == "BN_GROUP":
                kind = arr[k].i[0]
                name, byt, fl = ("BN_ACT_FWD", "BN_BWD_REDUCE", "BN_BWD_APPLY", "BN_BWD_FUSED")[kind] + " (grouped)", 0, 0
                for j in descs[k]:
                    byt += bn_algorithmic(kind, j.C, j.npix, bool(j.res), bool(j.dres), bool(j.dres_accum))
            elif op == "BN_ACT_FWD":
                name, fl = op, 0
                byt = bn_algorithmic(0, arr[k].i[3], arr[k].l[1], arr[k].i[1] > 0)
            elif op == "BN_BWD_REDUCE":
                name, fl = op, 0
                byt = bn_algorithmic(1, arr[k].i[3], arr[k].l[0])
            elif op in ("BN_BWD_APPLY", "BN_BWD_FUSED"):
                name, fl = op, 0
                byt = bn_algorithmic(2, arr[k].i[5], arr[k].l[0], dres=arr[k].i[3] > 0, dres_acc=arr[k].i[4] > 0)
            elif op == "WGRAD":
                d = descs[k]
                name = f"wgrad2_kernel<NT={d.ntaps}>"
                npx = d.N * d.outH * d.outW
                byt = d.N * d.H * d.W * d.CinPad * 2 + npx * d.CoutPad * 2 + d.ntaps * d.CoutPad * d.CinPad * 4
                fl = 2.0 * npx * d.CoutPad * d.CinPad * d.ntaps
            elif op == "WGRAD_GROUP":
                name = "wgrad_group (all layers: wgrad2/wgrad3 grids + split reduce)"
                byt = fl = 0
                for d in descs[k]:
                    npx = d.N * d.outH * d.outW
                    byt += d.N * d.H * d.W * d.CinPad * 2 + npx * d.CoutPad * 2 + d.ntaps * d.Cout * d.Cin * 4
                    fl += 2.0 * npx * d.CoutPad * d.CinPad * d.ntaps
            else:
                name, byt, fl = op, 0, 0
            g = groups.setdefault(name, dict(ms=0.0, launches=0, bytes=0.0, flops=0.0))
            g["ms"] += ms; g["launches"] += 1; g["bytes"] += byt; g["flops"] += fl
    if in_graph is not None:
        g = groups.setdefault("SGD", dict(ms=0.0, launches=0, bytes=0.0, flops=0.0))
        g["ms"] += in_graph[("opt", 0)]; g["launches"] += 1
    total_ms = sum(g["ms"] for g in groups.values())

    def describe(name, g):
        avg_ms = g["ms"] / g["launches"]
        gbs = g["bytes"] / g["launches"] / (avg_ms * 1e-3) / 1e9
        tfs = g["flops"] / g["launches"] / (avg_ms * 1e-3) / 1e12
        # the roofline that bounds this kernel class: arithmetic intensity above the ridge (2500 TF/s / 8 TB/s = 312
        # flop/B) -> matrix cores, else HBM; both utilisations are reported
        mfma_bound = g["flops"] / max(g["bytes"], 1.0) > 2500e12 / 8000e9
        return dict(bound="mfma" if mfma_bound else "hbm", kernel=name,
                    achieved=round(tfs if mfma_bound else gbs, 1), peak=2500.0 if mfma_bound else 8000.0,
                    unit="TFLOP/s" if mfma_bound else "GB/s",
                    frac=round(tfs / 2500.0 if mfma_bound else gbs / 8000.0, 4),
                    traffic=(class_traffic(name, live, g["launches"]) if live is not None else pmc_traffic(name)),
                    avg_launch_ms=round(avg_ms, 5), launches_per_step=g["launches"],
                    algorithmic_bytes_per_launch=int(g["bytes"] / g["launches"]),
                    algorithmic_flops_per_launch=int(g["flops"] / g["launches"]), hbm_GBps=round(gbs, 1),
                    hbm_frac_of_8000=round(gbs / 8000.0, 4), mfma_tflops=round(tfs, 1),
                    mfma_frac_of_2500=round(tfs / 2500.0, 4), share_of_step_kernel_time=round(g["ms"] / total_ms, 3))

    # every class that moves tensor data competes for "dominant" (conv, wgrad AND the BatchNorm passes)
    cand = {k: v for k, v in groups.items() if v["bytes"] > 0}
    ranked = sorted(cand.items(), key=lambda kv: -kv[1]["ms"])
    rl = describe(*ranked[0])
    _, commit = _pmc_file()
    if rl["traffic"] is None:
        rl["traffic_source"] = None
    elif live is not None:
        rl["traffic_source"] = "live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this run on this box (KB units, FETCH_SIZE x2)"
    else:
        rl["traffic_source"] = "committed CSV (no rocprofv3 pass on this box): profiles/*_hbm_traffic_pmc.csv @ commit %s" % commit
    keys = ("kernel", "bound", "achieved", "unit", "frac", "avg_launch_ms", "launches_per_step",
            "share_of_step_kernel_time", "hbm_frac_of_8000", "mfma_frac_of_2500", "traffic")
    rl["top3"] = [{k: d[k] for k in keys} for d in (describe(*kv) for kv in ranked[:3])]
    # family aggregates: all forward / data-gradient convolution launches together, all BatchNorm passes together
    fam = {}
    for name, g in groups.items():
        f = ("conv fwd + dgrad (all three kernels; fused launches include their BatchNorm phase)"
             if any(name.startswith(v) for v in CONV_FAMILY.values()) else
             "BatchNorm fwd + bwd (all passes)" if name.startswith("BN_") else
             "weight gradient" if name.startswith("wgrad") else None)
        if f:
            a = fam.setdefault(f, dict(ms=0.0, launches=0, bytes=0.0, flops=0.0))
            for k in a:
                a[k] += g[k]
    rl["families"] = [dict(family=f, ms_per_step=round(a["ms"], 4), launches_per_step=a["launches"],
                           hbm_GBps=round(a["bytes"] / (a["ms"] * 1e-3) / 1e9, 1), hbm_frac_of_8000=round(a["bytes"] / (a["ms"] * 1e-3) / 8e12, 4),
                           mfma_tflops=round(a["flops"] / (a["ms"] * 1e-3) / 1e12, 1), mfma_frac_of_2500=round(a["flops"] / (a["ms"] * 1e-3) / 2.5e15, 4),
                           share_of_step_kernel_time=round(a["ms"] / total_ms, 3))
                      for f, a in sorted(fam.items(), key=lambda kv: -kv[1]["ms"])]
    rl["timing_source"] = ("in-graph: rocprofv3 --kernel-trace of the replayed hipGraph step on this box (median per dispatch over the replayed steps)"
                           if in_graph is not None else "HIP events around each command replayed alone (plan.time_cmds): ~2-3 us per launch above the in-graph duration")
    # the step as a whole against both roofs: SURVEY 8(d)'s ALGORITHMIC work (conv tensors touched once, bf16: 443.6 MB and
    # 79.35 GFLOP per image) over the measured step, next to the bytes the design as built moves (sum of every class's
    # algorithmic bytes per launch: BatchNorm as separate passes, split-K partials not counted)
    as_built = sum(g["bytes"] for g in groups.values())
    if ms_per_step:
        nimg = plan.b.conv_records[0].N
        alg_b, alg_f = 443.6e6 * nimg, 79.35e9 * nimg
        rl["whole_step"] = dict(
            algorithmic_bytes=int(alg_b), algorithmic_flops=int(alg_f), ms_per_step=round(ms_per_step, 3),
            hbm_GBps=round(alg_b / (ms_per_step * 1e-3) / 1e9, 1), hbm_frac_of_8000=round(alg_b / (ms_per_step * 1e-3) / 8e12, 4),
            mfma_tflops=round(alg_f / (ms_per_step * 1e-3) / 1e12, 1), mfma_frac_of_2500=round(alg_f / (ms_per_step * 1e-3) / 2.5e15, 4),
            as_built_bytes=int(as_built), as_built_over_algorithmic=round(as_built / alg_b, 3),
            sum_kernel_ms=round(total_ms, 3), kernel_time_over_step=round(total_ms / ms_per_step, 3))
    breakdown = {k: dict(ms=round(v["ms"], 4), launches=v["launches"],
                         GBps=round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1) if v["bytes"] and v["ms"] > 0 else None,
                         TFLOPs=round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["flops"] and v["ms"] > 0 else None)
                 for k, v in sorted(groups.items(), key=lambda kv: -kv[1]["ms"])}
    return rl, breakdown, total_ms


def yolox_roofline(args, st, ms, world):
    """--full part of the YOLOX line: the per-class roofline of the step (live rocprofv3 counter passes and a kernel trace
    of the replayed step, each in a child run of this file) -> (roofline block, per-class breakdown, kernel ms per step)"""
    live = None
    if world == 1 and os.environ.get("MI_BENCH_NO_PMC") != "1":      # (A/B scripts: tools/abn.sh skips the two counter passes)
        # counters of THIS box (the committed CSV of an earlier box is only the fallback): the child must take the
        # same BatchNorm backward form as this run
        prev = os.environ.get("MI_BN_FUSED")
        os.environ["MI_BN_FUSED"] = "1" if st["plan"].bn_fused else "0"
        live = live_pmc_traffic(args)
        if prev is None:
            os.environ.pop("MI_BN_FUSED", None)
        else:
            os.environ["MI_BN_FUSED"] = prev
    trace = live_kernel_trace(args) if (world == 1 and not args.no_graph and os.environ.get("MI_BENCH_NO_PMC") != "1") else None
    rl, breakdown, kernel_ms = roofline_block(st["plan"], live=live, trace=trace, ms_per_step=ms)
    if trace is not None and "in-graph" in rl["timing_source"]:
        rl["whole_step"]["traced_step_span_ms"] = round(trace[1] * 1e-3, 3)
        # the accounting must close: the dispatches of a step cannot add up to more than the step
        closes = kernel_ms <= 1.02 * max(ms, trace[1] * 1e-3)
        rl["whole_step"]["accounting_closes"] = bool(closes)
        if os.environ.get("MI_BENCH_STRICT") == "1":
            assert closes, (kernel_ms, ms, trace[1])
    return rl, breakdown, kernel_ms


def cpu_baseline(batch=16, size=640, steps=5):
    """CPU path timed on this box's host cores: fwd + SimOTA loss + bwd + SGD(momentum), fp32, the benchmark's batch.
    kind "reference": the reference's OWN modules loaded by path (oracle/ref_loader.py, only where /root/reference
    exists); kind "port": oracle/yolox_oracle.py (the restatement of the same path) - the GPU box has no reference
    tree.  Median of `steps` timed steps after one warm-up."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import yolox_oracle as O
    import ref_loader
    # bounded thread count: on a 256-thread host the small convs run slower oversubscribed (measured 0.008 img/s at
    # 256 threads); 32 is the count we report as `cores`
    torch.set_num_threads(min(os.cpu_count() or 1, int(os.environ.get("MI_CPU_BASELINE_THREADS", "32"))))
    imgs, labels = O.synth_batch(batch, size, size, seed=1234)
    ts = []
    if ref_loader.available():
        kind = "reference"
        model, _ = ref_loader.build_reference_yolox(0.33, 0.5, 80, seed=0)
        model.train()
        opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        for it in range(steps + 1):
            t0 = time.perf_counter()
            out = model(imgs, labels)          # (loss, iou_loss, conf_loss, cls_loss, l1_loss, num_fg)
            opt.zero_grad()
            (out[0] + out[1] + out[2] + out[3]).backward()   # detectron2 sums the whole loss dict
            opt.step()
            ts.append(time.perf_counter() - t0)
        what = "the reference's own CSPDarknet/YOLOPAFPN/YOLOXHead modules loaded by path (oracle/ref_loader.py)"
    else:
        kind = "port"
        sd = O.init_state_dict(0.33, 0.5, 80, seed=0)
        params = [v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k]
        opt = torch.optim.SGD(params, lr=0.01, momentum=0.9, weight_decay=1e-4)
        for it in range(steps + 1):
            t0 = time.perf_counter()
            res = O.train_step_losses(sd, imgs, labels)
            opt.zero_grad()
            (res[0] + res[1] + res[2] + res[3]).backward()
            opt.step()
            ts.append(time.perf_counter() - t0)
        what = "oracle/yolox_oracle.py (CPU restatement of the reference path; no reference tree on this box)"
    t = sorted(ts[1:])[len(ts[1:]) // 2]
    return dict(value=round(batch / t, 3), unit="images/sec", cores=torch.get_num_threads(), kind=kind,
                sample=f"median of {steps} timed steps after 1 warm-up, B={batch} {size}x{size} fp32 "
                       f"fwd+loss+bwd+SGD through {what}")


def h2d_inclusive(model, args, world, rank, dev):
    """the same step fed from PINNED HOST memory: a fresh uint8 batch per step (16x3x640x640 B = 19.7 MB) + labels,
    copied on a dedicated stream into a double buffer while the previous step computes (NativeTrainer.feed); the forward
    graph of each staging buffer reads the staged uint8 image directly (Focus packer).  SURVEY.md 8(d) defines the step
    as including this copy (meta_arch/yolox.py:96,183).  Same contract as the resident loop: `warmup` untimed FED steps
    (the first ones create the copy stream, the staging buffers and the staged forward graphs - round 5 timed those
    one-off costs inside a 20-step region: profiles/r06_h2d_where_the_gap_was.txt), then exactly `steps` timed ones."""
    from yolov7_d2_amd.engine import NativeTrainer
    tr = NativeTrainer(model, lr=0.01 / 64 * args.batch * world, use_graph=not args.no_graph, input_u8=True)
    host = []
    for k in range(2):
        imgs, labels = synth_batch_device(args.batch, args.size, args.size, 4321 + 7 * k + rank, "cpu")
        host.append((imgs.to(torch.uint8).pin_memory(), labels.pin_memory()))
    st = tr.load_batch(host[0][0].to(dev), host[0][1].to(dev))
    for _ in range(2):                       # eager pass, capture
        tr.step(st)
    tr.feed(st, *host[0])
    for i in range(max(args.warmup, 3)):     # fed warm-up: both staged forward graphs captured and replayed
        tr.step(st)
        tr.feed(st, *host[(i + 1) % 2])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):              # `steps` steps, `steps` host -> device copies (the one in flight at the
        tr.step(st)                          # start was enqueued above and lands under step 0's wait; the last feed's
        tr.feed(st, *host[(i + 1) % 2])      # copy completes inside the region)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
    return args.batch * world * args.steps / dt, dt / args.steps * 1e3


def detr_algorithmic_flops(B, H, W, enc=6, dec=6, Q=100, E=256, ffn=2048, nh=8, freeze_at=2):
    """ALGORITHMIC floating-point operations of one DETR-R50 training step on a padded B x 3 x H x W batch (2 per
    multiply-add; forward + data gradient + weight gradient for trainable layers, forward only for the frozen stem + res2;
    attention backward 2.5 x its forward): ResNet-50 (torchvision-style, stride in the 3x3: detr_256_6_6_torchvision.yaml),
    input_proj, 6 + 6 transformer layers, the heads.  Returns (total, {part: flops})."""
    parts = {}
    h, w = (H + 1) // 2, (W + 1) // 2
    stem = 2.0 * B * h * w * 64 * 3 * 49
    h, w = (h + 1) // 2, (w + 1) // 2
    res, cin = 0.0, 64
    frozen = stem
    for si, (nb, bc) in enumerate(((3, 64), (4, 128), (6, 256), (3, 512))):
        cout = bc * 4
        stage = 0.0
        for k in range(nb):
            stride = 2 if (k == 0 and si > 0) else 1
            ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
            f = 2.0 * B * (h * w * cin * bc + ho * wo * bc * bc * 9 + ho * wo * bc * cout)
            if k == 0:
                f += 2.0 * B * ho * wo * cin * cout
            stage += f
            h, w, cin = ho, wo, cout
        if si + 2 <= freeze_at:
            frozen += stage
        else:
            res += 3.0 * stage
    parts["resnet50 (stem + res2 frozen: forward only)"] = frozen + res
    L_ = h * w
    T = B * L_
    parts["input_proj"] = 3 * 2.0 * T * 2048 * E
    lin_e = 2.0 * T * (4 * E * E + 2 * E * ffn)
    att_e = 4.0 * B * L_ * L_ * E
    parts["encoder"] = enc * (3 * lin_e + 3.5 * att_e)
    TQ = B * Q
    lin_d = 2.0 * (TQ * (4 * E * E) + TQ * 2 * E * E + T * 2 * E * E + TQ * 2 * E * ffn)
    att_d = 4.0 * B * (Q * Q + Q * L_) * E
    parts["decoder"] = dec * (3 * lin_d + 3.5 * att_d)
    parts["heads"] = 3 * 2.0 * dec * TQ * (E * 81 + 2 * E * E + E * 4)
    return sum(parts.values()), parts


def cpu_baseline_detr(model, inputs, nimg=2, steps=2):
    """the DETR-R50 training step on the host cores through the CPU restatements (oracle/resnet_oracle.py,
    oracle/detr_net_oracle.py, oracle/detr_oracle.py - fp32 torch; the reference's own Detr needs the reference tree, which
    the GPU box does not have): `nimg` images of the bench batch, forward + Hungarian matching + set criterion on all six
    levels + backward + AdamW, median of `steps` timed steps after one warm-up.  kind "port"."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import detr_net_oracle as DN
    import detr_oracle as DO
    import resnet_oracle as R
    import torch.nn.functional as F
    torch.set_num_threads(min(os.cpu_count() or 1, int(os.environ.get("MI_CPU_BASELINE_THREADS", "32"))))
    BP = "detr.backbone.0.backbone."
    sd = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    bsd = {k[len(BP):]: v for k, v in sd.items() if k.startswith(BP)}
    train = [v.requires_grad_(True) for k, v in list(sd.items()) if v.is_floating_point() and "running" not in k and ".norm." not in k
             and not k.startswith(BP + "stem") and not k.startswith(BP + "res2")]
    opt = torch.optim.AdamW(train, lr=1e-4, weight_decay=1e-4)
    ins = inputs[:nimg]
    Hm = (max(i["image"].shape[1] for i in ins) + 31) // 32 * 32
    Wm = (max(i["image"].shape[2] for i in ins) + 31) // 32 * 32
    mean = model.pixel_mean.detach().float().cpu().reshape(3, 1, 1).clone()
    std = model.pixel_std.detach().float().cpu().reshape(3, 1, 1).clone()
    x = torch.zeros(nimg, 3, Hm, Wm)
    mask = torch.ones(nimg, Hm, Wm, dtype=torch.bool)
    targets = []
    for b, i in enumerate(ins):
        img = i["image"].detach().float().cpu()
        _, h, w = img.shape
        x[b, :, :h, :w] = (img - mean) / std
        mask[b, :h, :w] = False
        bx = i["instances"].gt_boxes.tensor.detach().float().cpu()
        cxcywh = torch.stack([(bx[:, 0] + bx[:, 2]) / 2 / w, (bx[:, 1] + bx[:, 3]) / 2 / h, (bx[:, 2] - bx[:, 0]) / w, (bx[:, 3] - bx[:, 1]) / h], 1)
        targets.append(dict(labels=i["instances"].gt_classes.detach().cpu().long(), boxes=cxcywh))
    wd = dict(loss_ce=1.0, loss_bbox=5.0, loss_giou=2.0)
    ts = []
    for it in range(steps + 1):
        t0 = time.perf_counter()
        feat = R.forward(bsd, x, stride_in_1x1=False)["res5"]
        m = F.interpolate(mask[None].float(), size=feat.shape[-2:]).to(torch.bool)[0]
        pos = DN.position_embedding_sine(m, 128)
        o = DN.detr_after_backbone(sd, feat, m, pos, nhead=8, prefix="detr.")
        lg, bxs = o["logits"], o["boxes"]
        outputs = dict(pred_logits=lg[-1], pred_boxes=bxs[-1], aux_outputs=[dict(pred_logits=a, pred_boxes=b_) for a, b_ in zip(lg[:-1], bxs[:-1])])
        losses = DO.set_criterion(outputs, targets, 80, 0.1)
        total = sum(v * wd[k.rsplit("_", 1)[0] if k[-1].isdigit() else k] for k, v in losses.items()
                    if (k.rsplit("_", 1)[0] if k[-1].isdigit() else k) in wd)
        opt.zero_grad()
        total.backward()
        opt.step()
        ts.append(time.perf_counter() - t0)
    t = sorted(ts[1:])[len(ts[1:]) // 2]
    return dict(value=round(nimg / t, 3), unit="images/sec", cores=torch.get_num_threads(), kind="port",
                sample=f"median of {steps} timed steps after 1 warm-up, {nimg} images of the bench batch (padded {Hm}x{Wm}), fp32 "
                       "fwd + matching + criterion (6 levels) + bwd + AdamW through oracle/resnet_oracle.py + detr_net_oracle.py + "
                       "detr_oracle.py (CPU restatements; the reference tree is not on this box)")


def detr_roofline(B, H_, W_, dev, ms_step):
    """--full part of --config detr: the fused attention kernels alone at the encoder shape against the 2.5 PFLOP/s dense
    bf16 peak, with and without attention dropout, and the whole step's algorithmic flops over `ms_step`"""
    # attention kernels alone, encoder self-attention shape: 20 back-to-back launches through the C-ABI between HIP events
    # on the launch stream (the autograd wrapper's Python time - ~35 us per call - is not the kernel's)
    from yolov7_d2_amd import _lib as L
    L_, E, nh = (H_ // 32) * ((W_ + 31) // 32), 256, 8
    q, k, v, go = (torch.randn(L_, B, E, device=dev).to(torch.bfloat16) for _ in range(4))
    o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
    lse, dws = (torch.empty(B, nh, L_, device=dev) for _ in range(2))
    lib, spx, scl = L.lib(), L.stream_ptr(), 1.0 / 32 ** 0.5
    fwd = lambda: L.check(lib.mi_mha_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, o.data_ptr(), lse.data_ptr(), B, nh, L_, L_, E, scl, spx), "mha_fwd")
    bwd = lambda: L.check(lib.mi_mha_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, o.data_ptr(), lse.data_ptr(), go.data_ptr(), dws.data_ptr(),
                                         dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, nh, L_, L_, E, scl, spx), "mha_bwd")
    times = []
    for fn in (fwd, bwd):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 20)
    tf, tb = times
    # the same forward as the step runs it: attention-weight dropout p = 0.1 (counter-based mask recomputed in the backward)
    fwd_d = lambda: L.check(lib.mi_mha_fwd_dropout(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, o.data_ptr(), lse.data_ptr(), B, nh, L_, L_, E,
                                                   scl, 0.1, 12345, spx), "mha_fwd_dropout")
    bwd_d = lambda: L.check(lib.mi_mha_bwd_dropout(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, o.data_ptr(), lse.data_ptr(), go.data_ptr(),
                                                   dws.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, nh, L_, L_, E, scl, 0.1, 12345, spx),
                            "mha_bwd_dropout")
    times_d = []
    for fn in (fwd_d, bwd_d):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times_d.append(e0.elapsed_time(e1) / 20)
    tfd, tbd = times_d
    fl_f = 4.0 * L_ * L_ * 32 * B * nh
    fl_b = 2.5 * fl_f          # dP, dV, dS->dQ, dK + the recomputed scores (x2: dq and dkv kernels each recompute S)
    Hp, Wp = (H_ + 63) // 64 * 64, (W_ + 63) // 64 * 64      # Detr.shape_bucket = 64: the padded tensor the step computes on
    alg, alg_parts = detr_algorithmic_flops(B, Hp, Wp)
    return {"bound": "mfma", "kernel": "mha_fwd2_kernel WITH attention dropout p=0.1, as the step runs it (encoder self-attention, L=%d, B=%d, 8 heads x 32)" % (L_, B),
            "achieved": round(fl_f / (tfd * 1e-3) / 1e12, 1), "peak": 2500.0, "unit": "TFLOP/s",
            "frac": round(fl_f / (tfd * 1e-3) / 1e12 / 2500.0, 4), "traffic": None, "avg_launch_ms": round(tfd, 4),
            "without_dropout": {"achieved": round(fl_f / (tf * 1e-3) / 1e12, 1), "frac": round(fl_f / (tf * 1e-3) / 1e12 / 2500.0, 4),
                                "avg_launch_ms": round(tf, 4)},
            "mha_bwd_with_dropout": {"achieved": round(fl_b / (tbd * 1e-3) / 1e12, 1), "unit": "TFLOP/s",
                                     "frac": round(fl_b / (tbd * 1e-3) / 1e12 / 2500.0, 4), "ms": round(tbd, 4)},
            "mha_bwd": {"achieved": round(fl_b / (tb * 1e-3) / 1e12, 1), "unit": "TFLOP/s",
                        "frac": round(fl_b / (tb * 1e-3) / 1e12 / 2500.0, 4), "ms": round(tb, 4),
                        "kernels": "mha_delta + mha_bwd_dq2 + mha_bwd_dkv2"},
            "whole_step": {"algorithmic_flops": alg, "parts_GFLOP": {k_: round(v_ / 1e9, 1) for k_, v_ in alg_parts.items()},
                           "padded_batch": [B, 3, Hp, Wp], "ms_per_step": round(ms_step, 3),
                           "mfma_tflops": round(alg / (ms_step * 1e-3) / 1e12, 1),
                           "mfma_frac_of_2500": round(alg / (ms_step * 1e-3) / 1e12 / 2500.0, 4),
                           "note": "2 flops per multiply-add; fwd + dgrad + wgrad of the trainable layers, forward only for the "
                                   "frozen stem + res2, attention backward 2.5 x forward (bench.detr_algorithmic_flops)"}}


def bench_detr(args):
    """--config detr: BASELINE.json configs[3] - DETR-R50 (6 + 6 layers, 100 queries, dropout 0.1) training step at
    800 x 1333 (the padded batch of the reference's MIN_SIZE_TRAIN 800 / MAX 1333), fwd + Hungarian matching + set
    criterion + bwd + AdamW; with --full also the MFMA utilisation of the fused attention kernels at the encoder shape
    (L = 25 x 42 = 1050 tokens) against the 2.5 PFLOP/s dense bf16 peak."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import yolov7_d2_amd as M
    from yolov7_d2_amd.d2shim import Boxes, Instances
    from yolov7_d2_amd.modeling.attention import mha_core
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    B = args.batch if args.batch != 16 else 4
    H_, W_ = 800, 1333
    model = M.build_model(M.detr_r50_cfg(device="cuda:0"))
    model.train()
    g = torch.Generator().manual_seed(1234)
    inputs = []
    for b in range(B):
        h, w = (H_, W_) if b == 0 else (H_ - 32 * (b % 3), W_ - 64 * (b % 4))      # different sizes: padding masks
        n = int(torch.randint(1, 21, (1,), generator=g))
        wh = 16 + torch.rand(n, 2, generator=g) * 256
        xy = torch.rand(n, 2, generator=g) * (torch.tensor([w, h]) - wh).clamp(min=1)
        inst = Instances((h, w), gt_boxes=Boxes(torch.cat([xy, xy + wh], 1)),
                         gt_classes=torch.randint(0, 80, (n,), generator=g))
        inputs.append(dict(image=torch.randint(0, 256, (3, h, w), generator=g).float().to(dev), instances=inst))
    params = [p for p in model.parameters() if p.requires_grad]
    graphed = not args.no_graph
    if graphed:     # the same AdamW update as ONE launch over the 235 parameter tensors (optim.MultiTensorAdamW)
        from yolov7_d2_amd.optim import MultiTensorAdamW
        opt = MultiTensorAdamW(params, lr=1e-4, weight_decay=1e-4)
    else:
        opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=1e-4)
    if graphed:
        # forward + backward + AdamW of the eager module tree as ONE hipGraph per padded batch shape (graph_step.py); the
        # host half (image padding, ground truth -> device) runs every step, outside the graph
        from yolov7_d2_amd.graph_step import GraphedTrainStep
        gstep = GraphedTrainStep(model, opt)

        def step():
            return gstep(inputs)["total"]
    else:
        def step():
            losses = model(inputs)
            total = sum(v for k, v in losses.items() if k in model.criterion.weight_dict)
            opt.zero_grad(set_to_none=True)
            total.backward()
            opt.step()
            return total

    for _ in range(max(args.warmup, 2)):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.dump_outputs:       # (before the batch-7 loop below steps the model again)
        dump_outputs(args.dump_outputs, dict(total_loss=last.reshape(1),
                                             params_sample=seeded_sample(torch.cat([p.detach().reshape(-1) for p in params]), 1 << 22, seed=1)))
    # the reference's own per-GPU batch: IMS_PER_BATCH 56 on 8 GPUs = 7 (configs/coco/detr/detr_256_6_6_torchvision.yaml:26)
    bs7 = None
    if args.full and graphed and args.batch == 16 and os.environ.get("MI_BENCH_DETR_BS7", "1") == "1":
        g7 = torch.Generator().manual_seed(4321)
        in7 = list(inputs)
        for b in range(B, 7):
            h, w = H_ - 32 * (b % 3), W_ - 64 * (b % 4)
            n = int(torch.randint(1, 21, (1,), generator=g7))
            wh = 16 + torch.rand(n, 2, generator=g7) * 256
            xy = torch.rand(n, 2, generator=g7) * (torch.tensor([w, h]) - wh).clamp(min=1)
            in7.append(dict(image=torch.randint(0, 256, (3, h, w), generator=g7).float().to(dev),
                            instances=Instances((h, w), gt_boxes=Boxes(torch.cat([xy, xy + wh], 1)), gt_classes=torch.randint(0, 80, (n,), generator=g7))))
        for _ in range(3):
            gstep(in7)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            gstep(in7)
        torch.cuda.synchronize()
        d7 = time.perf_counter() - t1
        bs7 = dict(batch=7, value=round(7 * args.steps / d7, 2), ms_per_step=round(d7 / args.steps * 1e3, 3),
                   note="the reference's per-GPU batch (IMS_PER_BATCH 56 / 8 GPUs)")
    ms_step = dt / args.steps * 1e3
    out = {
        "metric": "images/sec training, DETR-R50 800x1333", "value": round(B * args.steps / dt, 2), "unit": "images/sec",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"DETR-R50 (6+6, 100 queries, dropout 0.1, FREEZE_AT 2) bs={B}/GPU, padded batch of "
                               f"<=800x1333 images: fwd + Hungarian matcher + SetCriterion + bwd + AdamW "
                               + ("(one hipGraph per padded shape, host half outside)" if graphed else "(eager ops)"),
                   "hipgraph": graphed,
                   "final_loss": round(float(last), 4)},
    }
    if args.full:
        out["roofline"] = detr_roofline(B, H_, W_, dev, ms_step)
        if bs7 is not None:
            out["at_reference_batch"] = bs7
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_detr(model, inputs)
    print(json.dumps(out))


def _time_conv(K, Cout, N, H, W, taps, iters=20):
    """one forward convolution of the library alone (HIP events on the launch stream): (ms, flops, algorithmic bytes)"""
    from yolov7_d2_amd import _lib as L
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, H, W, K, generator=g).to(dev, torch.bfloat16)
    k = 3 if taps == 9 else 1
    w = (torch.randn(Cout, K, k, k, generator=g) / (k * K ** 0.5)).to(dev)
    img = torch.empty(taps * K * Cout, dtype=torch.bfloat16, device=dev)
    L.check(L.lib().mi_pack_conv_weight(w.data_ptr(), Cout, K, k, k, img.data_ptr(), K, Cout, None, 0, 0, L.stream_ptr()), "pack")
    y = torch.empty(N, H, W, Cout, dtype=torch.bfloat16, device=dev)
    d = L.mi_conv_desc()
    d.x, d.w, d.y, d.ldx, d.ldy = x.data_ptr(), img.data_ptr(), y.data_ptr(), K, Cout
    d.N, d.H, d.W, d.outH, d.outW, d.gridH, d.gridW = N, H, W, H, W, H, W
    d.in_stride = d.out_stride = 1
    d.K8, d.Cout, d.CoutPad, d.ntaps = K // 8, Cout, Cout, taps
    t = 0
    for r in range(k):
        for c in range(k):
            d.tap_dy[t], d.tap_dx[t], d.tap_w[t] = r - k // 2, c - k // 2, r * k + c
            t += 1
    for _ in range(3):
        L.check(L.lib().mi_conv2d(C.byref(d), L.stream_ptr()), "conv2d")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        L.check(L.lib().mi_conv2d(C.byref(d), L.stream_ptr()), "conv2d")
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, 2.0 * N * H * W * Cout * K * taps, N * H * W * (K + Cout) * 2 + taps * K * Cout * 2


def bench_sparseinst(args):
    """--config sparseinst: BASELINE.json configs[4] on ONE GPU - SparseInst-R50 (InstanceContextEncoder + GroupIAMDecoder,
    100 instance queries, FREEZE_AT 0) training step at 640 x 640: fwd + matcher + criterion (focal / dice / BCE / objectness)
    + bwd + AdamW on bitmask targets.  --full adds roofline = the decoder's 3x3 256-channel convolution stack at 80 x 80 (eight such
    layers per step: 4 instance-branch + 4 mask-branch) on the matrix cores."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import yolov7_d2_amd as M
    from yolov7_d2_amd.d2shim import Instances
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    B = args.batch if args.batch != 16 else 8
    S = args.size
    model = M.build_model(M.sparse_inst_r50_giam_cfg(device="cuda:0"))
    model.train()
    g = torch.Generator().manual_seed(1234)
    inputs = []
    yy, xx = torch.meshgrid(torch.arange(S).float(), torch.arange(S).float(), indexing="ij")
    for b in range(B):
        n = int(torch.randint(1, 11, (1,), generator=g))
        masks = torch.zeros(n, S, S)
        for k in range(n):           # random rectangles / ellipses ("bitmask GTs = random rectangles/ellipses")
            cy, cx = float(torch.rand(1, generator=g)) * S, float(torch.rand(1, generator=g)) * S
            ry, rx = 16 + float(torch.rand(1, generator=g)) * S * 0.25, 16 + float(torch.rand(1, generator=g)) * S * 0.25
            masks[k] = (((yy - cy).abs() < ry) & ((xx - cx).abs() < rx)) if k % 2 == 0 else ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) < 1)
        inst = Instances((S, S), gt_classes=torch.randint(0, 80, (n,), generator=g).to(dev), gt_masks=masks.to(dev))
        inputs.append(dict(image=torch.randint(0, 256, (3, S, S), generator=g).float().to(dev), instances=inst, height=S, width=S))
    params = [p for p in model.parameters() if p.requires_grad]
    from yolov7_d2_amd.optim import MultiTensorAdamW      # the AdamW update as ONE launch over all parameter tensors
    opt = MultiTensorAdamW(params, lr=5e-5, weight_decay=0.05)

    graphed = not args.no_graph
    if graphed:     # round 4: the criterion no longer reads the host, so the whole step is ONE captured hipGraph
        from yolov7_d2_amd.graph_step import GraphedTrainStep
        gstep = GraphedTrainStep(model, opt)

        def step():
            return gstep(inputs)["total"]
    else:
        def step():
            losses = model(inputs)
            total = sum(losses.values())
            opt.zero_grad(set_to_none=True)
            total.backward()
            opt.step()
            return total

    for _ in range(max(args.warmup, 2)):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, dict(total_loss=last.reshape(1),
                                             params_sample=seeded_sample(torch.cat([p.detach().reshape(-1) for p in params]), 1 << 22, seed=1)))
    out = {
        "metric": "images/sec training, SparseInst-R50 640x640", "value": round(B * args.steps / dt, 2), "unit": "images/sec",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"SparseInst-R50 G-IAM (100 queries, FREEZE_AT 0) bs={B}/GPU {S}x{S}: fwd + matcher + criterion + "
                               "bwd + AdamW, random rectangle / ellipse bitmask targets",
                   "hipgraph": graphed, "final_loss": round(float(last), 4)},
    }
    if args.full:
        ms, fl, byt = _time_conv(256, 256, B, S // 8, S // 8, 9)
        tf = fl / (ms * 1e-3) / 1e12
        out["roofline"] = {"bound": "mfma", "kernel": f"conv_igemm_kernel, 3x3 256->256 at {S // 8}x{S // 8}, B={B} (the decoder's eight-layer stack)",
                           "achieved": round(tf, 1), "peak": 2500.0, "unit": "TFLOP/s", "frac": round(tf / 2500.0, 4), "traffic": None,
                           "avg_launch_ms": round(ms, 4), "algorithmic_flops_per_launch": int(fl), "algorithmic_bytes_per_launch": int(byt)}
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_sparseinst(S)
    print(json.dumps(out))


def cpu_baseline_sparseinst(S, B=2, steps=2):
    """config 5 on the host cores: detectron2's ResNet-50 as restated by oracle/resnet_oracle.py (d2 is un-vendored) feeding the
    REFERENCE'S OWN InstanceContextEncoder / GroupIAMDecoder / SparseInstCriterion loaded by path where /root/reference exists
    ("reference"); without that tree only the backbone restatement can run ("port": fwd + bwd of R50 + a mean loss)."""
    import types
    import resnet_oracle as RO
    import ref_loader
    torch.set_num_threads(min(os.cpu_count() or 1, int(os.environ.get("MI_CPU_BASELINE_THREADS", "32"))))
    g = torch.Generator().manual_seed(7)
    bb = RO.R50Module(50, ("res3", "res4", "res5"))
    x = torch.randn(B, 3, S, S, generator=g)
    kind, mods, crit = "port", None, None
    if ref_loader.available():
        import yolov7_d2_amd as M
        si = ref_loader.load_sparseinst()
        cfg = M.sparse_inst_r50_giam_cfg(device="cpu")
        enc = si.encoder.InstanceContextEncoder(cfg, bb.output_shape())
        dec = si.decoder.GroupIAMDecoder(cfg)
        crit = si.loss.SparseInstCriterion(cfg, si.loss.SparseInstMatcher(cfg))
        mods, kind = (enc, dec), "reference"

        class _BM:
            def __init__(self, t): self.tensor = t
            def __len__(self): return self.tensor.shape[0]
        tg = [dict(labels=torch.randint(0, 80, (3,), generator=g), masks=_BM((torch.rand(3, S, S, generator=g) > 0.7).float())) for _ in range(B)]
    params = list(bb.parameters()) + ([p for m in mods for p in m.parameters()] if mods else [])
    opt = torch.optim.AdamW(params, lr=5e-5)
    ts = []
    for it in range(steps + 1):
        t0 = time.perf_counter()
        f = bb(x)
        if mods:
            loss = sum(crit(mods[1](mods[0](f)), tg, (S, S)).values())
        else:
            loss = sum(v.mean() for v in f.values())
        opt.zero_grad()
        loss.backward()
        opt.step()
        ts.append(time.perf_counter() - t0)
    t = sorted(ts[1:])[len(ts[1:]) // 2]
    what = ("oracle R50 restatement + the reference's own encoder / decoder / criterion by path" if kind == "reference"
            else "oracle/resnet_oracle.py backbone only (no reference tree on this box): an upper bound of the CPU rate")
    return dict(value=round(B / t, 3), unit="images/sec", cores=torch.get_num_threads(), kind=kind,
                sample=f"median of {steps} timed steps after 1 warm-up, B={B} {S}x{S} fp32 fwd+loss+bwd+AdamW through {what}")


def pmc_child(args):
    """the workload of the live counter passes: the same plan, three eager steps (graphs hide the dispatches from the
    counter collection on some ROCm builds), the BatchNorm backward form fixed to the parent's choice"""
    import yolov7_d2_amd as M
    from yolov7_d2_amd.engine import NativeTrainer
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    model = M.build_model(M.yolox_s_cfg(device="cuda:0"))
    tr = NativeTrainer(model, lr=0.01 / 64 * args.batch, use_graph=False, input_u8=True)
    imgs, labels = synth_batch_device(args.batch, args.size, args.size, 1234, torch.device("cuda", 0))
    st = tr.load_batch(imgs.to(torch.uint8), labels)
    for _ in range(3):
        tr.step(st)
    torch.cuda.synchronize()


def trace_child(args):
    """the workload of the live kernel trace: the benchmark's own step captured into hipGraphs and replayed"""
    import yolov7_d2_amd as M
    from yolov7_d2_amd.engine import NativeTrainer
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    model = M.build_model(M.yolox_s_cfg(device="cuda:0"))
    tr = NativeTrainer(model, lr=0.01 / 64 * args.batch, use_graph=True, input_u8=True)
    imgs, labels = synth_batch_device(args.batch, args.size, args.size, 1234, torch.device("cuda", 0))
    st = tr.load_batch(imgs.to(torch.uint8), labels)
    for _ in range(4 + 10):
        tr.step(st)
    torch.cuda.synchronize()


def self_launch(args):
    """`python bench.py --gpus N` with no rendezvous in the environment: re-execute this command line as N ranks of one
    node (`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free>`),
    the form the driver itself uses for N > 1.  The children inherit stdout: rank 0's JSON line is this process's line."""
    import socket
    import subprocess
    share = os.environ.get("MI_DIST_SHARE_DEVICE", "0") == "1"
    have = torch.cuda.device_count()
    if not share and have < args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus}: only {have} GPU(s) visible (MI_DIST_SHARE_DEVICE=1 "
                         "MI_DIST_BACKEND=gloo rehearses the world > 1 path on one device)")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL's peer mappings fail without it on this driver
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    rc = subprocess.call(cmd, env=env)
    if rc:
        raise SystemExit(rc)


def main():
    ap = argparse.ArgumentParser(
        formatter_class=argparse.RawDescriptionHelpFormatter,
        description="images/sec of the YOLOX-s training step (BASELINE.json: metric, configs[1]; configs[2] with --gpus N) on MI355X.",
        epilog="""BASELINE.json configs and this program:
  configs[0]  YOLOX-tiny 416x416 bs 2 "on detectron2 CPU device": NOT runnable through this product by design.  MODEL.DEVICE
              cpu constructs the model, its registry / YAML / state_dict surface (tests/test_abi_and_config.py,
              tests/test_reference_yamls.py) but forward() raises MI355Error: there is no CPU compute path (a CPU fallback
              would be a second implementation behind the same API, which the scope contract rules out).  The tiny network
              itself is covered on the HIP device against a golden of the reference's own modules
              (tests/test_gpu_widths.py, tests/golden/yolox_tiny_step_416.npz); the reference CPU path timed beside the
              GPU number is the `cpu_baseline` block of the --full line.
  configs[1]  this program's default line (N = 1).      configs[2]  --gpus 8 (one rank per GPU, RCCL).
  configs[3]  --config detr (builder-run; not the driver's metric).      configs[4]  --config sparseinst (one GPU).
`value` keeps the uint8 batch resident in HBM when the timed region starts (the task contract); SURVEY.md 8(d) defines the
step WITH the host -> device copy of the batch: that is `value_incl_h2d` (--full; fed from pinned memory, double-buffered).
A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line (value, ms_per_step, config with
the final losses).  --full adds every other measurement, each in runs of its own after the timed steps: `roofline` (live
rocprofv3 counter and trace passes), `value_incl_h2d`, `cpu_baseline`, the `ddp` block of --gpus N; for --config detr /
sparseinst their `roofline` and `cpu_baseline`, and detr's `at_reference_batch` line.""")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure everything besides the headline figure: roofline, value_incl_h2d, "
                         "cpu_baseline, ddp (--gpus N), the secondary configs' rooflines, CPU baselines and batch-7 line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-h2d", action="store_true", help="(--full) skip the host-fed (PCIe-inclusive) measurement")
    ap.add_argument("--breakdown", type=str, default="", help="(--full) write the per-kernel-class breakdown JSON here")
    ap.add_argument("--config", type=str, default="yolox", help="yolox (the headline metric) | detr (BASELINE configs[3]) | sparseinst (configs[4], one GPU)")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (float32, 64 MB at most in all): "
                         "yolox - the loss vector, the updated parameters, seeded samples of the raw head outputs and of the "
                         "gradients; detr / sparseinst - the total loss and a seeded sample of the updated parameters")
    ap.add_argument("--pmc-child", action="store_true", help="(internal) a few eager steps under rocprofv3 --pmc, no output")
    ap.add_argument("--trace-child", action="store_true", help="(internal) graph-replayed steps under rocprofv3 --kernel-trace, no output")
    args = ap.parse_args()
    if args.breakdown and not args.full:
        ap.error("--breakdown comes from the roofline measurement: it needs --full")
    if args.pmc_child:
        return pmc_child(args)
    if args.trace_child:
        return trace_child(args)
    if args.config == "detr":
        return bench_detr(args)
    if args.config == "sparseinst":
        return bench_sparseinst(args)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started bare (`python bench.py --gpus N`): become the launcher of the reference's `launch(main, num_gpus, ...)`
        # (train_det.py:78-87) - one rank per GPU under torch.distributed.run on a free local port; rank 0 prints the line
        return self_launch(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # MI_DIST_SHARE_DEVICE=1 + MI_DIST_BACKEND=gloo: a 1-GPU box rehearses the world > 1 code path (two ranks on device 0,
    # gradients exchanged through gloo's host staging) - a functional check of the schedule, not a measurement
    backend = os.environ.get("MI_DIST_BACKEND", "nccl")
    if os.environ.get("MI_DIST_SHARE_DEVICE", "0") == "1":
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE {world}"

    import yolov7_d2_amd as M
    from yolov7_d2_amd.engine import NativeTrainer

    torch.manual_seed(0)
    model = M.build_model(M.yolox_s_cfg(device=f"cuda:{local}"))
    # the batch is resident in HBM in the form the reference's data loader hands it over: uint8 [B, 3, H, W] (d2's
    # DatasetMapper); preprocess_image's .type(torch.float) (meta_arch/yolox.py:96-99) is fused into the Focus packer
    trainer = NativeTrainer(model, lr=0.01 / 64 * args.batch * world, use_graph=not args.no_graph, input_u8=True)
    imgs, labels = synth_batch_device(args.batch, args.size, args.size, 1234 + rank, dev)
    st = trainer.load_batch(imgs.to(torch.uint8), labels)

    for _ in range(max(args.warmup, 2)):   # >= 2: eager warm-up, then graph capture
        trainer.step(st)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        trainer.step(st)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
    losses = trainer.losses(st)[:4].tolist()
    if args.dump_outputs and rank == 0:
        # what the last timed step handed back, copied to the host before anything below steps this trainer again: the
        # loss vector, the updated parameter arena (fp32, ~36 MB), fixed samples of the raw head outputs and the gradients
        dump_outputs(args.dump_outputs, dict(losses=trainer.losses(st), params=trainer.params.data,
                                             head_outputs_sample=seeded_sample(st["ps"].preds(), 1 << 21, seed=1),
                                             grads_sample=seeded_sample(trainer.params.grad, 1 << 21, seed=2)))
    ms = dt / args.steps * 1e3
    value = args.batch * world * args.steps / dt

    ddp = None
    if args.full and world > 1:
        # self-explaining scaling line: the buckets, what each all-reduce costs alone, and how much of the communication
        # is NOT hidden under backward (same timed loop with the collectives skipped)
        red = st["red"]
        sizes, alone = [], []
        for (lo, hi, _) in red.buckets:
            buf = trainer.params.grad[lo:hi]
            for _ in range(2):
                dist.all_reduce(buf)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(5):
                dist.all_reduce(buf)
            torch.cuda.synchronize()
            alone.append(round((time.perf_counter() - t1) / 5 * 1e3, 4))
            sizes.append(round((hi - lo) * 4 / 1e6, 2))
        red.enabled = False
        torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            trainer.step(st)
        torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
        t_nocomm = torch.tensor([time.perf_counter() - t1], device=dev, dtype=torch.float64)
        dist.all_reduce(t_nocomm, op=dist.ReduceOp.MAX)
        red.enabled = True
        # bus bandwidth of each bucket's all-reduce alone, the NCCL-tests convention: algbw * 2 (n - 1) / n
        busbw = [round(sz * 1e6 / (t * 1e-3) * 2 * (world - 1) / world / 1e9, 2) if t > 0 else None for sz, t in zip(sizes, alone)]
        ddp = dict(ranks=world, rccl_ranks=world if backend == "nccl" else 0, busbw_GBps=busbw,
                   # which gradient-exchange schedule ran (engine.NativeTrainer: MI_DDP_OVERLAP=auto times both backward
                   # schedules with their collectives at the first capture and keeps the faster)
                   schedule=trainer.ddp_choice or dict(mode=trainer.ddp_mode, forced_by="MI_DDP_OVERLAP=" + os.environ.get("MI_DDP_OVERLAP", "")),
                   backend="nccl (RCCL over xGMI)" if backend == "nccl" else backend + " (rehearsal)", buckets_MB=sizes, bucket_allreduce_alone_ms=alone,
                   bwd_segments=len(st["segs"]), ms_per_step_without_allreduce=round(float(t_nocomm) / args.steps * 1e3, 3),
                   exposed_comm_ms=round(ms - float(t_nocomm) / args.steps * 1e3, 3))
    incl = None
    if args.full and not args.no_h2d:
        incl = h2d_inclusive(model, args, world, rank, dev)
    if rank == 0:
        out = {
            "metric": "images/sec training, YOLOX-s 640x640 bs=16/GPU", "value": round(value, 2),
            "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "synthetic",
            "config": {"workload": f"YOLOX-s CSPDarknet+PAFPN {args.size}x{args.size} bs={args.batch}/GPU: fwd + SimOTA "
                                   "loss + bwd + grad all-reduce + SGD(momentum) step, uint8 image batch + labels resident in HBM",
                       "value_definition": "inputs resident in HBM at the start of the timed region (task contract); SURVEY 8(d)'s "
                                           "step includes the host->device copy of each batch: value_incl_h2d (--full)",
                       "global_batch": args.batch * world, "parallelism": f"dp{world}",
                       "hipgraph": not args.no_graph,
                       "final_losses": [round(x, 4) for x in losses],
                       "bn_backward": dict(form="fused (one launch, grid barrier)" if st["plan"].bn_fused else "reduce + apply",
                                           selected_on_device=st["plan"].bn_fused_timing)},
        }
        if args.full:
            rl, breakdown, kernel_ms = yolox_roofline(args, st, ms, world)
            out["config"]["sum_kernel_ms_per_step"] = round(kernel_ms, 3)
            out["roofline"] = rl
            if ddp is not None:
                out["ddp"] = ddp
            if incl is not None:
                # the same step fed from pinned host memory (fresh uint8 batch per step, double-buffered, overlapped):
                # SURVEY 8(d)'s definition of the step; `value` keeps the inputs resident as the task statement prescribes
                out["value_incl_h2d"] = round(incl[0], 2)
                out["ms_per_step_incl_h2d"] = round(incl[1], 3)
            if world == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline()
                # where the reference tree is absent the live leg above can only be the restatement ("port"); the
                # REFERENCE'S OWN modules timed where that tree exists (the build container, 8 cores) are recorded under profiles/
                rec = os.path.join(ROOT, "profiles", "r04_cpu_baseline_reference.json")
                if out["cpu_baseline"]["kind"] != "reference" and os.path.exists(rec):
                    with open(rec) as f:
                        out["cpu_baseline"]["reference_recorded"] = json.load(f)
            if args.breakdown:
                with open(args.breakdown, "w") as f:
                    json.dump(breakdown, f, indent=1)
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
