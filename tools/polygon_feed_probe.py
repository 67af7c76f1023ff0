"""What INPUT.MASK_FORMAT "polygon" costs in the host half of a SparseInst step, against what a user had to do before the
device rasteriser existed: rasterise on the CPU and hand prepare_batch dense masks from host memory.

One 640 x 640 batch of 8 with COCO-like instance counts (2 - 14 per image, rings of 12 - 60 vertices, some instances of two
rings).  prepare_batch is timed two ways - its host time alone (the call returns without waiting for the device) and with
the device drained after every call:
  polygon : MASK_FORMAT "polygon", the vertices go up (a few KB) and mi_polygon_masks rasterises on the device
  dense   : MASK_FORMAT "bitmask", the same masks as uint8 tensors in host memory (M x 640 x 640 bytes per image go over PCIe);
            the CPU rasterisation itself is NOT in this time
and the rasteriser kernel's own duration is read from `rocprofv3 --kernel-trace --stats` over a child run of this file.

  python tools/polygon_feed_probe.py [--iters 30] [--out profiles/polygon_feed_probe.txt]
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

COUNTS = (3, 12, 5, 7, 2, 9, 6, 14)
H = W = 640


def coco_like(seed=0):
    """per image a list of instances: wobbly closed outlines of 12 - 60 vertices, radius 15 - 160 px, partly off the image"""
    rng = np.random.default_rng(seed)
    out = []
    for n in COUNTS:
        insts = []
        for i in range(n):
            rings = []
            for _ in range(2 if i % 5 == 4 else 1):
                k = int(rng.integers(12, 61))
                ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, k))
                rad = rng.uniform(15.0, 160.0) * rng.uniform(0.7, 1.3, k)
                cx, cy = rng.uniform(0.0, W), rng.uniform(0.0, H)
                xy = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
                rings.append(np.round(xy, 2).reshape(-1))
            insts.append(rings)
        out.append(insts)
    return out


def child(iters):
    """the rasteriser alone, for the kernel trace"""
    from yolov7_d2_amd import ops
    polys = coco_like()
    for _ in range(iters):
        ops.polygon_masks_batch(polys, [(H, W)] * len(polys), "cuda")
    torch.cuda.synchronize()


def kernel_time(iters):
    tmp = tempfile.mkdtemp(prefix="poly_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "poly", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--iters", str(iters)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return None, f"rocprofv3 failed (rc {r.returncode}): {r.stderr[-400:]}"
    us = [(int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3 for row in csv.DictReader(open(files[0]))
          if "polygon_masks_kernel" in row["Kernel_Name"]]
    stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    line = ""
    if stats:
        line = "".join(l for l in open(stats[0]) if "polygon_masks_kernel" in l or l.startswith('"Name"')).strip()
    return us, line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if args.child:
        return child(args.iters)
    import yolov7_d2_amd as M
    from yolov7_d2_amd import ops
    from yolov7_d2_amd.d2shim import Instances
    torch.manual_seed(0)
    cfg = M.sparse_inst_r50_giam_cfg(device="cuda")
    cfg.INPUT.MASK_FORMAT = "polygon"
    model = M.build_model(cfg)
    model.train()
    polys = coco_like()
    dense = [m.cpu() for m in ops.polygon_masks_batch(polys, [(H, W)] * len(polys), "cuda")]
    gen = torch.Generator().manual_seed(0)
    images = [torch.randint(0, 256, (3, H, W), generator=gen, dtype=torch.uint8).cuda() for _ in COUNTS]
    classes = [torch.randint(0, 80, (n,), generator=gen) for n in COUNTS]
    batch = {"polygon": [dict(image=im, instances=Instances((H, W), gt_classes=c, gt_masks=p)) for im, c, p in zip(images, classes, polys)],
             "bitmask": [dict(image=im, instances=Instances((H, W), gt_classes=c, gt_masks=d)) for im, c, d in zip(images, classes, dense)]}
    lines = [f"polygon_feed_probe: batch {len(COUNTS)} x {H} x {W}, instances per image {COUNTS} ({sum(COUNTS)} masks = "
             f"{sum(COUNTS) * H * W / 1e6:.1f} MB dense, {sum(r.nbytes for i in polys for inst in i for r in inst) / 1e3:.1f} KB of vertices), "
             f"{args.iters} calls each, medians"]
    res = {}
    for fmt in ("polygon", "bitmask"):
        model.mask_format = fmt
        st = model.prepare_batch(batch[fmt])
        for _ in range(3):
            model.prepare_batch(batch[fmt], static=st)
        torch.cuda.synchronize()
        host, full = [], []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            model.prepare_batch(batch[fmt], static=st)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host.append((t1 - t0) * 1e3)
            full.append((t2 - t0) * 1e3)
        res[fmt] = (statistics.median(host), statistics.median(full))
        name = "polygon (rasterised on the device)" if fmt == "polygon" else "dense   (uint8 masks from host memory)"
        lines.append(f"  prepare_batch, {name}: host {res[fmt][0]:7.3f} ms   host + device drained {res[fmt][1]:7.3f} ms")
    us, stat = kernel_time(10)
    if us is None:
        lines.append(f"  polygon_masks_kernel: no trace - {stat}")
    else:
        lines.append(f"  polygon_masks_kernel (rocprofv3 --kernel-trace --stats, {len(us)} dispatches): median {statistics.median(us):.1f} us, "
                     f"min {min(us):.1f} us, max {max(us):.1f} us")
        if stat:
            lines.append("  " + stat.replace("\n", "\n  "))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
