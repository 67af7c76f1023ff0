"""What COCO evaluation costs at COCO-val scale, on synthetic data: the device path (COCOEvaluator: process per batch, then
evaluate) against the host restatement of cocoapi's COCOeval (tests/cocoeval_ref.py, loop form, one core) on the same data.

  bbox : 5000 images of 480 x 640, 80 categories, about 7 ground truths and 100 detections per image
  segm : 200 such images, polygon ground truth, 100 dense masks per image

Detections are jittered copies of ground truths (so matches exist at every threshold) plus background; scores are float32.
`process` is timed with HIP events around each batch of 16 images, `evaluate` by the wall clock (it ends in its one
read-back), its kernels with events around the launches; the IoU kernels are timed alone at one image's shape.  The two
sides must agree exactly - the probe asserts it - so the times are for the same numbers.

  python tools/coco_eval_probe.py [--images 5000] [--segm-images 200] [--out profiles/coco_eval_probe.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np   # noqa: E402
import torch         # noqa: E402

H, W, K = 480, 640, 80


def synth(n_images, seed):
    """-> COCO dict (octagon polygons), per image (classes int64 [100], scores float32 [100], boxes XYXY float32 [100, 4])"""
    g = np.random.default_rng(seed)
    images, anns, dets = [], [], {}
    for i in range(n_images):
        img_id = i + 1
        images.append({"id": img_id, "height": H, "width": W})
        n = int(np.clip(g.poisson(7), 0, 40))
        bw, bh = g.integers(8, 300, n), g.integers(8, 300, n)
        x, y = (g.uniform(size=n) * (W - bw)).astype(np.int64), (g.uniform(size=n) * (H - bh)).astype(np.int64)
        cat = g.integers(1, K + 1, n) if i % 3 else np.minimum(g.geometric(0.15, n), K)       # a third of the images: few, frequent categories
        for j in range(n):
            c = 0.25
            ring = [x[j] + c * bw[j], y[j], x[j] + (1 - c) * bw[j], y[j], x[j] + bw[j], y[j] + c * bh[j], x[j] + bw[j], y[j] + (1 - c) * bh[j],
                    x[j] + (1 - c) * bw[j], y[j] + bh[j], x[j] + c * bw[j], y[j] + bh[j], x[j], y[j] + (1 - c) * bh[j], x[j], y[j] + c * bh[j]]
            anns.append({"id": len(anns) + 1, "image_id": img_id, "category_id": int(cat[j]), "iscrowd": int(g.uniform() < 0.01),
                         "area": float(bw[j] * bh[j]) * (1 - 2 * c * c), "bbox": [float(x[j]), float(y[j]), float(bw[j]), float(bh[j])],
                         "segmentation": [[float(v) for v in ring]]})
        D = 100
        src = g.integers(0, max(n, 1), D)
        from_gt = (g.uniform(size=D) < 0.5) & (n > 0)
        b = np.zeros((D, 4), np.float32)
        cls = g.integers(0, K, D)
        rw, rh = g.integers(8, 200, D), g.integers(8, 200, D)
        b[:, 0], b[:, 1] = g.uniform(size=D) * (W - rw), g.uniform(size=D) * (H - rh)
        b[:, 2], b[:, 3] = b[:, 0] + rw, b[:, 1] + rh
        if n:
            jit = g.normal(0, 0.08, (D, 4)) * np.stack([bw[src], bh[src], bw[src], bh[src]], 1)
            gb = np.stack([x[src], y[src], x[src] + bw[src], y[src] + bh[src]], 1) + jit
            b[from_gt] = gb[from_gt]
            cls[from_gt] = cat[src][from_gt] - 1
        b[:, [0, 2]] = np.clip(b[:, [0, 2]], 0, W)
        b[:, [1, 3]] = np.clip(b[:, [1, 3]], 0, H)
        b[:, 2], b[:, 3] = np.maximum(b[:, 2], b[:, 0] + 1), np.maximum(b[:, 3], b[:, 1] + 1)
        dets[img_id] = (cls.astype(np.int64), g.uniform(0.01, 1, D).astype(np.float32), b)
    return {"images": images, "annotations": anns, "categories": [{"id": c + 1, "name": str(c)} for c in range(K)]}, dets


def box_masks(b):
    """device: XYXY float32 [D, 4] -> bool [D, H, W], the pixels whose index lies in [round(x0), round(x1)) x [round(y0), round(y1))"""
    r = b.round()
    yy = torch.arange(H, device=b.device).view(1, H, 1)
    xx = torch.arange(W, device=b.device).view(1, 1, W)
    return (xx >= r[:, 0].view(-1, 1, 1)) & (xx < r[:, 2].view(-1, 1, 1)) & (yy >= r[:, 1].view(-1, 1, 1)) & (yy < r[:, 3].view(-1, 1, 1))


class LazyMask:
    """the same mask on the host, rasterised when the restatement asks for it (20 000 dense masks do not fit otherwise)"""

    def __init__(self, b):
        self.r = [int(v) for v in np.round(np.asarray(b, np.float32))]

    def __array__(self, dtype=None, copy=None):
        m = np.zeros((H, W), np.uint8)
        m[self.r[1]:self.r[3], self.r[0]:self.r[2]] = 1
        return m if dtype is None else m.astype(dtype)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def run(task, dataset, dets, lines, batch=16):
    import cocoeval_ref as R
    import polygon_raster_ref as P
    from yolov7_d2_amd import evaluation as E
    from yolov7_d2_amd.d2shim import Boxes, Instances
    ev = E.COCOEvaluator(dataset, tasks=(task,))
    ev.timing = True
    ids = sorted(dets)
    dev_dets = {i: tuple(torch.from_numpy(a).cuda() for a in dets[i]) for i in ids}

    def instances(i):
        cls, sc, b = dev_dets[i]
        inst = Instances((H, W), scores=sc, pred_classes=cls)
        if task == "bbox":
            inst.pred_boxes = Boxes(b)
        else:
            inst.pred_masks = box_masks(b)
        return inst
    for warm in (True, False):
        ev.reset()
        ms = []
        for k in range(0, len(ids) if not warm else min(len(ids), 2 * batch), batch):
            chunk = ids[k:k + batch]
            outs = [{"instances": instances(i)} for i in chunk]
            torch.cuda.synchronize()
            ms.append(timed(lambda: ev.process([{"image_id": i} for i in chunk], outs))[0] / len(chunk))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.evaluate()
        t_eval = time.perf_counter() - t0
    n = len(ids)
    lines.append(f"{task}: {n} images, {len(dataset['annotations'])} ground truths, {100 * n} detections")
    lines.append(f"  device process   : {statistics.median(ms):8.3f} ms / image (median over batches of {batch}; min {min(ms):.3f}, max {max(ms):.3f}), "
                 f"{sum(ms) * batch / 1e3:.2f} s in all")
    lines.append(f"  device evaluate(): {t_eval * 1e3:8.1f} ms in all (host tables, sorts, launches, the one read-back, summarize)")
    for name, v in ev.timings[task].items():
        lines.append(f"      {name:<20s}{v:9.3f} ms")
    results = []
    for i in ids:
        cls, sc, b = dets[i]
        bb = b.copy()
        bb[:, 2] -= bb[:, 0]
        bb[:, 3] -= bb[:, 1]
        for d in range(len(cls)):
            r = {"image_id": i, "category_id": int(cls[d]) + 1, "score": float(sc[d])}
            if task == "bbox":
                r["bbox"] = bb[d].tolist()
            else:
                r["mask"] = LazyMask(b[d])
            results.append(r)
    t0 = time.perf_counter()
    ref = R.evaluate(dataset, results, task, polygon_fn=P.instance_mask)
    t_ref = time.perf_counter() - t0
    same = all(np.array_equal(ev.eval[k], ref[k]) for k in ("precision", "recall", "scores")) and np.array_equal(ev.stats[task], ref["stats"])
    dev_total = sum(ms) * batch / 1e3 + t_eval
    lines.append(f"  host restatement : {t_ref:8.2f} s in all (tests/cocoeval_ref.py, numpy loop form, 1 core of {os.cpu_count()})")
    lines.append(f"  device total {dev_total:.2f} s vs host {t_ref:.2f} s: the device path is {'FASTER' if dev_total < t_ref else 'NOT faster'} "
                 f"({t_ref / dev_total:.1f}x); arrays and stats {'EQUAL' if same else 'DIFFER'}; AP {ref['stats'][0]:.4f}")
    assert same, task


def kernels_alone(lines, iters=20):
    from yolov7_d2_amd import evaluation as E
    g = torch.Generator().manual_seed(0)
    b = torch.rand(107, 4, generator=g).cuda()
    b = torch.stack([b[:, 0] * 400, b[:, 1] * 300, b[:, 0] * 400 + 20 + b[:, 2] * 200, b[:, 1] * 300 + 20 + b[:, 3] * 150], 1)
    xywh = torch.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).double()
    crowd = torch.zeros(7, dtype=torch.uint8, device="cuda")
    masks = box_masks(b)
    lines.append(f"IoU kernels alone, one image's shape (100 detections x 7 ground truths, {H} x {W}), median of {iters}:")
    for name, fn in (("mi_coco_box_iou", lambda: E.coco_box_iou(xywh[:100], xywh[100:], crowd)),
                     ("mi_coco_mask_iou", lambda: E.coco_mask_iou(masks[:100], masks[100:], crowd))):
        fn()
        ts = [timed(fn)[0] for _ in range(iters)]
        lines.append(f"  {name:<18s}{statistics.median(ts) * 1e3:9.1f} us")
    lines.append(f"  (each with the allocation of its outputs; the mask IoU - pack, areas, pairs - reads {107 * H * W / 1e6:.1f} MB of masks once)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--segm-images", type=int, default=200)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    lines = [f"COCO evaluation probe on {torch.cuda.get_device_name(0)}: device path (COCOEvaluator) vs host restatement of cocoapi's COCOeval"]
    dataset, dets = synth(args.images, 0)
    run("bbox", dataset, dets, lines)
    dataset, dets = synth(args.segm_images, 1)
    run("segm", dataset, dets, lines)
    kernels_alone(lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
