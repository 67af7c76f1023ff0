"""SMCADetr's two new kernels and its training step, measured on the device, one process, the forms alternating:

  postprocess  focal_topk_postprocess (mi_focal_topk_postprocess, one launch for the batch) without and with out_sizes, beside the
               torch composition of the reference's inference (smca_detr.py:216-264: sigmoid, topk, //, %, per image
               cxcywh -> xyxy, gather, Boxes.scale) and of detector_postprocess (scale, clip; the nonempty() filter needs a host
               read and is left out on both sides) on device tensors.  B 1, 4, 16; Q 300; C 80, 91; K 100.
  box tail     box_ref_sigmoid (mi_box_ref_sigmoid_fwd / _bwd) beside the slice add + repeat + mi_sigmoid_f32 (detr._SigmoidF32),
               forward and forward + backward, at L 6, B 4, Q 300.
  step         the captured training step (GraphedTrainStep, MultiTensorAdamW) of SMCADetr (smcadetr_origin.yaml's values) and of
               Detr R50, 800 x 1333 padded batch of 4, images / s.

HIP events around back-to-back calls, median of 7 windows after a warm-up.

  python tools/smcadetr_probe.py [--out profiles/smcadetr_probe.txt] [--no-step]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                        # noqa: E402


def window(fn, n=20):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / n


def interleaved(fns, reps=7):
    """median us of each of fns: their windows alternate"""
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(ts, fns):
            t.append(window(f))
    return [statistics.median(t) for t in ts]


def composition(box_cls, box_pred, image_sizes, out_sizes, k=100):
    """the reference's inference (+ detector_postprocess's scale and clip when out_sizes is given) as torch calls on the device"""
    prob = box_cls.sigmoid()
    scores, topk_indexes = torch.topk(prob.view(box_cls.shape[0], -1), k, dim=1)
    topk_boxes = torch.div(topk_indexes, box_cls.shape[2], rounding_mode="floor")
    labels = topk_indexes % box_cls.shape[2]
    res = []
    for i, (s, l, b, (h, w)) in enumerate(zip(scores, labels, box_pred, image_sizes)):
        x_c, y_c, bw, bh = b.unbind(-1)
        xyxy = torch.stack([(x_c - 0.5 * bw), (y_c - 0.5 * bh), (x_c + 0.5 * bw), (y_c + 0.5 * bh)], dim=-1)
        t = torch.gather(xyxy, 0, topk_boxes[i].unsqueeze(-1).repeat(1, 4))
        t[:, 0::2] *= w
        t[:, 1::2] *= h
        if out_sizes is not None:
            oh, ow = out_sizes[i]
            t[:, 0::2] *= ow / w
            t[:, 1::2] *= oh / h
            t = torch.stack((t[:, 0].clamp(min=0, max=ow), t[:, 1].clamp(min=0, max=oh), t[:, 2].clamp(min=0, max=ow),
                             t[:, 3].clamp(min=0, max=oh)), dim=-1)
        res.append((t, s, l))
    return res


def step_rate(kind, B=4, steps=12, warmup=3):
    import yolov7_d2_amd as M
    from yolov7_d2_amd.d2shim import Boxes, Instances
    from yolov7_d2_amd.graph_step import GraphedTrainStep
    from yolov7_d2_amd.optim import MultiTensorAdamW
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    H_, W_ = 800, 1333
    model = M.build_model(M.smca_detr_cfg(device="cuda:0") if kind == "SMCADetr" else M.detr_r50_cfg(device="cuda:0"))
    model.train()
    g = torch.Generator().manual_seed(1234)
    inputs = []
    for b in range(B):
        h, w = (H_, W_) if b == 0 else (H_ - 32 * (b % 3), W_ - 64 * (b % 4))
        n = int(torch.randint(1, 21, (1,), generator=g))
        wh = 16 + torch.rand(n, 2, generator=g) * 256
        xy = torch.rand(n, 2, generator=g) * (torch.tensor([w, h]) - wh).clamp(min=1)
        inst = Instances((h, w), gt_boxes=Boxes(torch.cat([xy, xy + wh], 1)), gt_classes=torch.randint(0, 80, (n,), generator=g))
        inputs.append(dict(image=torch.randint(0, 256, (3, h, w), generator=g).float().to(dev), instances=inst))
    opt = MultiTensorAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-4)
    gstep = GraphedTrainStep(model, opt)
    try:
        for _ in range(warmup):
            last = gstep(inputs)["total"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            last = gstep(inputs)["total"]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return B * steps / dt, dt / steps * 1e3, float(last)
    finally:
        gstep.close()
        del model, opt
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smcadetr_probe.txt"))
    ap.add_argument("--no-step", action="store_true", help="skip the two captured training steps")
    args = ap.parse_args()
    from yolov7_d2_amd import _lib as L
    from yolov7_d2_amd.modeling import box_ref_sigmoid, focal_topk_postprocess
    from yolov7_d2_amd.modeling.detr import _SigmoidF32
    dev = "cuda"
    lines = [f"SMCADetr probe; {torch.cuda.get_device_name(0)}",
             "postprocess: focal_topk_postprocess (one launch) vs the torch composition of the reference's inference (+ detector_postprocess's "
             "scale and clip with out_sizes), K 100; microseconds per call, median of 7 interleaved windows of 20 calls; x = composition / kernel",
             f"{'B':>2} {'Q':>4} {'C':>3} | {'kernel':>8} {'compos.':>9} {'x':>6} | {'kernel+out':>10} {'compos.+out':>11} {'x':>6}"]
    slower = []
    for B in (1, 4, 16):
        for C in (80, 91):
            Q = 300
            g = torch.Generator().manual_seed(B * 100 + C)
            lg = (torch.randn(B, Q, C, generator=g) * 1.5 - 4.6).to(dev)
            bx = torch.rand(B, Q, 4, generator=g).mul(0.9).add(0.05).to(dev)
            sizes = [(800 - 32 * (b % 3), 1333 - 64 * (b % 4)) for b in range(B)]
            outs = [(480 + 7 * b, 640 + 5 * b) for b in range(B)]
            sd = torch.tensor(sizes, dtype=torch.int64, device=dev)
            od = torch.tensor(outs, dtype=torch.int64, device=dev)
            tk, tc, tko, tco = interleaved([lambda: focal_topk_postprocess(lg, bx, sd), lambda: composition(lg, bx, sizes, None),
                                            lambda: focal_topk_postprocess(lg, bx, sd, od), lambda: composition(lg, bx, sizes, outs)])
            lines.append(f"{B:>2} {Q:>4} {C:>3} | {tk:>8.1f} {tc:>9.1f} {tc / tk:>6.1f} | {tko:>10.1f} {tco:>11.1f} {tco / tko:>6.1f}")
            for name, a, b_ in (("", tk, tc), (" with out_sizes", tko, tco)):
                if a > b_:
                    slower.append(f"B {B} C {C}{name}: kernel {a:.1f} us > composition {b_:.1f} us")
    lines.append("slower than the composition: " + ("; ".join(slower) if slower else "nowhere"))
    Lv, B, Q = 6, 4, 300
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(Lv, B, Q, 4, generator=g) * 2).to(dev).requires_grad_(True)
    p = torch.randn(B, Q, 2, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(Lv, B, Q, 4, generator=g).to(dev)

    def old():
        c = x + 0
        c[..., :2] = c[..., :2] + p.unsqueeze(0).repeat(Lv, 1, 1, 1)
        return _SigmoidF32.apply(c)

    tf, to, tfb, tob = interleaved([lambda: box_ref_sigmoid(x, p), old, lambda: torch.autograd.grad(box_ref_sigmoid(x, p), [x, p], dy),
                                    lambda: torch.autograd.grad(old(), [x, p], dy)])
    lines.append(f"box head tail, L {Lv} B {B} Q {Q} (us): forward fused {tf:.1f} vs slice add + repeat + mi_sigmoid_f32 {to:.1f} (x {to / tf:.1f}); "
                 f"forward + backward fused {tfb:.1f} vs {tob:.1f} (x {tob / tfb:.1f})")
    if not args.no_step:
        for kind in ("SMCADetr", "Detr"):
            ips, ms, tot = step_rate(kind)
            lines.append(f"captured training step, 800 x 1333 padded batch of 4, {kind}: {ips:.1f} images/s ({ms:.1f} ms per step; last total loss {tot:.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
