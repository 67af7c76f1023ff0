"""What the SparseInst inference postprocess costs behind the decoder: the reference's per-image loop (SparseInst.inference)
against the batched path (sparseinst_inference_batched, csrc/sparseinst_infer.hip), interleaved in one process.

Decoder-shaped random inputs: B = 8 images padded to 640 x 640, N = 100 queries, C = 80 classes, mask logits 160 x 160 as the
decoder leaves them (NHWC bf16, 128 channels), output sizes like COCO's (480 x 640 and 427 x 640 mixed), at two class
thresholds: nearly all queries kept, and about 10 per image.  Each path is timed with HIP events around one call, the two
alternating, after a warm-up; the two entry points of the batched path are also timed alone (events around the launches),
against the bytes they have to move: every mask logit once, every result byte once.

  python tools/sparseinst_infer_probe.py [--iters 30] [--out profiles/sparseinst_infer_probe.txt]
"""
import argparse
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch         # noqa: E402

B, N, C, HP, WP, HM, WM, NP = 8, 100, 80, 640, 640, 160, 160, 128
IMAGE_SIZES = [(480, 640), (427, 640), (640, 480), (640, 427), (480, 640), (427, 640), (512, 640), (640, 640)]
OUT_SIZES = [(480, 640), (427, 640), (640, 480), (640, 427), (480, 640), (427, 640), (400, 500), (333, 333)]


def decoder_like(seed=0):
    gen = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B, N, C, generator=gen) * 2.0 - 3.0).cuda()
    obj = torch.randn(B, N, 1, generator=gen).cuda()
    # smooth blobs rather than noise: masks with an inside and an outside, like a trained decoder's
    low = torch.randn(B, NP, HM // 8, WM // 8, generator=gen).cuda() * 4.0
    masks = torch.nn.functional.interpolate(low, size=(HM, WM), mode="bilinear", align_corners=False)
    nhwc = masks.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    return {"pred_logits": logits, "pred_scores": obj, "pred_masks": nhwc.permute(0, 3, 1, 2)[:, :N], "_masks_nhwc": nhwc}


def threshold_for(output, per_image):
    """the class threshold that keeps about `per_image` queries per image"""
    s = torch.sqrt(output["pred_logits"].sigmoid() * output["pred_scores"].sigmoid()).max(-1).values
    return float(s.flatten().sort(descending=True).values[min(per_image * B, B * N) - 1]) - 1e-6


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import yolov7_d2_amd as M
    from yolov7_d2_amd import _lib as L
    from yolov7_d2_amd.modeling import sparseinst as S
    output = decoder_like()
    inputs = [dict(height=h, width=w) for h, w in OUT_SIZES]
    lines = [f"sparseinst_infer_probe: B = {B}, padded {HP} x {WP}, N = {N}, masks {HM} x {WM} NHWC bf16 ({NP} channels), outputs "
             f"{sorted(set(OUT_SIZES))}, {args.iters} calls each (alternating, HIP events), medians"]
    for name, per_image in (("nearly all kept", 97), ("about 10 kept", 10)):
        thr = threshold_for(output, per_image)
        stub = types.SimpleNamespace(cls_threshold=thr, mask_threshold=0.45)
        loop = lambda: M.SparseInst.inference(stub, output, inputs, (HP, WP), IMAGE_SIZES)                 # noqa: E731
        fast = lambda: M.SparseInst.inference_batched(stub, output, inputs, (HP, WP), IMAGE_SIZES)         # noqa: E731
        for _ in range(3):
            a, b = loop(), fast()
        torch.cuda.synchronize()
        kept = [len(r.scores) for r in b]
        assert kept == [len(r.scores) for r in a]
        mism = max(float((x.pred_masks != y.pred_masks).float().mean()) for x, y in zip(a, b) if x.has("pred_masks"))
        del a, b
        t = {"loop": [], "batched": []}
        for _ in range(args.iters):
            t["loop"].append(timed(loop)[0])
            t["batched"].append(timed(fast)[0])
        out_bytes = sum(k * h * w for k, (h, w) in zip(kept, OUT_SIZES))
        lines.append(f"  {name} (cls threshold {thr:.4f}: {kept} kept, {out_bytes / 1e6:.1f} MB of masks out, mismatch share vs loop {mism:.1e})")
        for k in ("loop", "batched"):
            lines.append(f"    {k:8s} {statistics.median(t[k]):8.3f} ms / batch   (min {min(t[k]):.3f}, max {max(t[k]):.3f})")
        lines.append(f"    ratio loop / batched: {statistics.median(t['loop']) / statistics.median(t['batched']):.2f}")
        # the two entry points alone
        lib = L.lib()
        nhwc = output["_masks_nhwc"]
        v = nhwc.permute(0, 3, 1, 2)
        margs = (nhwc.data_ptr(), 1) + tuple(v.stride())
        logits, obj = output["pred_logits"].contiguous(), output["pred_scores"].reshape(B, N).contiguous()
        counts = torch.empty(B, dtype=torch.int32, device="cuda")
        keptq = torch.empty(B, N, dtype=torch.int32, device="cuda")
        scores = torch.empty(B, N, device="cuda")
        labels = torch.empty(B, N, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.mi_sparseinst_infer_ws_bytes(B, N, HM, WM) // 4, device="cuda")
        sel = lambda: L.check(lib.mi_sparseinst_infer_select(logits.data_ptr(), obj.data_ptr(), *margs, B, N, C, HM, WM, thr, 0.45,    # noqa: E731
                                                             counts.data_ptr(), keptq.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                                                             ws.data_ptr(), ws.numel() * 4, L.stream_ptr()), "select")
        sel()
        n = counts.tolist()
        descs = (L.mi_sparseinst_infer_desc * B)()
        total = 0
        for i in range(B):
            d = descs[i]
            d.out_off, d.n, (d.h_img, d.w_img), (d.Hout, d.Wout) = total, n[i], IMAGE_SIZES[i], OUT_SIZES[i]
            total += n[i] * d.Hout * d.Wout
        flat = torch.empty(total, dtype=torch.uint8, device="cuda")
        msk = lambda: L.check(lib.mi_sparseinst_infer_masks(*margs, B, N, HM, WM, HP, WP, keptq.data_ptr(), descs, 0.45,              # noqa: E731
                                                            flat.data_ptr(), total, L.stream_ptr()), "masks")
        read_all = B * HM * WM * NP * 2
        read_kept = sum(n) * HM * WM * 2
        for label, fn, nbytes, what in (("select + rescore (2 launches)", sel, read_all, "all mask logits read once"),
                                        ("resize + threshold (1 launch)", msk, read_kept + total, "kept mask logits read once + result written once")):
            for _ in range(3):
                fn()
            ms = statistics.median(timed(fn)[0] for _ in range(args.iters))
            lines.append(f"    {label}: {ms * 1e3:8.1f} us, {nbytes / 1e6:7.1f} MB ({what}) -> {nbytes / ms / 1e9:6.3f} TB/s effective")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
