"""What the staged deformable convolution (csrc/deform_conv.hip + the convolution kernels' 1x1 route) costs, launch by launch,
beside the plain 3x3 convolution it replaces - and what the DCN backbone does to the captured SparseInst step.

Part 1, per launch (HIP events around 20 back-to-back launches, median of 7 such windows), at the shapes of SparseInst-R50-DCN
at bs 8, 640 x 640: res4 (256 channels, output 40 x 40) and res5 (512 channels, output 20 x 20), stride 1 and stride 2 (the
first block of each stage: input 80 x 80 resp. 40 x 40).  Offsets ~ N(0, 1.5).
  forward : mi_deform_im2col, the 1x1 GEMM over 9*C channels          | plain 3x3 forward
  backward: dcol (1x1 data gradient), gW (weight gradient on col, dy),
            mi_deform_zero_f32, mi_deform_absmax, mi_deform_col2im,
            mi_deform_dx_finish                                       | plain 3x3 data gradient, weight gradient
col2im's float-atomic traffic is DERIVED, not measured: rows * 9 taps * 4 corners * C * 4 bytes before skipped corners; the
measured time is set against it and against the chip-wide float-atomic rate (about 1.3 TB/s of added bytes).

Part 2, the captured SparseInst step (GraphedTrainStep, bs 8, 640 x 640, AdamW) in images per second: the plain R50 backbone,
DCN on res4 + res5 with the columns kept for the backward pass, and with the columns sampled again there
(MI_DEFORM_KEEP_COL=0) - same process, one model after the other, the plain backbone once more at the end.

  python tools/deform_conv_probe.py [--steps 10] [--out profiles/deform_conv_probe.txt] [--no-step]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch         # noqa: E402

ATOMIC_RATE = 1.3e12        # bytes of float atomic adds per second, chip-wide (MI355X)
B = 8


def window(fn, n=20, reps=7):
    """microseconds per call: events around n back-to-back calls, median over reps windows"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / n)
    return statistics.median(out)


def layer_times(Cc, Hin, stride, lines):
    from yolov7_d2_amd import _lib as L
    from yolov7_d2_amd.modeling.resnet import _deform_cols, _deform_geom, _tap_major
    from yolov7_d2_amd.ops import _ConvGeom
    lib, sp, dev = L.lib(), L.stream_ptr(), "cuda"
    g = torch.Generator().manual_seed(Cc + Hin + stride)
    H = W = Hin
    Ho = Wo = (H - 1) // stride + 1
    rows = B * Ho * Wo
    x = torch.randn(B, H, W, Cc, generator=g).relu().to(dev, torch.bfloat16)
    off = torch.zeros(B, Ho, Wo, 32)
    off[..., :18] = torch.randn(B, Ho, Wo, 18, generator=g) * 1.5
    off = off.to(dev, torch.bfloat16)
    w = (torch.randn(Cc, Cc, 3, 3, generator=g) * (2.0 / (9 * Cc)) ** 0.5).to(dev)
    scale, shift = torch.ones(Cc, device=dev), torch.zeros(Cc, device=dev)
    dy = torch.randn(B, Ho, Wo, Cc, generator=g).to(dev, torch.bfloat16)
    # ---- deformable, staged
    gd = _deform_geom((B, Cc, H, W), w.shape, stride)
    wf, wd = gd.pack(_tap_major(w), dgrad=True, scale=scale)
    col = _deform_cols(x, off, 32, Ho, Wo, stride)
    y = torch.empty(B, Ho, Wo, Cc, dtype=torch.bfloat16, device=dev)
    dcol = torch.empty_like(col)
    dx32 = torch.empty(B, H, W, Cc, device=dev)
    doff = torch.empty(B, Ho, Wo, 32, dtype=torch.bfloat16, device=dev)
    dx = torch.empty(B, H, W, Cc, dtype=torch.bfloat16, device=dev)
    t = {}
    t["im2col"] = window(lambda: L.check(lib.mi_deform_im2col(x.data_ptr(), Cc, off.data_ptr(), 32, col.data_ptr(), B, H, W, Cc, stride, 1, 1, sp), "im2col"))
    t["gemm 1x1 (9C)"] = window(lambda: gd.fwd(col, wf, y, bias=shift, relu=True))
    t["dcol 1x1 dgrad"] = window(lambda: gd.dgrad(dy, wd, dcol))
    t["gW wgrad(col, dy)"] = window(lambda: gd.wgrad_scaled(col, dy, scale))
    t["zero fp32 dx"] = window(lambda: L.check(lib.mi_deform_zero_f32(dx32.data_ptr(), dx32.numel(), sp), "zero"))

    gmax = torch.zeros(4, device=dev)
    gd.dgrad(dy, wd, dcol)
    t["max |dcol|"] = window(lambda: L.check(lib.mi_deform_absmax(dcol.data_ptr(), dcol.numel(), gmax.data_ptr(), sp), "absmax"))

    def col2im():       # (the sum keeps growing over the window: the time does not depend on the values)
        L.check(lib.mi_deform_col2im(dcol.data_ptr(), x.data_ptr(), Cc, off.data_ptr(), 32, dx32.data_ptr(), doff.data_ptr(),
                                     gmax.data_ptr(), B, H, W, Cc, stride, 1, 1, sp), "col2im")
    t["col2im"] = window(col2im)
    t["fp32 -> bf16 dx (+mask)"] = window(lambda: L.check(lib.mi_deform_dx_finish(dx32.data_ptr(), x.data_ptr(), Cc, dx.data_ptr(), Cc, B * H * W, Cc, sp), "finish"))
    # ---- the plain 3x3 convolution at the same shape
    gp = _ConvGeom((B, Cc, H, W), w.shape, stride, 1)
    pf, pd = gp.pack(w, dgrad=True, scale=scale)
    dxp = torch.empty(B, H, W, Cc, dtype=torch.bfloat16, device=dev)
    p = {}
    p["forward"] = window(lambda: gp.fwd(x, pf, y, bias=shift, relu=True))
    p["data gradient"] = window(lambda: gp.dgrad(dy, pd, dxp))
    p["weight gradient"] = window(lambda: gp.wgrad_scaled(x, dy, scale))
    atom = rows * 9 * 4 * Cc * 4
    fwd_d, bwd_d = t["im2col"] + t["gemm 1x1 (9C)"], sum(v for k, v in t.items() if k not in ("im2col", "gemm 1x1 (9C)"))
    lines.append(f"  C {Cc}, input {H} x {W}, stride {stride} -> output {Ho} x {Wo} ({rows} rows, col {rows * 9 * Cc * 2 / 1e6:.1f} MB)")
    for k, v in t.items():
        lines.append(f"    deformable  {k:26s} {v:9.1f} us")
    for k, v in p.items():
        lines.append(f"    plain 3x3   {k:26s} {v:9.1f} us")
    lines.append(f"    forward  deformable {fwd_d:8.1f} us vs plain {p['forward']:8.1f} us ({fwd_d / p['forward']:.2f}x);  backward deformable "
                 f"{bwd_d:8.1f} us vs plain {p['data gradient'] + p['weight gradient']:8.1f} us ({bwd_d / (p['data gradient'] + p['weight gradient']):.2f}x)")
    lines.append(f"    col2im: derived atomic traffic {atom / 1e9:.3f} GB (before skipped corners) -> {atom / ATOMIC_RATE * 1e6:.0f} us at the chip-wide "
                 f"atomic rate; measured {t['col2im']:.0f} us = {atom / (t['col2im'] * 1e-6) / 1e12:.2f} TB/s of derived bytes; "
                 f"share of the deformable backward {t['col2im'] / bwd_d:.0%}")


def si_inputs(S=640):
    from yolov7_d2_amd.d2shim import Instances
    g = torch.Generator().manual_seed(1234)
    out = []
    for _ in range(B):
        n = int(torch.randint(1, 11, (1,), generator=g))
        masks = torch.zeros(n, S, S)
        for k in range(n):
            y0, x0 = int(torch.randint(0, S - 64, (1,), generator=g)), int(torch.randint(0, S - 64, (1,), generator=g))
            hh, ww = int(torch.randint(32, S - y0, (1,), generator=g)), int(torch.randint(32, S - x0, (1,), generator=g))
            masks[k, y0:y0 + hh, x0:x0 + ww] = 1
        inst = Instances((S, S), gt_classes=torch.randint(0, 80, (n,), generator=g).cuda(), gt_masks=masks.cuda())
        out.append(dict(image=torch.randint(0, 256, (3, S, S), generator=g).float().cuda(), instances=inst, height=S, width=S))
    return out


def step_rates(steps, lines):
    import yolov7_d2_amd as M
    from yolov7_d2_amd.graph_step import GraphedTrainStep
    from yolov7_d2_amd.optim import MultiTensorAdamW
    inputs = si_inputs()

    def run(deform, keep):
        os.environ["MI_DEFORM_KEEP_COL"] = keep          # (read when the step is captured)
        torch.manual_seed(0)
        cfg = M.sparse_inst_r50_giam_cfg(device="cuda:0")
        if deform:
            cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = [False, False, True, True]
        model = M.build_model(cfg).train()
        with torch.no_grad():
            for m in model.modules():
                if hasattr(m, "conv2_offset"):
                    m.conv2_offset.weight.normal_(0, 0.01)
                    m.conv2_offset.bias.normal_(0, 0.5)
        opt = MultiTensorAdamW([p for p in model.parameters() if p.requires_grad], lr=5e-5, weight_decay=0.05)
        gs = GraphedTrainStep(model, opt)
        rates = []
        try:
            for _ in range(3):
                gs(inputs)
            torch.cuda.synchronize()
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    last = gs(inputs)["total"]
                e1.record()
                e1.synchronize()
                rates.append(B * steps / (e0.elapsed_time(e1) * 1e-3))
                assert bool(torch.isfinite(last))
        finally:
            gs.close()
            os.environ.pop("MI_DEFORM_KEEP_COL", None)
        return rates

    lines.append(f"captured SparseInst step, bs {B}, 640 x 640, AdamW: images/s, 3 windows of {steps} steps each, one model after the other")
    base = None
    for name, deform, keep in (("plain R50", False, "1"), ("DCN res4 + res5, columns kept", True, "1"),
                               ("DCN res4 + res5, columns re-sampled", True, "0"), ("plain R50 (again)", False, "1")):
        rates = run(deform, keep)
        med = statistics.median(rates)
        base = med if base is None else base
        lines.append(f"  {name:38s} {med:8.1f} images/s  (windows {', '.join('%.1f' % r for r in rates)}; {B / med * 1e3:.2f} ms / step, "
                     f"{(B / med - B / base) * 1e3:+.2f} ms vs plain)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--no-step", action="store_true", help="part 1 only")
    args = ap.parse_args()
    from yolov7_d2_amd import _lib as L
    L.require_device()
    lines = ["deform_conv_probe: per-launch times (HIP events around 20 back-to-back launches, median of 7 windows), bs 8"]
    for Cc, Hin, stride in ((256, 40, 1), (256, 80, 2), (512, 20, 1), (512, 40, 2)):
        layer_times(Cc, Hin, stride, lines)
    if not args.no_step:
        step_rates(args.steps, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
