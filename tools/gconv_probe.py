"""The grouped 3x3 convolution (csrc/conv_grouped.hip) beside what a user has today, torch.nn.functional.conv2d(groups = G) in
bf16 channels_last, at the 3x3 layers of RegNetX-400MF on a batch of 16 images of 640 x 640.

Shapes: the stage widths and depths are recomputed here from the design-space parameters of RegNetX-400MF (w_a 24.48, w_0 24,
w_m 2.54, group width 16, depth 22: widths 32 / 64 / 160 / 384 with 1 / 2 / 7 / 12 blocks, at 160 / 80 / 40 / 20 pixels, groups
2 / 4 / 10 / 24).  Per stage: the stride-1 layer of its later blocks and the stride-2 layer of its first block (input at twice
the resolution).

Per shape and pass - forward, data gradient, weight gradient - in the same process: the library's launch(es) through the C ABI
(weight images packed once, outside the window, as a step plan would hold them) and torch's (F.conv2d, then
aten::convolution_backward with one output asked for).  HIP events around 20 back-to-back calls, median of 7 windows, after a
warm-up of the shape.  Achieved bytes/s: the algorithmic bytes - the operand read once + the result written once (forward: x and
y, data gradient: dy and dx, weight gradient: x and dy) - over the measured time, set against the measured 6.29 TB/s copy
ceiling.  The op-level lines time torch.ops.mi355.conv2d_grouped (layout handling and the weight pack included) forward and
forward + backward against F.conv2d the same way.  Every shape and pass where the library is slower is listed at the end.

  python tools/gconv_probe.py [--out profiles/gconv_probe.txt] [--batch 16]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                        # noqa: E402
import torch.nn.functional as F     # noqa: E402

COPY_CEILING = 6.29e12      # bytes per second, measured copy rate of the MI355X


def regnet_stages(w_a=24.48, w_0=24, w_m=2.54, depth=22, group_width=16, q=8):
    """[(width, blocks, groups)] of a RegNet X type (bottleneck ratio 1): the quantised linear width rule of the design space"""
    import math
    ws = []
    for i in range(depth):
        k = round(math.log((i * w_a + w_0) / w_0) / math.log(w_m))
        ws.append(int(round(w_0 * w_m ** k / q) * q))
    stages = []
    for w in ws:
        if stages and stages[-1][0] == w:
            stages[-1][1] += 1
        else:
            stages.append([w, 1])
    out = []
    for w, d in stages:
        g = min(group_width, w)
        w = int(round(w / g) * g)          # the width becomes a multiple of the group width
        out.append((w, d, w // g))
    return out


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


def probe_shape(B, Cc, G, Hin, stride, lines, losses):
    from yolov7_d2_amd import _lib as L
    lib, sp, dev = L.lib(), L.stream_ptr(), "cuda"
    Cg = Cc // G
    H = W = Hin
    Ho = Wo = (H - 1) // stride + 1
    g = torch.Generator().manual_seed(Cc + Hin + stride)
    x = torch.randn(B, H, W, Cc, generator=g).to(dev, torch.bfloat16)
    dy = torch.randn(B, Ho, Wo, Cc, generator=g).to(dev, torch.bfloat16)
    w = (torch.randn(Cc, Cg, 3, 3, generator=g) * (2.0 / (9 * Cg)) ** 0.5).to(dev)
    y = torch.empty(B, Ho, Wo, Cc, dtype=torch.bfloat16, device=dev)
    dx = torch.empty(B, H, W, Cc, dtype=torch.bfloat16, device=dev)
    gw = torch.empty(Cc, Cg, 3, 3, device=dev)
    nimg = L.check(lib.mi_gconv_weight_image_bytes(Cc, Cg), "image bytes") // 2
    wf, wd = (torch.empty(nimg, dtype=torch.bfloat16, device=dev) for _ in range(2))
    L.check(lib.mi_gconv_pack_weight(w.data_ptr(), Cc, Cg, wf.data_ptr(), wd.data_ptr(), sp), "pack")

    def desc(**kw):
        d = L.mi_gconv_desc()
        d.N, d.H, d.W, d.Cin, d.Cout, d.G, d.kh, d.kw, d.stride, d.padding, d.dilation = B, H, W, Cc, Cc, G, 3, 3, stride, 1, 1
        d.ldx = d.ldy = Cc
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    df = desc(x=x.data_ptr(), y=y.data_ptr(), w=wf.data_ptr())
    dd = desc(x=dx.data_ptr(), y=dy.data_ptr(), w=wd.data_ptr())
    dw = desc(x=x.data_ptr(), y=dy.data_ptr(), gw=gw.data_ptr())
    ns = C.c_int32(0)
    need = L.check(lib.mi_gconv_wgrad_plan(C.byref(dw), C.byref(ns)), "plan")
    ws = torch.empty(max(int(need), 16), dtype=torch.uint8, device=dev)
    dw.ws, dw.ws_bytes = ws.data_ptr(), ws.numel()
    # torch: the same tensors as NCHW views of channels_last memory, bf16 weight
    xt, dyt, wt = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2), w.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert xt.is_contiguous(memory_format=torch.channels_last)

    def t_bwd(mask):
        return torch.ops.aten.convolution_backward(dyt, xt, wt, None, [stride, stride], [1, 1], [1, 1], False, [0, 0], G, mask)

    passes = [
        ("forward", lambda: L.check(lib.mi_gconv_fwd(C.byref(df), sp), "fwd"),
         lambda: F.conv2d(xt, wt, None, stride, 1, 1, G), x.numel() * 2 + y.numel() * 2),
        ("data gradient", lambda: L.check(lib.mi_gconv_dgrad(C.byref(dd), sp), "dgrad"),
         lambda: t_bwd([True, False, False]), dy.numel() * 2 + dx.numel() * 2),
        ("weight gradient", lambda: L.check(lib.mi_gconv_wgrad(C.byref(dw), sp), "wgrad"),
         lambda: t_bwd([False, True, False]), x.numel() * 2 + dy.numel() * 2),
    ]
    name = f"C {Cc:3d} G {G:2d} Cg {Cg} in {Hin:3d}^2 stride {stride}"
    for pname, mine, theirs, nbytes in passes:
        tm, tt = window(mine), window(theirs)
        rate = nbytes / (tm * 1e-6)
        extra = f"  ({ns.value} split partials)" if pname == "weight gradient" else ""
        lines.append(f"{name} | {pname:15s} | mi355 {tm:8.1f} us | torch {tt:8.1f} us | torch / mi355 {tt / tm:5.2f} | "
                     f"{nbytes / 1e6:7.1f} MB -> {rate / 1e12:5.2f} TB/s = {100 * rate / COPY_CEILING:4.1f} % of the copy ceiling{extra}")
        print(lines[-1], flush=True)
        if tm > tt:
            losses.append(f"{name} | {pname}: mi355 {tm:.1f} us vs torch {tt:.1f} us")
    # op level: what a module patched with ops.patch_grouped_convs runs (layout checks, weight pack, allocation included)
    from yolov7_d2_amd import ops  # noqa: F401
    wp, wtp = w.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    xa, xb = xt.detach().clone().requires_grad_(True), xt.detach().clone().requires_grad_(True)

    def op_step(fn, xin, wpar):
        xin.grad = wpar.grad = None
        fn(xin, wpar).backward(dyt)

    rows = [("op forward", lambda: torch.ops.mi355.conv2d_grouped(xt, w, None, stride, 1, G), lambda: F.conv2d(xt, wt, None, stride, 1, 1, G)),
            ("op forward + backward", lambda: op_step(lambda a, b: torch.ops.mi355.conv2d_grouped(a, b, None, stride, 1, G), xa, wp),
             lambda: op_step(lambda a, b: F.conv2d(a, b, None, stride, 1, 1, G), xb, wtp))]
    for pname, mine, theirs in rows:
        tm, tt = window(mine), window(theirs)
        lines.append(f"{name} | {pname:21s} | mi355 {tm:8.1f} us | torch {tt:8.1f} us | torch / mi355 {tt / tm:5.2f}")
        print(lines[-1], flush=True)
        if tm > tt:
            losses.append(f"{name} | {pname}: mi355 {tm:.1f} us vs torch {tt:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gconv_probe.txt"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    a = ap.parse_args()
    stages = regnet_stages()
    assert [s[0] for s in stages] == [32, 64, 160, 384] and [s[2] for s in stages] == [2, 4, 10, 24], stages
    if not torch.cuda.is_available():
        raise SystemExit("gconv_probe: no GPU - nothing is measured without one")
    lines = [f"grouped 3x3 convolution, RegNetX-400MF 3x3 layers, batch {a.batch} x {a.size}^2, bf16 NHWC; device {torch.cuda.get_device_name(0)}",
             f"stages (width, blocks, groups): {stages}", "times: median of 7 windows of 20 back-to-back calls (HIP events)", ""]
    losses = []
    res = a.size // 4               # stem stride 2, stage 1 stride 2
    for (w, d, g) in stages:
        probe_shape(a.batch, w, g, res, 1, lines, losses)          # blocks 2 .. d of the stage (stage 1 of this type has none)
        probe_shape(a.batch, w, g, res * 2, 2, lines, losses)      # the first block of the stage
        res //= 2
    lines += ["", "slower than torch (shape | pass):"] + (losses or ["  none"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-(len(losses) + 2):]))


if __name__ == "__main__":
    main()
