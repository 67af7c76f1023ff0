"""The fused BatchNorm + ReLU block tail (csrc/bn_relu.hip) beside its composition from the launches that existed before it, the
statistics pass behind the grouped 3x3 convolution, and the captured DETR step on RegNetX-400MF beside DETR-R50 - at DETR's
batch of 4 images of 800 x 1333.

Shapes: the four stage outputs of RegNetX-400MF (widths 32 / 64 / 160 / 384 at strides 4 / 8 / 16 / 32: 200 x 334, 100 x 167,
50 x 84 and 25 x 42 pixels per image).

1. Block tail, forward and backward, projection form (two norms) and identity form (plain residual).  A = the fused launches
   (mi_bn_relu_fwd; mi_bn_relu_bwd_reduce + _apply).  B = the composition: mi_bn_act_fwd(act 0) on the projection,
   mi_bn_act_fwd(act 0, res) on c, mi_ew_bf16 ReLU; backward mi_ew_bf16 ReLU' then mi_bn_act_bwd_reduce + _apply per norm.  Same
   process, same tensors, windows INTERLEAVED (A, B, A, B ...): HIP events around 20 back-to-back calls, median of 7 windows per
   side, after a warm-up of the shape.  Bytes/s: the tensors the fused form must move (forward 3 maps; backward 10 maps for the
   projection form, 7 for the identity form whose dres is overwritten: reduce stores dz there) over the measured time, against
   the 6.29 TB/s copy ceiling of profiles/gconv_probe.txt.  The accumulators are zeroed inside the timed call on both sides (one small memset each).
2. mi_bn_stats against the mi_gconv_fwd it follows (stride-1 layer of each stage).
3. The captured training step (GraphedTrainStep, MultiTensorAdamW) of DETR on RegNetX-400MF and on R50, same process, same
   batch: images/s from a host clock around 20 replays that end in a device synchronise.

  python tools/regnet_probe.py [--out profiles/regnet_probe.txt] [--no-detr]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                        # noqa: E402

COPY_CEILING = 6.29e12      # bytes per second, measured copy rate of the MI355X (profiles/gconv_probe.txt)
BATCH, HEIGHT, WIDTH = 4, 800, 1333
STAGES = [(32, 4, 2), (64, 8, 4), (160, 16, 10), (384, 32, 24)]      # (width, stride, groups) of RegNetX-400MF


def windows(fns, n=20, reps=7):
    """microseconds per call of each fn: events around n back-to-back calls, the fns' windows interleaved, median over reps"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            out[i].append(e0.elapsed_time(e1) * 1e3 / n)
    return [statistics.median(o) for o in out]


def rate(nbytes, us):
    r = nbytes / (us * 1e-6)
    return f"{nbytes / 1e6:7.1f} MB -> {r / 1e12:5.2f} TB/s = {100 * r / COPY_CEILING:4.1f} % of the copy ceiling"


def probe_tail(Cc, stride, lines, slower):
    from yolov7_d2_amd import _lib as L
    lib, sp, dev = L.lib(), L.stream_ptr(), "cuda"
    H, W = -(-HEIGHT // stride), -(-WIDTH // stride)
    npix = BATCH * H * W
    CA = (Cc + 31) // 32 * 32
    g = torch.Generator().manual_seed(Cc)
    bf = lambda: torch.randn(npix, Cc, generator=g).to(dev, torch.bfloat16)
    f32 = lambda v=None: (torch.rand(Cc, generator=g) + 0.5).to(dev) if v is None else torch.full((Cc,), v, device=dev)
    yc, yp, x, da = bf(), bf(), bf(), bf()
    out, t1, t2, dz, dyc, dyp, dres = (torch.empty(npix, Cc, dtype=torch.bfloat16, device=dev) for _ in range(7))
    gam = [f32(), f32()]
    bet = [f32(0.1), f32(-0.1)]
    stat = [torch.empty(4, Cc, device=dev) for _ in range(2)]
    dg, db = [torch.empty(Cc, device=dev) for _ in range(2)], [torch.empty(Cc, device=dev) for _ in range(2)]
    acc = [torch.zeros(L.MI_BN_SLOTS * CA * 2, dtype=torch.float64, device=dev) for _ in range(2)]
    dacc = [torch.zeros(L.MI_BN_SLOTS * CA * 2, dtype=torch.float64, device=dev) for _ in range(2)]
    for a, y in zip(acc, (yc, yp)):
        L.check(lib.mi_bn_stats(y.data_ptr(), Cc, npix, Cc, a.data_ptr(), L.MI_BN_SLOTS, sp), "mi_bn_stats")

    def desc(two):
        d = L.mi_bn_relu_desc()
        for k, (n, y, dy) in enumerate(((d.n1, yc, dyc), (d.n2, yp, dyp))[: 2 if two else 1]):
            n.y, n.ldy, n.acc, n.nslots, n.count = y.data_ptr(), Cc, acc[k].data_ptr(), L.MI_BN_SLOTS, npix
            n.gamma, n.beta, n.eps, n.momentum = gam[k].data_ptr(), bet[k].data_ptr(), 1e-5, 0.1
            n.scale, n.shift, n.mean, n.invstd = (stat[k][i].data_ptr() for i in range(4))
            n.dacc, n.dy, n.lddy, n.dgamma, n.dbeta = dacc[k].data_ptr(), dy.data_ptr(), Cc, dg[k].data_ptr(), db[k].data_ptr()
        if not two:
            d.res, d.ldres, d.dres, d.lddres = x.data_ptr(), Cc, dres.data_ptr(), Cc
        d.a, d.lda, d.da, d.ldda, d.npix, d.C, d.relu = out.data_ptr(), Cc, da.data_ptr(), Cc, npix, Cc, 1
        return d

    def bn_fwd(k, y, res, o):
        L.check(lib.mi_bn_act_fwd(y.data_ptr(), Cc, acc[k].data_ptr(), L.MI_BN_SLOTS, npix, gam[k].data_ptr(), bet[k].data_ptr(), 1e-5,
                                  0.1, None, None, None, stat[k][0].data_ptr(), stat[k][1].data_ptr(), stat[k][2].data_ptr(),
                                  stat[k][3].data_ptr(), None if res is None else res.data_ptr(), Cc, o.data_ptr(), Cc, npix, Cc, 0,
                                  sp), "mi_bn_act_fwd")

    nblk = max(1, min(1024, -(-npix // (256 // (Cc // 8)) // 4)))

    def bn_bwd(k, y, dy, dres_):
        dacc[k].zero_()
        st = stat[k]
        L.check(lib.mi_bn_act_bwd_reduce(dz.data_ptr(), Cc, y.data_ptr(), Cc, st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
                                         st[3].data_ptr(), dacc[k].data_ptr(), L.MI_BN_SLOTS, nblk, npix, Cc, 0, sp), "bwd_reduce")
        L.check(lib.mi_bn_act_bwd_apply(dz.data_ptr(), Cc, y.data_ptr(), Cc, st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
                                        st[3].data_ptr(), gam[k].data_ptr(), dacc[k].data_ptr(), L.MI_BN_SLOTS, npix, dg[k].data_ptr(),
                                        db[k].data_ptr(), dy.data_ptr(), Cc, None, 0, 0, npix, Cc, 0, sp), "bwd_apply")

    for two, form in ((True, "projection"), (False, "identity  ")):
        d = desc(two)

        def fused_fwd():
            L.check(lib.mi_bn_relu_fwd(C.byref(d), sp), "mi_bn_relu_fwd")

        def comp_fwd():
            if two:
                bn_fwd(1, yp, None, t1)
                bn_fwd(0, yc, t1, t2)
            else:
                bn_fwd(0, yc, x, t2)
            L.check(lib.mi_ew_bf16(t2.data_ptr(), None, out.data_ptr(), t2.numel(), 1, sp), "relu")

        def fused_bwd():
            dacc[0].zero_()
            if two:
                dacc[1].zero_()
            L.check(lib.mi_bn_relu_bwd_reduce(C.byref(d), sp), "reduce")
            L.check(lib.mi_bn_relu_bwd_apply(C.byref(d), sp), "apply")

        def comp_bwd():
            L.check(lib.mi_ew_bf16(da.data_ptr(), out.data_ptr(), dz.data_ptr(), da.numel(), 2, sp), "relu'")
            bn_bwd(0, yc, dyc, None)          # (identity form: dz itself is the residual's gradient)
            if two:
                bn_bwd(1, yp, dyp, None)

        fused_fwd()
        maps = yc.numel() * 2
        for pname, a_fn, b_fn, nmaps in (("forward ", fused_fwd, comp_fwd, 3), ("backward", fused_bwd, comp_bwd, 10 if two else 7)):
            ta, tb = windows([a_fn, b_fn])
            name = f"C {Cc:3d} {H:3d} x {W:3d} | tail {form} {pname}"
            lines.append(f"{name} | fused {ta:7.1f} us | composed {tb:7.1f} us | composed / fused {tb / ta:5.2f} | {rate(nmaps * maps, ta)}")
            print(lines[-1], flush=True)
            if ta > tb:
                slower.append(f"{name}: fused {ta:.1f} us vs composed {tb:.1f} us")


def probe_stats(Cc, stride, G, lines):
    from yolov7_d2_amd import _lib as L
    lib, sp, dev = L.lib(), L.stream_ptr(), "cuda"
    H, W = -(-HEIGHT // stride), -(-WIDTH // stride)
    npix = BATCH * H * W
    Cg = Cc // G
    g = torch.Generator().manual_seed(Cc + 1)
    x = torch.randn(BATCH, H, W, Cc, generator=g).to(dev, torch.bfloat16)
    y = torch.empty_like(x)
    w = (torch.randn(Cc, Cg, 3, 3, generator=g) * (2.0 / (9 * Cg)) ** 0.5).to(dev)
    nimg = L.check(lib.mi_gconv_weight_image_bytes(Cc, Cg), "image bytes") // 2
    wf = torch.empty(nimg, dtype=torch.bfloat16, device=dev)
    L.check(lib.mi_gconv_pack_weight(w.data_ptr(), Cc, Cg, wf.data_ptr(), None, sp), "pack")
    d = L.mi_gconv_desc()
    d.N, d.H, d.W, d.Cin, d.Cout, d.G, d.kh, d.kw, d.stride, d.padding, d.dilation = BATCH, H, W, Cc, Cc, G, 3, 3, 1, 1, 1
    d.ldx = d.ldy = Cc
    d.x, d.y, d.w = x.data_ptr(), y.data_ptr(), wf.data_ptr()
    acc = torch.zeros(L.MI_BN_SLOTS * ((Cc + 31) // 32 * 32) * 2, dtype=torch.float64, device=dev)
    tc, ts = windows([lambda: L.check(lib.mi_gconv_fwd(C.byref(d), sp), "gconv"),
                      lambda: L.check(lib.mi_bn_stats(y.data_ptr(), Cc, npix, Cc, acc.data_ptr(), L.MI_BN_SLOTS, sp), "stats")])
    lines.append(f"C {Cc:3d} {H:3d} x {W:3d} G {G:2d} | mi_gconv_fwd {tc:7.1f} us | mi_bn_stats {ts:7.1f} us = {100 * ts / tc:5.1f} % of it | "
                 f"{rate(y.numel() * 2, ts)}")
    print(lines[-1], flush=True)


def probe_detr(lines):
    import yolov7_d2_amd as M
    from yolov7_d2_amd.d2shim import Boxes, Instances
    from yolov7_d2_amd.graph_step import GraphedTrainStep
    from yolov7_d2_amd.optim import MultiTensorAdamW
    g = torch.Generator().manual_seed(0)
    batch = []
    for _ in range(BATCH):
        n = 8
        wh = 32 + torch.rand(n, 2, generator=g) * 300
        xy = torch.rand(n, 2, generator=g) * (torch.tensor([WIDTH, HEIGHT]) - wh)
        inst = Instances((HEIGHT, WIDTH), gt_boxes=Boxes(torch.cat([xy, xy + wh], 1)), gt_classes=torch.randint(0, 80, (n,), generator=g))
        batch.append(dict(image=torch.randint(0, 256, (3, HEIGHT, WIDTH), generator=g).float().cuda(), instances=inst))
    for name, setup in (("RegNetX-400MF", lambda c: c.merge_from_list(["MODEL.BACKBONE.NAME", "build_regnet_backbone",
                                                                         "MODEL.REGNETS.TYPE", "RegNetX_400MF"])),
                        ("R50          ", lambda c: None)):
        cfg = M.detr_r50_cfg(device="cuda")
        setup(cfg)
        torch.manual_seed(1)
        model = M.build_model(cfg).train()
        opt = MultiTensorAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-4)
        step = GraphedTrainStep(model, opt)
        try:
            for _ in range(3):
                step(batch)
            torch.cuda.synchronize()
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                for _ in range(20):
                    out = step(batch)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) / 20)
            t = statistics.median(times)
            lines.append(f"captured DETR step, backbone {name} | batch {BATCH} x {HEIGHT} x {WIDTH} | {t * 1e3:7.2f} ms per step | "
                         f"{BATCH / t:6.1f} images/s | total loss {float(out['total']) if 'total' in out else float('nan'):.3f}")
            print(lines[-1], flush=True)
        finally:
            step.close()
        del model, opt, step
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regnet_probe.txt"))
    ap.add_argument("--no-detr", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regnet_probe: no GPU - nothing is measured without one")
    lines = [f"RegNet block tail, statistics pass and DETR step; batch {BATCH} x {HEIGHT} x {WIDTH}, bf16 NHWC; device {torch.cuda.get_device_name(0)}",
             "kernel times: median of 7 interleaved windows of 20 back-to-back calls (HIP events)", ""]
    slower = []
    for (w, s, g) in STAGES:
        probe_tail(w, s, lines, slower)
    lines.append("")
    for (w, s, g) in STAGES:
        probe_stats(w, s, g, lines)
    lines += ["", "fused tail slower than the composition (shape | pass):"] + (["  " + s for s in slower] or ["  none"])
    lines.append("")
    if not a.no_detr:
        probe_detr(lines)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
