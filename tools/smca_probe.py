"""Attention with SMCA's Gaussian prior (csrc/mha.hip PRIOR instantiations through modeling.smca_core) beside two baselines,
bf16 on the device, interleaved in one process:

  (i)  the dense torch composition the reference runs (smca_attention.py:179-287 after the in-projection): the dense prior
       [Lq, Lk, B heads] is BUILT from point / coef as smcadetr_backbone.py:285-310 builds it (that is part of what the fused
       form replaces), added to the [B heads, Lq, Lk] scores, softmax, dropout, x V; autograd keeps what it keeps;
  (ii) mha_core on the same q, k, v (csrc/mha.hip without the prior): what the prior costs over plain attention.

Shapes: B 4, 8 heads, 300 queries, maps 25 x 42 (800 x 1333 at stride 32) and 19 x 25, attention dropout 0 and 0.1.  Forward: one
call; backward: torch.autograd.grad of the output for q, k, v, point, coef (mha_core: q, k, v).  HIP events around 10 back-to-back
calls, median of 7 windows after a warm-up, the three forms alternating window by window.

  python tools/smca_probe.py [--out profiles/smca_probe.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                        # noqa: E402

MAPS = [(25, 42), (19, 25)]
B, HEADS, HD, LQ, SMOOTH = 4, 8, 32, 300, 8.0


def window(fn, n=10):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smca_probe.txt"))
    args = ap.parse_args()
    from yolov7_d2_amd.modeling import attention_torch, dense_gaussian, mha_core, smca_core
    dev = "cuda"
    E = HEADS * HD
    lines = [f"SMCA attention: fused (mi_smca_fwd / bwd) vs (i) the dense torch composition incl. building the prior, (ii) mha_core without "
             f"the prior; B {B}, {HEADS} heads, {LQ} queries, bf16, {torch.cuda.get_device_name(0)}",
             "times: microseconds per call, median of 7 interleaved windows of 10 calls; x = dense / fused; +% = fused over mha_core",
             f"{'map':>7} {'drop':>4} | {'fwd fused':>9} {'dense':>8} {'x':>5} {'mha':>7} {'+%':>5} | {'bwd fused':>9} {'dense':>8} {'x':>5} "
             f"{'mha':>7} {'+%':>5} | max |fused - dense| / max |dense|: out, dq dk dv dpoint dcoef (dropout 0 only)"]
    slower = []
    for Hm, W in MAPS:
        for p in (0.0, 0.1):
            Lk = Hm * W
            g = torch.Generator(device="cpu").manual_seed(Lk)
            rnd = lambda *s: torch.randn(*s, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
            q, k, v = rnd(LQ, B, E), rnd(Lk, B, E), rnd(Lk, B, E)
            point = (torch.rand(LQ, B, HEADS, 2, generator=g) * torch.tensor([W - 1.0, Hm - 1.0])).to(dev).requires_grad_(True)
            coef = torch.cat([(0.3 + 0.7 * torch.rand(LQ, B, HEADS, 2, generator=g)) ** 2, torch.zeros(LQ, B, HEADS, 1)], -1).to(dev).requires_grad_(True)
            mask = torch.zeros(B, Hm, W, dtype=torch.bool, device=dev)
            mask[1, :, W * 5 // 7:] = True
            mask = mask.flatten(1)
            dout = torch.randn(LQ, B, E, generator=g).to(dev, torch.bfloat16)
            ops = [q, k, v, point, coef]
            fused = lambda: smca_core(q, k, v, point, coef, (Hm, W), SMOOTH, mask, HEADS, p, 1234)
            dense = lambda: attention_torch(q, k, v, dense_gaussian(point, coef, (Hm, W), SMOOTH).to(torch.bfloat16), mask, HEADS, p)
            plain = lambda: mha_core(q, k, v, mask, HEADS, p, 1234)
            tf, td, tm = interleaved([fused, dense, plain])
            of, od, om = fused(), dense(), plain()
            bf, bd, bm = interleaved([lambda: torch.autograd.grad(of, ops, dout, retain_graph=True),
                                      lambda: torch.autograd.grad(od, ops, dout, retain_graph=True),
                                      lambda: torch.autograd.grad(om, ops[:3], dout, retain_graph=True)])
            errs = ""
            if p == 0:
                gf, gd = torch.autograd.grad(of, ops, dout, retain_graph=True), torch.autograd.grad(od, ops, dout, retain_graph=True)
                rel = lambda a, b: float((a.float() - b.float()).abs().max() / b.float().abs().max())
                errs = " ".join(f"{e:.1e}" for e in [rel(of, od)] + [rel(a, b) for a, b in zip(gf, gd)])
            lines.append(f"{Hm:>3}x{W:<3} {p:>4} | {tf:>9.1f} {td:>8.1f} {td / tf:>5.1f} {tm:>7.1f} {100 * (tf / tm - 1):>5.0f} | "
                         f"{bf:>9.1f} {bd:>8.1f} {bd / bf:>5.1f} {bm:>7.1f} {100 * (bf / bm - 1):>5.0f} | {errs}")
            if tf > td:
                slower.append(f"forward {Hm}x{W} dropout {p}: fused {tf:.1f} us > dense {td:.1f} us")
            if bf > bd:
                slower.append(f"backward {Hm}x{W} dropout {p}: fused {bf:.1f} us > dense {bd:.1f} us")
            del of, od, om
    lines.append("slower than the dense composition: " + ("; ".join(slower) if slower else "nowhere"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
