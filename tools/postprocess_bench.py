"""YOLOX eval postprocess: the per-image loop (`_postprocess_per_image`, two host syncs per image) against the batched
device path (`postprocess` -> `postprocess_batched` + one read-back of the counts) on the same inputs, alternating the
two in one process; device events around each call, a synchronise after it.  Both paths are checked for bit equality on
every configuration before anything is timed.

Inputs: oracle synth_decoded's clustered boxes and class scores, with the objectness of a detector that sees few
objects (sigmoid of a normal whose mean is drawn per image), so each image keeps a different, realistic share of its
anchors as candidates; n_i per image is printed so the mix of NMS forms (4 n <= 4000: offsets, else class by class) is
visible.

  python tools/postprocess_bench.py [--B 1 16] [--A 8400 12600] [--conf 0.001 0.01 0.3] [--iters 20] [--out f.txt]
A kernel trace of the batched path alone: --only batched --iters 5 under rocprofv3 --kernel-trace --stats."""
import argparse
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import yolox_oracle as O  # noqa: E402
import yolov7_d2_amd as M  # noqa: E402

PP = importlib.import_module("yolov7_d2_amd.modeling.postprocess")   # (the package re-exports the function of that name)


def make_input(B, A, seed, C=80):
    pred = O.synth_decoded(B, A, seed, num_classes=C)
    g = torch.Generator().manual_seed(seed + 1)
    mu = torch.rand(B, 1, generator=g) * 3.0 - 6.0              # per-image objectness logit mean in [-6, -3)
    pred[..., 4] = torch.sigmoid(mu + 2.5 * torch.randn(B, A, generator=g))
    return pred


def bits(t):
    return t.contiguous().view(torch.int32)


def check_equal(x, C, conf, nms):
    a, b = x.clone(), x.clone()
    ref = PP._postprocess_per_image(a, C, conf, nms)
    got = M.postprocess(b, C, conf, nms)
    assert torch.equal(bits(a), bits(b)), "prediction rewrite differs"
    for i, (r, g) in enumerate(zip(ref, got)):
        assert (r is None) == (g is None), i
        if r is not None:
            assert r.shape == g.shape and torch.equal(bits(r), bits(g)), i


def time_call(fn, x, buf):
    buf.copy_(x)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(buf)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3      # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--A", type=int, nargs="+", default=[8400, 12600])
    ap.add_argument("--conf", type=float, nargs="+", default=[0.001, 0.01, 0.3])
    ap.add_argument("--nms", type=float, default=0.65)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["both", "batched"], default="both")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("postprocess_bench: needs a GPU (nothing to time on the CPU)")
    dev = torch.device("cuda")
    C = 80
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# postprocess: per-image loop vs batched, nms {a.nms}, {a.iters} timed calls each (alternating), "
         f"{a.warmup} warm-up; us per image = median call time / B; device events + synchronise")
    emit(f"{'B':>3} {'A':>6} {'conf':>6} | {'loop us/img':>11} {'batched us/img':>14} {'device-only us/img':>18} "
         f"{'speed-up':>8} | n_i (candidates per image)")
    loop = lambda t: PP._postprocess_per_image(t, C, conf, a.nms)                 # noqa: E731
    full = lambda t: M.postprocess(t, C, conf, a.nms)                             # noqa: E731
    dev_only = lambda t: M.postprocess_batched(t, C, conf, a.nms)                 # noqa: E731
    for B in a.B:
        for A in a.A:
            for conf in a.conf:
                x = make_input(B, A, seed=1000 * B + A + int(conf * 1e4)).to(dev)
                n = ((x[..., 4] * x[..., 5:5 + C].max(-1).values) >= conf).sum(1).tolist()
                buf = torch.empty_like(x)
                if a.only == "batched":
                    for _ in range(a.warmup):
                        time_call(dev_only, x, buf)
                    ts = [time_call(dev_only, x, buf) for _ in range(a.iters)]
                    emit(f"{B:>3} {A:>6} {conf:>6} | {'-':>11} {'-':>14} {statistics.median(ts) / B:>18.1f} "
                         f"{'-':>8} | {n}")
                    continue
                check_equal(x, C, conf, a.nms)
                for _ in range(a.warmup):
                    for fn in (loop, full, dev_only):
                        time_call(fn, x, buf)
                tl, tf, td = [], [], []
                for _ in range(a.iters):
                    tl.append(time_call(loop, x, buf))
                    tf.append(time_call(full, x, buf))
                    td.append(time_call(dev_only, x, buf))
                ml, mf, md = (statistics.median(t) / B for t in (tl, tf, td))
                emit(f"{B:>3} {A:>6} {conf:>6} | {ml:>11.1f} {mf:>14.1f} {md:>18.1f} {ml / mf:>7.1f}x | {n}")
    emit("# equality: per-image loop == batched, bit for bit, on every configuration above"
         if a.only == "both" else "# batched path only (trace run)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    t0 = time.time()
    main()
    print(f"# wall {time.time() - t0:.1f} s")
