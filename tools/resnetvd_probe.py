"""What the ResNet-vd backbone costs on one MI355X, two measurements in one process.

(a) the shortcut's pool kernels (mi_avgpool2x2s2_fwd / _bwd) against torch's F.avg_pool2d(2, 2, ceil_mode=True,
    count_include_pad=False) forward and backward on the same bf16 channels-last tensors, at the three pooled shapes of a
    640 x 640 batch of 8: 80x80x256 (from 160x160), 40x40x512, 20x20x1024.  Each side runs `--reps` back-to-back calls
    between two HIP events (a single call is a few microseconds: launch overhead, not the kernel); the two sides alternate
    `--rounds` times after a warm-up; the medians and the spread of the per-call times are written down, and the bytes each
    pass has to move (input once + output once) over the median.
(b) the SparseInst training step (batch 8, 640 x 640, bench.py's synthetic targets) with build_resnet_vd_backbone beside the
    same step with build_resnet_backbone: eager and captured (graph_step.GraphedTrainStep), the four variants alternating.
    Nobody has measured this backbone before: there is no target, the numbers are a first record.

  python tools/resnetvd_probe.py [--rounds 15] [--reps 50] [--steps 10] [--out profiles/resnetvd_probe.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                      # noqa: E402
import torch.nn.functional as F   # noqa: E402

POOL_SHAPES = [(8, 160, 160, 256), (8, 80, 80, 512), (8, 40, 40, 1024)]     # inputs; the pooled maps are 80x80, 40x40, 20x20


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps      # us per call


def probe_pool(args, say):
    from yolov7_d2_amd import _lib as L
    lib = L.lib()
    say(f"(a) pool kernels against torch, {args.rounds} alternating rounds of {args.reps} back-to-back calls, us per call: median [min .. max]")
    verdict = []
    for (N, H, W, C) in POOL_SHAPES:
        g = torch.Generator().manual_seed(H)
        x = torch.randn(N, C, H, W, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
        xh = x.permute(0, 2, 3, 1)
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        y = torch.empty(N, Ho, Wo, C, dtype=torch.bfloat16, device="cuda")
        dy = torch.randn(N, C, Ho, Wo, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
        dyh = dy.permute(0, 2, 3, 1)
        dx = torch.empty(N, H, W, C, dtype=torch.bfloat16, device="cuda")
        xg = x.clone().requires_grad_(True)
        yt = F.avg_pool2d(xg, 2, 2, ceil_mode=True, count_include_pad=False)
        st = L.stream_ptr()

        def ours_f():
            L.check(lib.mi_avgpool2x2s2_fwd(xh.data_ptr(), C, y.data_ptr(), C, N, H, W, C, st), "fwd")

        def ours_b():
            L.check(lib.mi_avgpool2x2s2_bwd(dyh.data_ptr(), C, dx.data_ptr(), C, None, 0, 0, N, H, W, C, st), "bwd")

        def torch_f():
            with torch.no_grad():
                F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False)

        def torch_b():
            torch.autograd.grad(yt, xg, dy, retain_graph=True)
        # same results first (faster and different is not faster)
        ours_f(); ours_b()
        assert torch.equal(y.permute(0, 3, 1, 2), F.avg_pool2d(x.float(), 2, 2, ceil_mode=True, count_include_pad=False).to(torch.bfloat16))
        assert torch.equal(dx.permute(0, 3, 1, 2), torch.autograd.grad(yt, xg, dy, retain_graph=True)[0])
        byt = (N * H * W * C + N * Ho * Wo * C) * 2
        for name, a, b in (("forward ", ours_f, torch_f), ("backward", ours_b, torch_b)):
            for fn in (a, b):
                events(fn, args.reps)                      # warm-up
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(events(a, args.reps))
                tb.append(events(b, args.reps))
            ma, mb = statistics.median(ta), statistics.median(tb)
            verdict.append(ma <= mb)
            say(f"  {Ho}x{Wo}x{C} pooled (batch {N}) {name}: mi_avgpool2x2s2 {ma:7.2f} [{min(ta):7.2f} .. {max(ta):7.2f}]   "
                f"torch {mb:7.2f} [{min(tb):7.2f} .. {max(tb):7.2f}]   {byt / 1e6:.1f} MB -> {byt / ma / 1e6:.2f} TB/s   "
                f"{'not slower' if ma <= mb else 'SLOWER'} than torch")
    say("  (each tensor pair, 33 - 131 MB, is re-read call after call and fits the 256 MB Infinity Cache: the TB/s are cache-assisted rates, for both sides alike, not HBM rates)")
    say(f"  the new kernels are {'not slower than torch at any of the three shapes' if all(verdict) else 'SLOWER than torch somewhere: see above'}")


def probe_step(args, say):
    import yolov7_d2_amd as M
    from yolov7_d2_amd.d2shim import Instances
    from yolov7_d2_amd.graph_step import GraphedTrainStep
    from yolov7_d2_amd.optim import MultiTensorAdamW
    B, S = 8, 640
    g = torch.Generator().manual_seed(1234)
    yy, xx = torch.meshgrid(torch.arange(S).float(), torch.arange(S).float(), indexing="ij")
    inputs = []
    for b in range(B):
        n = int(torch.randint(1, 11, (1,), generator=g))
        masks = torch.zeros(n, S, S)
        for k in range(n):
            cy, cx = float(torch.rand(1, generator=g)) * S, float(torch.rand(1, generator=g)) * S
            ry, rx = 16 + float(torch.rand(1, generator=g)) * S * 0.25, 16 + float(torch.rand(1, generator=g)) * S * 0.25
            masks[k] = ((yy - cy).abs() < ry) & ((xx - cx).abs() < rx)
        inst = Instances((S, S), gt_classes=torch.randint(0, 80, (n,), generator=g).cuda(), gt_masks=masks.cuda())
        inputs.append(dict(image=torch.randint(0, 256, (3, S, S), generator=g).float().cuda(), instances=inst, height=S, width=S))
    runs = {}
    closers = []
    for bb in ("build_resnet_vd_backbone", "build_resnet_backbone"):
        for graphed in (False, True):
            torch.manual_seed(0)
            cfg = M.sparse_inst_r50_giam_cfg(device="cuda")
            cfg.MODEL.BACKBONE.NAME = bb
            model = M.build_model(cfg).train()
            opt = MultiTensorAdamW([p for p in model.parameters() if p.requires_grad], lr=5e-5, weight_decay=0.05)
            if graphed:
                gs = GraphedTrainStep(model, opt)
                closers.append(gs)
                fn = (lambda gs=gs: gs(inputs)["total"])
            else:
                def fn(model=model, opt=opt):
                    losses = model(inputs)
                    total = sum(losses.values())
                    opt.zero_grad(set_to_none=True)
                    total.backward()
                    opt.step()
                    return total
            runs[(bb, "captured" if graphed else "eager")] = fn
    times = {k: [] for k in runs}
    for k, fn in runs.items():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds_step):
        for k, fn in runs.items():
            times[k].append(events(fn, args.steps) / 1e3)       # ms per step
    say(f"(b) SparseInst training step, batch {B} x {S} x {S}, {args.rounds_step} alternating rounds of {args.steps} steps, "
        "ms per step: median [min .. max] -> images/s at the median")
    for k, t in times.items():
        m = statistics.median(t)
        say(f"  {k[0]:26s} {k[1]:8s} {m:8.2f} [{min(t):8.2f} .. {max(t):8.2f}]  -> {B / m * 1e3:7.1f} images/s")
    for gs in closers:
        gs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds-step", dest="rounds_step", type=int, default=5)
    ap.add_argument("--only", type=str, default="", help="pool | step")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnetvd_probe: needs the GPU (a timing taken anywhere else says nothing)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"resnetvd_probe on {torch.cuda.get_device_name(0)}")
    if args.only in ("", "pool"):
        probe_pool(args, say)
    if args.only in ("", "step"):
        probe_step(args, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
