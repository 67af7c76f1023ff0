"""Row-column decoupled attention (csrc/rcda.hip through modeling.rcda_core) beside the torch composition of the same
definition, bf16 on the device, in the two-stage matmul form the reference uses
(row_column_decoupled_attention.py:233-249: contract the shorter map side first, which materialises a [B heads, L, S, 32]
intermediate, S = min(H, W), and keeps it for the backward).

Shapes, all at B 4 (the batch of this project's captured DETR step at 800 x 1333) and 8 heads: L 900 and L 1050 on a 25 x 42
map (Anchor DETR's decoder and encoder), L 900 and L 4200 on 50 x 84 (a dilated C5 map and its encoder self-attention).
Both forms take the same projected operands (q_row, q_col [B, L, E], k_row [B, W, E], k_col [B, H, E], v [B, H, W, E]) and
masks.  Forward: one call; backward: torch.autograd.grad of the output for all five operands (fused: three launches + the
allocation of the gradients and the workspace; torch: whatever autograd runs).  HIP events around 10 back-to-back calls,
median of 7 windows after a warm-up, the two forms INTERLEAVED window by window in one process.

Bytes each form must move (algorithmic minimum, bf16): fused forward = the operands once + the output + the two lse rows;
fused backward = operands, cotangent and lse once + the five gradients + the softmax-gradient workspace written and read once.
Torch = the same + the [B heads, L, S, 32] intermediate written and read once forward, and read once + its gradient written
and read once backward (the score / softmax tensors of a few MB are left out of both).

  python tools/rcda_probe.py [--out profiles/rcda_probe.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                        # noqa: E402

SHAPES = [(900, 25, 42), (1050, 25, 42), (900, 50, 84), (4200, 50, 84)]
B, HEADS, HD = 4, 8, 32


def torch_core(q_row, q_col, k_row, k_col, v, mask_row, mask_col, heads):
    """the reference's composition after its in-projections, on batch-first operands -> [B, L, E]"""
    Bn, Lq, E = q_row.shape
    H, W = v.shape[1], v.shape[2]
    hd = E // heads
    scale = hd ** -0.5
    sp = lambda x: x.reshape(Bn, -1, heads, hd).transpose(1, 2).reshape(Bn * heads, -1, hd)
    qr, qc, kr, kc = sp(q_row) * scale, sp(q_col) * scale, sp(k_row), sp(k_col)
    vv = v.reshape(Bn, H, W, heads, hd).permute(0, 3, 1, 2, 4).reshape(Bn * heads, H, W, hd)
    wr = torch.bmm(qr, kr.transpose(1, 2)).view(Bn, heads, Lq, W).masked_fill(mask_row[:, None, None, :], float("-inf"))
    wc = torch.bmm(qc, kc.transpose(1, 2)).view(Bn, heads, Lq, H).masked_fill(mask_col[:, None, None, :], float("-inf"))
    wr = torch.softmax(wr.view(Bn * heads, Lq, W), dim=-1)
    wc = torch.softmax(wc.view(Bn * heads, Lq, H), dim=-1)
    if H < W:
        row = torch.matmul(wr, vv.permute(0, 2, 1, 3).reshape(Bn * heads, W, H * hd)).reshape(Bn * heads, Lq, H, hd).permute(0, 2, 1, 3)
        out = torch.matmul(wc.permute(1, 0, 2)[:, :, None, :], row.permute(2, 0, 1, 3)).squeeze(-2)        # [L, B heads, hd]
        return out.reshape(Lq, Bn, E).transpose(0, 1)
    col = torch.matmul(wc, vv.reshape(Bn * heads, H, W * hd)).reshape(Bn * heads, Lq, W, hd)
    out = torch.matmul(wr[:, :, None, :], col).squeeze(-2).permute(1, 0, 2)
    return out.reshape(Lq, Bn, E).transpose(0, 1)


def window(fn, n=10):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / n


def interleaved(fa, fb, reps=7):
    """(median us of fa, of fb): windows of the two alternate"""
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window(fa))
        tb.append(window(fb))
    return statistics.median(ta), statistics.median(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rcda_probe.txt"))
    args = ap.parse_args()
    from yolov7_d2_amd.modeling import rcda_core
    dev = "cuda"
    E = HEADS * HD
    lines = [f"row-column decoupled attention: fused (csrc/rcda.hip) vs the torch composition, B {B}, {HEADS} heads, bf16, {torch.cuda.get_device_name(0)}",
             "times: microseconds per call, median of 7 interleaved windows of 10 calls; MB: bytes each form must move (see the tool's text)",
             f"{'L':>5} {'map':>7} | {'fwd fused':>9} {'torch':>8} {'x':>5} | {'bwd fused':>9} {'torch':>8} {'x':>5} | "
             f"{'MB fwd f/t':>13} {'MB bwd f/t':>13} | max |fused - torch| / max |torch|: out, grads"]
    slower = []
    for Lq, H, W in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(Lq + H)
        rnd = lambda *s: torch.randn(*s, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
        ops = [rnd(B, Lq, E), rnd(B, Lq, E), rnd(B, W, E), rnd(B, H, E), rnd(B, H, W, E)]
        mask = torch.zeros(B, H, W, dtype=torch.bool, device=dev)
        mask[1, :, W * 5 // 7:] = True
        mask[1, H * 4 // 5:, :] = True
        mr, mc = mask[:, 0, :].contiguous(), mask[:, :, 0].contiguous()
        dout = torch.randn(B, Lq, E, generator=g).to(dev, torch.bfloat16)
        fused = lambda: rcda_core(*ops, mr, mc, HEADS)
        comp = lambda: torch_core(*ops, mr, mc, HEADS)
        tf, tt = interleaved(fused, comp)
        of, ot = fused(), comp()
        bf, bt = interleaved(lambda: torch.autograd.grad(of, ops, dout, retain_graph=True),
                             lambda: torch.autograd.grad(ot, ops, dout, retain_graph=True))
        gf, gt = torch.autograd.grad(of, ops, dout, retain_graph=True), torch.autograd.grad(ot, ops, dout, retain_graph=True)
        rel = lambda a, b: float((a.float() - b.float()).abs().max() / b.float().abs().max())
        errs = [rel(of, ot)] + [rel(a, b) for a, b in zip(gf, gt)]
        operands = B * (2 * Lq * E + (W + H) * E + H * W * E) * 2
        lse = 2 * B * HEADS * Lq * 4
        inter = B * HEADS * Lq * min(H, W) * HD * 2
        ws = B * HEADS * (H + W) * ((Lq + 31) // 32 * 32) * 2
        mb_ff, mb_tf = operands + B * Lq * E * 2 + lse, operands + B * Lq * E * 2 + 2 * inter
        mb_fb, mb_tb = 2 * operands + B * Lq * E * 2 + lse + 2 * ws, 2 * operands + B * Lq * E * 2 + 3 * inter
        lines.append(f"{Lq:>5} {H:>3}x{W:<3} | {tf:>9.1f} {tt:>8.1f} {tt / tf:>5.1f} | {bf:>9.1f} {bt:>8.1f} {bt / bf:>5.1f} | "
                     f"{mb_ff / 1e6:>5.1f} /{mb_tf / 1e6:>6.1f} {mb_fb / 1e6:>5.1f} /{mb_tb / 1e6:>6.1f} | "
                     + " ".join(f"{e:.1e}" for e in errs))
        if tf > tt:
            slower.append(f"forward L {Lq} {H}x{W}: fused {tf:.1f} us > torch {tt:.1f} us")
        if bf > bt:
            slower.append(f"backward L {Lq} {H}x{W}: fused {bf:.1f} us > torch {bt:.1f} us")
        del ops, of, ot, gf, gt
    lines.append("slower than the composition: " + ("; ".join(slower) if slower else "nowhere"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
