#!/usr/bin/env python
"""GPU box, diagnostic build (tools/build_variant.sh bntl "-DMI_BN_CHAIN_TIMELINE" bn_act; MI355_LIB=.../libmi355det_bntl.so):
where does the one-launch BatchNorm backward spend the time between its two phases?  Thread 0 of every block stamps twelve
points (wall_clock64, 100 MHz, one counter for the whole chip): see csrc/bn_act.hip.  Per launch: the median and the maximum
over the blocks of every interval, the chain of the block that arrived last (it folds and releases), and the critical path
from the last arrival to the other blocks' first dy store.  All times in us (10 ns resolution).
Shapes: B = 16 maps of YOLOX-s; LAUNCHES measured launches per shape after three warm ones, rotating over NSET buffer sets."""
import ctypes as C, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from yolov7_d2_amd import _lib as L

lib = L.lib()
assert hasattr(lib, "mi_debug_bn_timeline"), "not a -DMI_BN_CHAIN_TIMELINE build (MI355_LIB)"
DEV = "cuda"
NP, NBMAX = 12, 1024
SHAPES = [(20, 256), (20, 512), (40, 128), (40, 256), (80, 64), (80, 128), (160, 64)]
NSET = int(os.environ.get("NSET", 3)); LAUNCHES = int(os.environ.get("LAUNCHES", 3))
sp = L.stream_ptr()
cap = lib.mi_bn_fused_set_capacity(0)
buf = (C.c_longlong * (NP * NBMAX))()
EVERY = [("phase 1: loads, dz, thread sums", 0, 1), ("thread sums -> LDS", 1, 2), ("block adds + fp64 atomics acknowledged", 2, 3),
         ("block barrier + arrival counted", 3, 4)]
OTHERS = [("arrival -> release observed", 4, 8), ("release observed -> totals in LDS", 8, 9), ("totals in LDS -> first dy store", 9, 10),
          ("first dy store -> end", 10, 11)]
LAST = [("arrival -> slots loaded", 4, 5), ("slots loaded -> totals stored, acknowledged", 5, 6), ("release issued", 6, 7),
        ("released -> totals in LDS", 7, 9), ("totals in LDS -> first dy store", 9, 10), ("first dy store -> end", 10, 11)]


def us(t):
    return t * 0.01


def med_max(v):
    return "%6.2f %6.2f" % (us(statistics.median(v)), us(max(v)))


for hw, Cc in SHAPES:
    npix = 16 * hw * hw
    ld = (Cc + 31) // 32 * 32
    sets = [(torch.randn(npix, ld, device=DEV).to(torch.bfloat16), torch.randn(npix, ld, device=DEV).to(torch.bfloat16),
             torch.empty(npix, ld, dtype=torch.bfloat16, device=DEV)) for _ in range(NSET)]
    mean = torch.zeros(Cc, device=DEV); invstd = torch.ones(Cc, device=DEV); gamma = torch.ones(Cc, device=DEV)
    scale = torch.ones(Cc, device=DEV); shift = torch.zeros(Cc, device=DEV)
    dacc = torch.zeros(L.MI_BN_SLOTS * ld * 2, dtype=torch.float64, device=DEV)
    dg = torch.zeros(Cc, device=DEV); db = torch.zeros(Cc, device=DEV)
    bar = torch.zeros(L.MI_BN_BAR_WORDS, dtype=torch.int32, device=DEV)
    PLn = 256 // (Cc // 8)
    nb = max(1, min(cap, -(-npix * (Cc // 8) // (PLn * (Cc // 8) * 4))))
    print("== %dx%dx%d  B 16  npix %d  blocks %d  items/thread %.1f  tensor %.1f MB" % (
        hw, hw, Cc, npix, nb, npix / (nb * PLn), npix * ld * 2 / 1e6), flush=True)
    for it in range(3 + LAUNCHES):
        da, y, dy = sets[it % NSET]
        dacc.zero_()
        torch.cuda.synchronize()
        L.check(lib.mi_bn_act_bwd_fused(da.data_ptr(), ld, y.data_ptr(), ld, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                                        invstd.data_ptr(), gamma.data_ptr(), dacc.data_ptr(), L.MI_BN_SLOTS, npix, dg.data_ptr(),
                                        db.data_ptr(), dy.data_ptr(), ld, None, 0, 0, npix, Cc, 1, bar.data_ptr(), sp), "fused")
        torch.cuda.synchronize()
        assert lib.mi_debug_bn_timeline(buf) == 0
        assert int(bar[2]) == 0, "a wait gave up"
        if it < 3:
            continue
        t = [[buf[b * NP + k] for k in range(NP)] for b in range(nb)]
        last = [b for b in range(nb) if t[b][7] != 0]
        assert len(last) == 1 and all(t[b][8] != 0 for b in range(nb) if b != last[0]), "stamps of the last block"
        lb = last[0]
        oth = [b for b in range(nb) if b != lb]
        t0 = min(r[0] for r in t)
        print("  launch %d: span %.2f (first start -> last end); last arriver: block %d" % (
            it - 2, us(max(r[11] for r in t) - t0), lb))
        print("    %-46s %6s %6s" % ("every block (median, max over blocks)", "med", "max"))
        for name, a, b in EVERY:
            print("    %-46s %s" % (name, med_max([r[b] - r[a] for r in t])))
        if oth:
            for name, a, b in OTHERS:
                print("    %-46s %s" % (name, med_max([t[k][b] - t[k][a] for k in oth])))
        print("    %-46s" % "the last arriver's own chain")
        for name, a, b in LAST:
            print("    %-46s %6.2f" % (name, us(t[lb][b] - t[lb][a])))
        arr = sorted(r[4] for r in t)
        print("    arrivals: first %.2f  median %.2f  last %.2f after the first start; loads consumed by the last arriver at %.2f" % (
            us(arr[0] - t0), us(statistics.median(arr) - t0), us(arr[-1] - t0), us(t[lb][1] - t0)))
        if oth:
            chain = [t[k][10] - t[lb][1] for k in oth]
            print("    CHAIN: last arriver's loads consumed -> first dy store of the other blocks: median %.2f  max %.2f;"
                  " of it last arrival -> release observed: median %.2f  max %.2f" % (
                      us(statistics.median(chain)), us(max(chain)), us(statistics.median([t[k][8] - t[lb][4] for k in oth])),
                      us(max(t[k][8] - t[lb][4] for k in oth))), flush=True)
