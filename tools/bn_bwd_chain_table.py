#!/usr/bin/env python
"""local: the one-launch BatchNorm backward, launch by launch, in two in-graph traces of the YOLOX-s step:
DIR/trace_<tagA>.csv and DIR/trace_<tagB>.csv (what tools/gpu_trace.sh writes) joined with DIR/tags.txt (the output of
tools/dump_tags.py).
Per launch: the plan's tag, map and C (a grouped launch: its number of jobs), us in A and in B (mean of the last replayed
steps), B - A, and the trace's own repeat-to-repeat difference for that launch (the larger of the two traces' max - min over
the replayed steps); the family sums.  usage: bn_bwd_chain_table.py DIR tagA tagB"""
import math, os, sys, collections
DIR = sys.argv[1]


def load(tag):
    rows = []
    for l in open(os.path.join(DIR, f"trace_{tag}.csv")):
        p = l.rstrip("\n").split("|")
        rows.append((p[0], int(p[1]), int(p[2])))
    starts = [i for i, r in enumerate(rows) if "focus_pack" in r[0]]
    steps = [rows[a:b] for a, b in zip(starts[:-1], starts[1:])]
    n = collections.Counter(len(s) for s in steps).most_common(1)[0][0]
    steps = [s for s in steps if len(s) == n][-4:]
    span = sum(s[-1][2] - s[0][1] for s in steps) / len(steps) / 1e3
    bn = [i for i in range(n) if "bn_bwd_fused" in steps[0][i][0]]
    return [(steps[0][i][0], [(s[i][2] - s[i][1]) / 1e3 for s in steps]) for i in bn], span, n, len(steps)


tags = [l.split(None, 4) for l in open(os.path.join(DIR, "tags.txt")) if l.startswith("bwd")]
bn_tags = [t for t in tags if t[2] == "BN_BWD_FUSED" or (t[2] == "BN_GROUP" and len(t) > 4 and t[4].startswith("kind3"))]
a, b = sys.argv[2:4]
ra, spana, na, sa = load(a)
rb, spanb, nb, sb = load(b)
assert len(ra) == len(rb) == len(bn_tags), (len(ra), len(rb), len(bn_tags))
print(f"{a}: {na} dispatches, step span {spana:.1f} us (mean of {sa} replayed steps);  {b}: {nb} dispatches, step span {spanb:.1f} us ({sb} steps)")
print(f"{'#':>3} {'map':>7} {'C':>5}  {a:>8} {b:>8} {'diff':>7} {'repeat':>7}  tag")
tot = collections.defaultdict(lambda: [0, 0.0, 0.0])
slower = 0
for k, (t, (name, da), (_, db)) in enumerate(zip(bn_tags, ra, rb)):
    info = dict()
    for w in (t[4].split() if len(t) > 4 else []):
        for key in ("count", "npix", "C", "kind", "jobs"):
            if w.startswith(key) and w[len(key):].isdigit():
                info[key] = int(w[len(key):])
    if "npix" in info:
        hw = int(round(math.sqrt(info["npix"] / 16)))
        m, c = f"{hw}x{hw}", str(info["C"])
    else:
        m, c = f"{info.get('jobs', '?')} jobs", "-"
    ma, mb = sum(da) / len(da), sum(db) / len(db)
    rep = max(max(da) - min(da), max(db) - min(db))
    fam = "group" if "group" in name else "single"
    for f in (fam, "all"):
        tot[f][0] += 1; tot[f][1] += ma; tot[f][2] += mb
    flag = ""
    if mb - ma > rep:
        slower += 1
        flag = "  SLOWER"
    print(f"{k:3d} {m:>7} {c:>5}  {ma:8.2f} {mb:8.2f} {mb - ma:7.2f} {rep:7.2f}  {t[3][:60]}{flag}")
for f in ("single", "group", "all"):
    n, x, y = tot[f]
    print(f"{f:>6}: {n} launches  {a} {x:8.1f} us  {b} {y:8.1f} us  diff {y - x:7.1f} us  ({(y - x) / max(n, 1):.2f} per launch)")
print(f"launches slower in {b} by more than their repeat-to-repeat difference: {slower}")
