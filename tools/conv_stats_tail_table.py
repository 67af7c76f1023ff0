#!/usr/bin/env python
"""local: what the BatchNorm-statistics part of the forward convolutions costs inside the captured YOLOX-s step.  Joins the
in-graph traces trace_<tag>.csv (tools/gpu_trace.sh, loaded by trace_steps.py) of several builds / settings by dispatch index:
  (1) every statistics launch (c1s_kernel / w3_kernel MODE 1, conv_igemm_kernel forward) per tag, summed per kernel class;
  (2) forward launch vs the data-gradient launch of the same kernel at the same shape (MODE 0, no statistics).
usage: conv_stats_tail_table.py <base tag> [tag ...]     (tags.txt from tools/dump_tags.py)"""
import collections, re, sys
import trace_steps as T


def short(k):
    return re.sub(r"^void ", "", k).replace("_kernel", "")


def mode_of(k):
    a = [x.strip() for x in k[k.index("<") + 1:k.rindex(">")].split(",")]
    if k.startswith("c1s"):
        return int(a[5]), (a[0], a[1], a[2], a[3])
    if k.startswith("w3"):
        return int(a[4]), (a[0], a[1], a[2], a[3], a[5], a[6])
    return None, None


tags = sys.argv[1:]
rows = {t: T.join(t) for t in tags}
base = rows[tags[0]][0]
print("# step span (us): " + "  ".join(f"{t} {rows[t][1]:.1f}" for t in tags))
# ---- (1) statistics launches, per tag
cls = collections.defaultdict(lambda: [0] + [0.0] * len(tags))
print("# statistics launches: tag, kernel, shape, us per tag (" + ", ".join(tags) + ")")
for i, (c, ds) in enumerate(base):
    if c[1] not in ("CONV", "CONV_GROUP") or c[0] != "fwd" or not ds:      # (CONV_GROUP: the CSP conv1 + conv2 pairs, the head towers)
        continue
    k = short(ds[0][0])
    m, _ = mode_of(k)
    if (k.startswith(("c1s", "w3")) and m != 1) or (c[1] == "CONV_GROUP" and not k.startswith(("c1s", "w3"))):
        continue      # (a grouped launch on the tile kernel: the head's prediction convolutions, no BatchNorm behind them)
    us = [rows[t][0][i][1][0][1] for t in tags]
    shape = re.sub(r"tile\S+.*$", "", c[3]).strip()
    print(f"{c[2][:44]:44s} {k[:40]:40s} {shape:26s} " + " ".join(f"{u:6.1f}" for u in us))
    key = k.split("<")[0] + " " + ("K" + k[k.index("<") + 1:].split(",")[0] if k.startswith(("c1s", "w3")) else "")
    cls[key][0] += 1
    for j, u in enumerate(us):
        cls[key][1 + j] += u
print("# per kernel class: launches, sum us per tag, difference to the base")
tot = [0.0] * len(tags)
for key, v in sorted(cls.items()):
    print(f"{key:24s} n={v[0]:3d} " + " ".join(f"{u:8.1f}" for u in v[1:]) + "   " + " ".join(f"{u - v[1]:+7.1f}" for u in v[2:]))
    tot = [a + b for a, b in zip(tot, v[1:])]
print(f"{'all':24s}       " + " ".join(f"{u:8.1f}" for u in tot) + "   " + " ".join(f"{u - tot[0]:+7.1f}" for u in tot[1:]))
# ---- (2) forward (MODE 1) vs data gradient (MODE 0) of the same instantiation, grid and shape
for t in tags:
    fwd, bwd = collections.defaultdict(list), collections.defaultdict(list)
    for c, ds in rows[t][0]:
        if c[1] != "CONV" or not ds:
            continue
        k = short(ds[0][0])
        m, inst = mode_of(k)
        if inst is None:
            continue
        sh = re.search(r"(\d+x\d+) K(\d+) Co(\d+)", c[3])
        if not sh or (c[0] == "bwd" and sh.group(2) != sh.group(3) and not k.startswith("c1s")):
            continue
        # a data gradient reads Co channels and writes K: the partner of a forward K -> Co is the gradient with the sizes swapped
        key = (k.split("<")[0], inst, ds[0][2], sh.group(1), (sh.group(2), sh.group(3)) if c[0] == "fwd" else (sh.group(3), sh.group(2)))
        if c[0] == "fwd" and m == 1:
            fwd[key].append(ds[0][1])
        if c[0] == "bwd" and m == 0:
            bwd[key].append(ds[0][1])
    print(f"# {t}: forward (statistics) vs data gradient (none), same kernel instantiation / grid / map: n, mean us, gap")
    gsum = 0.0
    for key in sorted(fwd, key=str):
        if key not in bwd:
            continue
        f, b = sum(fwd[key]) / len(fwd[key]), sum(bwd[key]) / len(bwd[key])
        gsum += (f - b) * len(fwd[key])
        print(f"  {key[0]}<{','.join(key[1])}> {key[3]:8s} K{key[4][0]}->{key[4][1]:4s} fwd n={len(fwd[key]):2d} {f:6.1f}   dgrad n={len(bwd[key]):2d} {b:6.1f}   gap {f - b:+5.1f}")
    print(f"  sum of gaps over the forward launches with a partner: {gsum:.1f} us")
