"""Numpy restatement of the polygon rasteriser the reference's SparseInst uses for INPUT.MASK_FORMAT "polygon"
(meta_arch/sparseinst.py:111-115: BitMasks.from_polygon_masks -> detectron2's polygons_to_bitmask = pycocotools frPyObjects,
merge, decode; the arithmetic is rleFrPoly of pycocotools' maskApi.c).

pycocotools and detectron2 are NOT installed where this suite runs, so this is an UNPINNED restatement - written from the
published algorithm, not checked against the library here - like the other pycocotools-facing oracles of this suite
(oracle/coco_rle_oracle.py).  tests/test_polygon_ref.py guards it: a hand-checked rectangle, the even crossing count of every
column, and an independent cross-check against PIL.ImageDraw.polygon.

It is deliberately the GLOBAL form: all points of the ring in one list, every consecutive pair looked at (the pairs that
straddle two edges included), the crossings as keys x * h + y, and a pixel set iff the number of keys <= its column-major
index is odd.  No per-column shortcut, no per-edge shortcut: those are what the kernel under test takes.

All arithmetic is IEEE double precision; int() truncates toward zero like the C casts.
"""
import math

import numpy as np


def ring_points(xy):
    """the (u, v) integer points rleFrPoly walks along the closed ring, 5x upsampled, edge after edge"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1)
    k = xy.size // 2
    X = [int(5.0 * float(xy[2 * j]) + 0.5) for j in range(k)]
    Y = [int(5.0 * float(xy[2 * j + 1]) + 0.5) for j in range(k)]
    X.append(X[0])
    Y.append(Y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            # (dx == dy == 0: the C original forms s = 0 / 0 and multiplies it by t = 0 - NaN + ys + 0.5 cast to int.  The one
            # point it emits has the u of both neighbours, so it never makes a crossing; it is emitted here with v = ys)
            s = float(ye - ys) / float(dx) if dx > 0 else 0.0
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(float(ys) + s * float(t) + 0.5))
        else:
            s = float(xe - xs) / float(dy)
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(float(xs) + s * float(t) + 0.5))
    return u, v


def ring_crossing_points(xy, h, w):
    """the ring's crossings as (column x, row y) with 0 <= x <= w - 1 and 0 <= y <= h, in walking order"""
    u, v = ring_points(xy)
    pts = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + 0.5) / 5.0 - 0.5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + 0.5) / 5.0 - 0.5
        if yd < 0:
            yd = 0.0
        elif yd > h:
            yd = float(h)
        yd = math.ceil(yd)
        pts.append((int(xd), int(yd)))
    return pts


def ring_crossings(xy, h, w):
    """the keys a = x * h + y of the ring's crossings, unsorted"""
    return [x * h + y for x, y in ring_crossing_points(xy, h, w)]


def ring_mask(xy, h, w):
    """uint8 [h, w]: pixel (y, x) is set iff the number of crossing keys <= x * h + y is odd"""
    keys = np.asarray(ring_crossings(xy, h, w), dtype=np.int64)
    toggles = np.zeros(h * w + 1, dtype=np.int64)
    keys = keys[keys <= h * w]                       # (a key is at most (w - 1) * h + h)
    np.add.at(toggles, keys, 1)
    par = (np.cumsum(toggles)[: h * w] & 1).astype(np.uint8)
    return np.ascontiguousarray(par.reshape(w, h).T)


def instance_mask(rings, h, w):
    """the union of the rings' masks (frPyObjects, merge, decode)"""
    m = np.zeros((h, w), dtype=np.uint8)
    for r in rings:
        m |= ring_mask(r, h, w)
    return m


def polygon_masks(instances, h, w):
    """uint8 [M, h, w] for one image: `instances` is a list of instances, each a list of rings [x0, y0, x1, y1, ...]"""
    out = np.zeros((len(instances), h, w), dtype=np.uint8)
    for i, rings in enumerate(instances):
        out[i] = instance_mask(rings, h, w)
    return out


# ------------------------------------------------------------------------------------------------ shared test cases
def random_rings(n=60, seed=0):
    """[(xy, h, w)]: rings of 3 - 8 vertices on images of 8 - 70 pixels a side, in turn with vertices sorted by angle (a
    simple ring), unsorted (self-intersecting) and snapped to half-integers; radii up to 0.7 of the image around a centre
    anywhere inside it, so vertices fall outside the image, negative coordinates included"""
    rng = np.random.default_rng(seed)
    cases = []
    for it in range(n):
        h, w = (int(v) for v in rng.integers(8, 71, 2))
        k = int(rng.integers(3, 9))
        ang = rng.uniform(0.0, 2.0 * np.pi, k)
        if it % 3 != 1:
            ang = np.sort(ang)
        rad = rng.uniform(0.1, 0.7, k) * max(h, w)
        cx, cy = rng.uniform(0.0, w), rng.uniform(0.0, h)
        xy = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).reshape(-1)
        if it % 3 == 2:
            xy = np.round(xy * 2.0) / 2.0
        cases.append((xy, h, w))
    return cases
