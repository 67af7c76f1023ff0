"""CPU: the yardstick of the polygon rasteriser (tests/polygon_raster_ref.py, an unpinned restatement of pycocotools'
rleFrPoly) is itself checked here - a hand-checked rectangle, the even number of crossings in every column, an independent
cross-check against PIL - together with the argument errors of mi_polygon_masks / ops.polygon_masks_batch that need no device."""
import ctypes as C

import numpy as np
import pytest

import polygon_raster_ref as R
from yolov7_d2_amd import _lib as L


def test_rectangle_by_hand():
    m = R.ring_mask([2, 2, 6, 2, 6, 5, 2, 5], 8, 10)
    want = np.zeros((8, 10), np.uint8)
    want[2:5, 2:6] = 1
    assert np.array_equal(m, want)
    # the same ring with its first vertex repeated, and walked the other way round
    assert np.array_equal(R.ring_mask([2, 2, 6, 2, 6, 5, 2, 5, 2, 2], 8, 10), want)
    assert np.array_equal(R.ring_mask([2, 5, 6, 5, 6, 2, 2, 2], 8, 10), want)
    assert R.instance_mask([[2, 2, 6, 2, 6, 5, 2, 5], [0, 0, 1, 0, 1, 1, 0, 1]], 8, 10).sum() == 12 + 1


def test_every_column_gets_an_even_number_of_crossings():
    """a closed ring crosses every line between two columns an even number of times: what lets a rasteriser restart the
    parity in every column (a crossing at row h counts for the column it was found in)"""
    total = 0
    for xy, h, w in R.random_rings(60, seed=0):
        pts = R.ring_crossing_points(xy, h, w)
        counts = np.bincount(np.asarray([x for x, _ in pts], dtype=np.int64), minlength=w)
        assert counts.shape == (w,) and (counts % 2 == 0).all(), (xy, h, w, counts)
        assert all(0 <= y <= h for _, y in pts)
        total += len(pts)
    assert total > 1000          # (the cases do cross the images)


def _dist_to_ring(px, py, xy):
    """distance of the points (px, py) to the closed polyline xy"""
    p = np.asarray(xy, np.float64).reshape(-1, 2)
    q = np.roll(p, -1, axis=0)
    best = np.full(px.shape, np.inf)
    for a, b in zip(p, q):
        d = b - a
        L2 = float(d @ d)
        t = np.zeros_like(px) if L2 == 0 else np.clip(((px - a[0]) * d[0] + (py - a[1]) * d[1]) / L2, 0.0, 1.0)
        best = np.minimum(best, np.hypot(px - (a[0] + t * d[0]), py - (a[1] + t * d[1])))
    return best


def test_cross_check_against_pil():
    """PIL.ImageDraw.polygon fills by another rule (and another pixel-centre convention), so the two may differ only along the
    boundary: every pixel they disagree on has its centre or one of its corners within 1.5 px of a polygon edge.  A condition
    on the restatement - the kernel is compared with the restatement exactly."""
    from PIL import Image, ImageDraw
    worst = 0.0
    for xy, h, w in R.random_rings(60, seed=0):
        ref = R.ring_mask(xy, h, w)
        img = Image.new("L", (w, h), 0)
        ImageDraw.Draw(img).polygon([(float(xy[2 * i]), float(xy[2 * i + 1])) for i in range(len(xy) // 2)], fill=1, outline=1)
        pil = np.asarray(img, dtype=np.uint8)
        ys, xs = np.nonzero(ref != pil)
        if ys.size == 0:
            continue
        d = np.full(ys.shape, np.inf)
        for ox, oy in ((0.5, 0.5), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)):
            d = np.minimum(d, _dist_to_ring(xs + ox, ys + oy, xy))
        worst = max(worst, float(d.max()))
    print("restatement vs PIL: farthest disagreeing pixel is", round(worst, 3), "px from an edge")
    assert worst <= 1.5


# ------------------------------------------------------------------------------------------------ argument errors, no device
def _job(ring_off, inst_off, h=16, w=16):
    ro = (C.c_int32 * len(ring_off))(*ring_off)
    io = (C.c_int32 * len(inst_off))(*inst_off)
    j = (L.mi_poly_job * 1)()
    fake = 0x1000                  # stands for device memory: every check below fails before anything is launched
    j[0].verts = j[0].ring_off = j[0].inst_off = j[0].out = fake
    j[0].ring_off_host, j[0].inst_off_host = C.addressof(ro), C.addressof(io)
    j[0].M, j[0].h, j[0].w = len(inst_off) - 1, h, w
    return j, (ro, io)


def test_entry_point_refuses_bad_arguments():
    lib = L.lib()
    with pytest.raises(L.MI355Error, match="args"):
        L.check(lib.mi_polygon_masks(None, 1, None), "mi_polygon_masks")
    j, keep = _job([0, 2], [0, 1])
    with pytest.raises(L.MI355Error, match="< 3"):
        L.check(lib.mi_polygon_masks(j, 1, None), "mi_polygon_masks")
    j, keep = _job([0, 4], [0, 1, 1])
    with pytest.raises(L.MI355Error, match="no ring"):
        L.check(lib.mi_polygon_masks(j, 1, None), "mi_polygon_masks")
    j, keep = _job([0, 4], [0, 1], h=100000)
    with pytest.raises(L.MI355Error, match="LDS"):
        L.check(lib.mi_polygon_masks(j, 1, None), "mi_polygon_masks")
    j, keep = _job([0, 4], [0, 1])
    j[0].out = None
    with pytest.raises(L.MI355Error, match="null"):
        L.check(lib.mi_polygon_masks(j, 1, None), "mi_polygon_masks")


def test_op_refuses_rings_that_are_no_polygons():
    from yolov7_d2_amd import ops
    with pytest.raises(ValueError, match="7 numbers"):
        ops.polygon_masks_batch([[[[1, 1, 5, 1, 5, 5, 1]]]], [(8, 8)], "cuda")
    with pytest.raises(ValueError, match="4 numbers"):
        ops.polygon_masks_batch([[[np.array([1.0, 1.0, 5.0, 5.0])]]], [(8, 8)], "cuda")
    with pytest.raises(ValueError, match="no ring"):
        ops.polygon_masks_batch([[[]]], [(8, 8)], "cuda")
    with pytest.raises(ValueError, match="LIST of rings"):
        ops.polygon_masks_batch([[[1, 1, 5, 1, 5, 5]]], [(8, 8)], "cuda")
    with pytest.raises(ValueError, match="coordinate"):
        ops.polygon_masks_batch([[[[1, 1, 5, 1, float("nan"), 5]]]], [(8, 8)], "cuda")
    with pytest.raises(ValueError, match="sizes"):
        ops.polygon_masks_batch([[]], [], "cuda")
