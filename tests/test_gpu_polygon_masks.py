"""Polygon ground truth rasterised on the device (csrc/polygon_masks.hip, ops.polygon_masks_batch, SparseInst.prepare_targets
with INPUT.MASK_FORMAT "polygon") against tests/polygon_raster_ref.py, the numpy restatement of what the reference calls on
the host (meta_arch/sparseinst.py:111-115: BitMasks.from_polygon_masks -> pycocotools' rleFrPoly).  Equality is EXACT
everywhere: the masks byte for byte, the losses bit for bit."""
import functools

import numpy as np
import pytest
import torch

import polygon_raster_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu(polygons, sizes):
    from yolov7_d2_amd import ops
    return ops.polygon_masks_batch(polygons, sizes, DEV)


def _check(polygons, sizes):
    """one call for the batch; every image equal to the restatement"""
    got = _gpu(polygons, sizes)
    assert len(got) == len(sizes)
    for b, (g, insts, (h, w)) in enumerate(zip(got, polygons, sizes)):
        assert g.dtype == torch.uint8 and g.is_cuda and tuple(g.shape) == (len(insts), h, w) and g.is_contiguous()
        want = torch.from_numpy(R.polygon_masks(insts, h, w))
        if not torch.equal(g.cpu(), want):
            bad = (g.cpu() != want).nonzero()
            raise AssertionError(f"image {b} ({h} x {w}): {bad.shape[0]} pixels differ, first (instance, y, x) = {bad[0].tolist()}; "
                                 f"polygons {insts}")
    return got


def _rings_on(h, w, n, seed):
    """n instances of one ring each on an h x w image, the mix of tests/polygon_raster_ref.random_rings at that scale"""
    rng = np.random.default_rng(seed)
    out = []
    for it in range(n):
        k = int(rng.integers(3, 9))
        ang = rng.uniform(0.0, 2.0 * np.pi, k)
        if it % 3 != 1:
            ang = np.sort(ang)
        rad = rng.uniform(0.1, 0.7, k) * max(h, w)
        cx, cy = rng.uniform(0.0, w), rng.uniform(0.0, h)
        xy = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).reshape(-1)
        if it % 3 == 2:
            xy = np.round(xy * 2.0) / 2.0
        out.append([xy])
    return out


def test_random_rings_equal_the_restatement():
    """60 seeded rings (simple, self-intersecting, half-integer; vertices outside the image, negative ones included), each on
    its own image of 8 - 70 pixels a side - one call, more images than one launch takes"""
    cases = R.random_rings(60, seed=0)
    _check([[[xy]] for xy, _, _ in cases], [(h, w) for _, h, w in cases])


def test_sizes_that_divide_neither_the_strip_nor_the_word():
    """33 x 65 and 65 x 33 (h x w): a second strip of one column, a second word of two rows (h + 1 = 34 toggle bits), widths
    that are no multiple of 4 (byte stores); 160 x 224 with 40 instances: several strips, six words per column, many blocks"""
    _check([_rings_on(33, 65, 6, 1), _rings_on(65, 33, 6, 2)], [(33, 65), (65, 33)])
    _check([_rings_on(160, 224, 40, 3)], [(160, 224)])


def _slope_ring(ox, oy):
    """edges whose upsampled steps are (30, 10), (30, 20), (5, 30), (-20, 30), (-50, 10), (5, -100): slopes 1/3, 2/3, 1/6,
    -2/3, 1/5, -1/20 walked over multiples of 3 steps from every residue - s * t lands on exact integers and halves, where
    ys + s * t + 0.5 as a fused multiply-add would round differently"""
    p = np.array([[2, 3], [8, 5], [14, 9], [15, 15], [11, 21], [1, 23]], dtype=np.float64)
    return (p + [ox, oy]).reshape(-1)


def test_special_rings():
    h, w = 40, 36
    base = [3, 3, 20, 4, 18, 22, 5, 19]
    collinear = [2, 2, 10, 10, 20, 20]
    insts = [
        [base + [3, 3]],                                               # first vertex repeated at the end
        [[3, 3, 20, 4, 20, 4, 18, 22, 5, 19]],                         # a repeated interior vertex
        [[3, 3, 3, 3, 20, 4, 18, 22, 18, 22, 18, 22, 5, 19]],          # runs of repeated vertices
        [collinear],                                                   # all vertices on one line
        [[-30, -30, -10, -30, -10, -10]],                              # wholly outside: above and left
        [[w + 5, 2, w + 30, 2, w + 30, 30]],                           # wholly outside: right
        [[2, h + 3, 30, h + 3, 30, h + 20]],                           # wholly outside: below
        [[w - 6, h - 6, w, h - 6, w, h, w - 6, h]],                    # touching x = w and y = h
        [[0, 0, w, 0, w, h, 0, h]],                                    # the whole image
        [[-5, -5, w + 5, -5, w + 5, h + 5, -5, h + 5]],                # more than the whole image
        [[4, 4, 16, 4, 16, 16, 4, 16], [10, 10, 24, 10, 24, 24, 10, 24], [28, 30, 34, 30, 31, 38]],   # a union: overlapping + disjoint
        [[4.5, 4.5, 16.5, 4.5, 16.5, 16.5, 4.5, 16.5]],                # half-integer rectangle
    ]
    insts += [[_slope_ring(ox, oy)] for ox, oy in ((0, 0), (0.2, 0.4), (0.6, 0.8), (-3.4, -2.2), (12.2, 9.6), (20.4, 14.0))]
    got = _check([insts], [(h, w)])[0].cpu()
    assert got[3].sum() == 0                                           # the collinear ring encloses nothing
    assert got[4].sum() == 0 and got[5].sum() == 0 and got[6].sum() == 0
    assert got[7].sum() == 36 and got[7, h - 6:, w - 6:].sum() == 36
    assert got[8].all() and got[9].all()
    a, b, c = (torch.from_numpy(R.ring_mask(r, h, w)) for r in insts[10])
    assert (a & b).any() and not (a & c).any() and torch.equal(got[10], a | b | c) and not torch.equal(got[10], a ^ b ^ c)


def test_batch_of_different_sizes_with_an_empty_image():
    sizes = [(48, 80), (21, 17), (70, 130), (9, 9)]
    polys = [_rings_on(48, 80, 5, 4), [], _rings_on(70, 130, 3, 5), _rings_on(9, 9, 2, 6)]
    polys[0][0] = polys[0][0] + polys[0][1]          # an instance of two rings
    got = _check(polys, sizes)
    assert tuple(got[1].shape) == (0, 21, 17)
    # every image empty: nothing to launch
    got = _gpu([[], []], [(5, 7), (8, 3)])
    assert [tuple(g.shape) for g in got] == [(0, 5, 7), (0, 8, 3)] and all(g.is_cuda for g in got)


def test_two_calls_give_identical_bytes():
    polys, sizes = [_rings_on(160, 224, 24, 7), _rings_on(96, 100, 9, 8)], [(160, 224), (96, 100)]
    a = _gpu(polys, sizes)
    b = _gpu(polys, sizes)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and sum(int(x.sum()) for x in a) > 0


def test_no_host_synchronisation():
    polys, sizes = [_rings_on(64, 64, 4, 9)], [(64, 64)]
    _gpu(polys, sizes)                                # (first call: the page-locked ring is allocated)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = _gpu(polys, sizes)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out[0].cpu(), torch.from_numpy(R.polygon_masks(polys[0], 64, 64)))


# ------------------------------------------------------------------------------------------------ end to end
class _Polygons:
    """what detectron2's PolygonMasks is to prepare_targets: `.polygons`, and .to(device) leaves it alone"""

    def __init__(self, polygons):
        self.polygons = polygons

    def to(self, device):
        return self

    def __len__(self):
        return len(self.polygons)


@functools.lru_cache(maxsize=None)
def _model():
    import yolov7_d2_amd as M
    torch.manual_seed(0)
    cfg = M.sparse_inst_r50_giam_cfg(device=DEV)
    cfg.INPUT.MASK_FORMAT = "polygon"            # what the reference's sparse_inst_r50_giam_aug.yaml sets
    model = M.build_model(cfg)
    assert model.mask_format == "polygon"
    model.train()
    return model


@functools.lru_cache(maxsize=None)
def _e2e_batches():
    """[(polygon inputs, bitmask inputs)]: the same batches - 2 images of about 5 instances - with the ground truth as
    polygons and as the restatement's dense masks; all of one padded shape"""
    from yolov7_d2_amd.d2shim import Instances
    out = []
    for seed, sizes, counts, wrap in ((11, ((192, 224), (160, 200)), (5, 6), False), (12, ((180, 210), (192, 224)), (4, 0), True),
                                      (13, ((170, 224), (192, 200)), (6, 5), True)):
        gen = torch.Generator().manual_seed(seed)
        poly_in, bit_in = [], []
        for k, ((h, w), n) in enumerate(zip(sizes, counts)):
            insts = _rings_on(h, w, n, 100 * seed + k)
            if n >= 2:
                insts[0] = insts[0] + [insts[1][0] * 0.5]            # one instance of two rings
            classes = torch.randint(0, 80, (n,), generator=gen)
            image = torch.randint(0, 256, (3, h, w), generator=gen).float()
            dense = torch.from_numpy(R.polygon_masks(insts, h, w))
            poly_in.append(dict(image=image, height=h, width=w,
                                instances=Instances((h, w), gt_classes=classes, gt_masks=_Polygons(insts) if wrap else insts)))
            bit_in.append(dict(image=image, height=h, width=w, instances=Instances((h, w), gt_classes=classes, gt_masks=dense)))
        out.append((poly_in, bit_in))
    return out


def _same(a, b):
    assert set(a) == set(b) == {"loss_ce", "loss_mask", "loss_dice", "loss_objectness"}
    for k in a:
        assert torch.isfinite(a[k]).all()
        assert torch.equal(a[k].detach(), b[k].detach()), (k, float(a[k]), float(b[k]))


@pytest.mark.parametrize("feed_batch", ["1", "0"])
def test_forward_losses_equal_the_bitmask_losses_bit_for_bit(monkeypatch, feed_batch):
    """MASK_FORMAT "polygon" fed polygons == "bitmask" fed the restatement's masks: everything after the rasteriser is the
    same launches on the same bytes.  With and without the batched feed (MI_FEED_BATCH)."""
    monkeypatch.setenv("MI_FEED_BATCH", feed_batch)
    model = _model()
    poly_in, bit_in = _e2e_batches()[0]
    try:
        model.mask_format = "polygon"
        with torch.no_grad():
            lp = model(poly_in)
        model.mask_format = "bitmask"
        with torch.no_grad():
            lb = model(bit_in)
    finally:
        model.mask_format = "polygon"
    _same(lp, lb)
    assert float(lp["loss_mask"]) > 0


def test_prepare_batch_refilled_in_place_equals_the_bitmask_losses():
    """the host / device split GraphedTrainStep drives: prepare_batch, then two refills IN PLACE with other batches of the same
    padded shape (one image without instances, polygons wrapped in an object with `.polygons`)"""
    model = _model()
    batches = _e2e_batches()
    assert len({model.batch_key(p) for p, _ in batches} | {model.batch_key(b) for _, b in batches}) == 1
    try:
        got, want = [], []
        for fmt, col, res in (("polygon", 0, got), ("bitmask", 1, want)):
            model.mask_format = fmt
            st = None
            for pair in batches:
                st = model.prepare_batch(pair[col], static=st)
                with torch.no_grad():
                    res.append({k: v.clone() for k, v in model.forward_prepared(st).items()})
    finally:
        model.mask_format = "polygon"
    for a, b in zip(got, want):
        _same(a, b)
    assert not torch.equal(got[0]["loss_mask"], got[1]["loss_mask"])       # (the refills did change the targets)


def test_dense_masks_under_polygon_format_are_refused():
    from yolov7_d2_amd.d2shim import Instances
    model = _model()
    try:
        model.mask_format = "polygon"
        inst = Instances((8, 8), gt_classes=torch.zeros(1, dtype=torch.int64), gt_masks=torch.zeros(1, 8, 8))
        with pytest.raises(TypeError, match="polygon"):
            model.prepare_targets([inst])
        empty = model.prepare_targets([Instances((8, 12), gt_classes=torch.zeros(0, dtype=torch.int64), gt_masks=[])])
        assert tuple(empty[0]["masks"].shape) == (0, 8, 12)
    finally:
        model.mask_format = "polygon"
