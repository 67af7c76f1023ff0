"""The COCO evaluator on the device (csrc/coco_eval.hip, yolov7_d2_amd.evaluation.COCOEvaluator) against its loop-form
restatement tests/cocoeval_ref.py: IoU kernels, RLE decoder and the whole of evaluate -> accumulate -> summarize, EXACTLY -
np.array_equal on float64 and integers, every element, no tolerance: both sides do the same fp64 operations in the same
order (the kernels are built without fma contraction) and everything else is integer."""
import types

import numpy as np
import pytest
import torch

import cocoeval_ref as R
import coco_rle_oracle as RO
import polygon_raster_ref as P
import yolov7_d2_amd as M
from test_eval_rle import _masks
from yolov7_d2_amd import _lib as L
from yolov7_d2_amd import evaluation as E
from yolov7_d2_amd.d2shim import Boxes, Instances

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------------ IoU kernels
def _boxes(n, seed):
    """XYWH doubles: integer and fractional boxes, and a family that touches / nests / misses its neighbours exactly"""
    g = np.random.default_rng(seed)
    b = np.concatenate([g.integers(0, 40, (n, 2)), g.integers(1, 30, (n, 2))], 1).astype(np.float64)
    b[1::3] += g.uniform(0, 1, (len(b[1::3]), 4))
    for k in range(0, n - 1, 5):                       # k + 1 starts where k ends: they touch, w == 0 -> IoU 0
        b[k + 1] = [b[k, 0] + b[k, 2], b[k, 1], 7, b[k, 3]]
    if n > 3:
        b[3] = [500, 500, 4, 4]                        # far from everything
    return b


@pytest.mark.parametrize("G", [0, 1, 7, 130])
@pytest.mark.parametrize("D", [0, 1, 7, 130])
def test_box_iou_equals_the_restatement(D, G):
    dt, gt = _boxes(D, 10 + D), _boxes(G, 10 + G) if G != D else _boxes(G, 10 + D)      # D == G: identical boxes, IoU 1 on the diagonal
    crowd = (np.arange(G) % 3 == 1).astype(np.uint8)
    want = R.bb_iou(dt, gt, crowd)
    got = E.coco_box_iou(_dev(dt), _dev(gt), _dev(crowd)).cpu().numpy()
    assert got.shape == (D, G) and got.dtype == np.float64 and np.array_equal(got, want)
    if D == G == 130:
        whole = (dt == np.round(dt)).all(1)             # (x + w) - x is w only where nothing rounds
        assert whole.sum() > 50 and (np.diag(want)[whole] == 1).all() and (np.diag(want) > 0.999999).all()
        assert (want == 0).sum() > 1000 and ((want > 0) & (want < 1)).sum() > 1000
        k = np.arange(0, 129, 5)
        assert (want[k, k + 1] == 0).all()              # the touching pairs


@pytest.mark.parametrize("H,W", [(1, 1), (37, 53), (64, 64), (65, 129), (480, 640)])
def test_mask_iou_equals_the_restatement(H, W):
    dm, gm = _masks(7, H, W, H + W), _masks(6, H, W, H * W)[::-1].copy()     # empty, full, one pixel, corner pixel, noise, discs
    crowd = np.array([0, 1, 0, 1, 0, 1], np.uint8)
    want = R.mask_iou(dm, gm, crowd)
    got = E.coco_mask_iou(_dev(dm), _dev(gm).bool(), _dev(crowd))
    for a, b in zip(got, want):
        a = a.cpu().numpy()
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert want[2][1] == H * W and want[2][0] == 0
    for D, G in ((0, 6), (7, 0), (0, 0)):
        iou, inter, da, ga = E.coco_mask_iou(_dev(dm[:D]), _dev(gm[:G]), _dev(crowd[:G]))
        assert iou.shape == (D, G) and np.array_equal(da.cpu().numpy(), want[2][:D]) and np.array_equal(ga.cpu().numpy(), want[3][:G])


@pytest.mark.parametrize("n,H,W", [(8, 37, 53), (5, 1, 1), (6, 480, 640), (5, 3, 1000)])
def test_rle_decode_equals_the_masks(n, H, W):
    ms = _masks(n, H, W, H * W + n)                    # [3] begins with a one (empty leading run), [4] is noise (~H*W/2 runs)
    counts = [RO.rle_counts_fast(m) for m in ms]
    assert counts[3][0] == 0 or H * W == 1
    got = E.rle_decode(counts, H, W, DEV).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, ms)
    assert E.rle_decode([], H, W, DEV).shape == (0, H, W)


def test_rle_decode_zero_length_runs_and_bad_counts():
    got = E.rle_decode([[2, 0, 1, 3], [0, 6], [6], [1, 1, 0, 0, 0, 2, 2]], 2, 3, DEV).cpu().numpy()
    want = np.stack([RO.rle_decode(c, 2, 3) for c in ([2, 0, 1, 3], [0, 6], [6], [1, 1, 0, 0, 0, 2, 2])])
    assert np.array_equal(got, want) and got[0].flatten(order="F").tolist() == [0, 0, 0, 1, 1, 1]
    with pytest.raises(L.MI355Error, match="mask 1"):       # an argument error of the launcher, no device-side assert
        E.rle_decode([[6], [2, 3]], 2, 3, DEV)
    assert np.array_equal(E.rle_decode([[6], [2, 3]], 2, 3, DEV, wait=False).cpu().numpy(), np.zeros((2, 2, 3), np.uint8))


# ------------------------------------------------------------------------------------------------------------ end to end
CATS = [2, 3, 5, 8, 11, 13, 21]                          # class index 5 (id 13): no ground truth; 6 (id 21): no detection
NAMES = ["c%d" % c for c in CATS]
SIZES = [(97, 131), (64, 96), (101, 67), (120, 161), (75, 75), (33, 47), (150, 99), (88, 123), (111, 111), (59, 140), (143, 77),
         (70, 101)]


def _rect(x, y, w, h):
    return [float(x), float(y), float(x + w), float(y), float(x + w), float(y + h), float(x), float(y + h)]


def _make_case():
    """12 images, 7 categories.  Image 11 (the 11th) has detections and no ground truth, image 12 ground truth and no
    detection; image 4 has 130 detections, 110 of class 0.  Ground truths are axis-aligned rectangles with sides that are
    multiples of 4 (so the half / three-quarter crops of a copy have IoU exactly 0.5 / 0.75 for boxes and masks), some with a
    second part, some exactly 32 x 32 / 96 x 96 (area on the range bounds), and crowd regions as RLE in both encodings."""
    g = np.random.default_rng(20240611)
    images, anns, per_image = [], [], {}
    for i, (h, w) in enumerate(SIZES):
        img_id = 10 * (i + 1) + 1
        images.append({"id": img_id, "height": h, "width": w})
        gts, dets = [], []                              # dets: (class, score, xyxy float32, mask)
        n_gt = 0 if i == 10 else (30 if i == 3 else int(g.integers(3, 12)))
        for j in range(n_gt):
            c = int(g.choice([0, 1, 2, 3, 4, 6]))
            if j == 0 and min(h, w) >= 97:
                bw = bh = 96
            elif j == 1:
                bw = bh = 32
            else:
                bw, bh = 4 * int(g.integers(1, 9)), 4 * int(g.integers(1, 9))
            x, y = int(g.integers(0, w - bw + 1)), int(g.integers(0, h - bh + 1))
            crowd = int(j % 7 == 5)
            if crowd:
                m = np.zeros((h, w), np.uint8)
                m[y:y + bh, x:x + bw] = 1
                m[y + 1:y + bh:3, x + 1:x + bw:2] = 0                # holes
                cnt = RO.rle_counts_fast(m)
                segm = {"size": [h, w], "counts": RO.rle_to_string(cnt) if j % 2 else [int(v) for v in cnt]}
                area = float(m.sum())
            else:
                rings, area = [_rect(x, y, bw, bh)], float(bw * bh)
                if j % 4 == 2 and x + bw + 6 <= w:                   # a second part, disjoint from the first
                    rings.append(_rect(x + bw + 2, y, 4, 4))
                    area += 16.0
                segm = rings
                m = P.instance_mask(rings, h, w)
                assert int(m.sum()) == int(area)
            anns.append({"id": len(anns) + 1, "image_id": img_id, "category_id": CATS[c], "iscrowd": crowd, "area": area,
                         "bbox": [float(x), float(y), float(bw), float(bh)], "segmentation": segm})
            gts.append((c, x, y, bw, bh, crowd, m))
        sc = lambda: np.float32(int(g.integers(1, 20)) / 20)        # few distinct scores: ties within and across images
        if i != 11:
            for (c, x, y, bw, bh, crowd, m) in gts:
                kind = int(g.integers(0, 6))
                if c == 6:                                           # class 6 is never detected
                    continue
                if crowd:                                            # two detections inside the crowd region
                    for q in range(2):
                        dm = np.zeros_like(m)
                        dm[y:y + bh // 2, x + q * (bw // 2):x + (q + 1) * (bw // 2)] = m[y:y + bh // 2, x + q * (bw // 2):x + (q + 1) * (bw // 2)]
                        dets.append((c, sc(), [x + q * (bw // 2), y, x + (q + 1) * (bw // 2), y + bh // 2], dm))
                elif kind == 0:                                      # a copy
                    dets.append((c, sc(), [x, y, x + bw, y + bh], m.copy()))
                elif kind in (1, 2):                                 # 2:1 / 4:3 crop of a copy: IoU exactly 0.5 / 0.75
                    cw = bw // 2 if kind == 1 else 3 * bw // 4
                    dm = np.zeros_like(m)
                    dm[y:y + bh, x:x + cw] = 1
                    dets.append((c, sc(), [x, y, x + cw, y + bh], dm))
                elif kind == 3:                                      # shifted by a fraction of a pixel / a few pixels, twice
                    for _ in range(2):
                        dx, dy = g.uniform(-3, 3, 2)
                        dm = np.roll(m, (int(round(dy)), int(round(dx))), (0, 1))
                        dets.append((c, sc(), [x + dx, y + dy, x + dx + bw, y + dy + bh], dm))
                elif kind == 4:                                      # the right box under the wrong class
                    dets.append(((c + 1) % 6, sc(), [x, y, x + bw, y + bh], m.copy()))
            for _ in range(int(g.integers(2, 6))):                   # background
                c = int(g.integers(0, 6))
                bw, bh = int(g.integers(2, 30)), int(g.integers(2, 30))
                x, y = int(g.integers(0, w - bw)), int(g.integers(0, h - bh))
                dm = (g.uniform(size=(h, w)) < 0.3).astype(np.uint8)
                dm[:y], dm[y + bh:], dm[:, :x], dm[:, x + bw:] = 0, 0, 0, 0
                dets.append((c, sc(), [x, y, x + bw, y + bh], dm))
            if i == 3:                                               # 130 detections, 110 of them of class 0
                other = [d for d in dets if d[0] != 0][:20]
                while len(other) < 20:
                    other.append((int(g.integers(1, 6)), sc(), [1, 1, 9, 9], np.eye(h, w, dtype=np.uint8)))
                dets = [d for d in dets if d[0] == 0][:110] + other
                g0 = [t for t in gts if t[0] == 0 and not t[5]]
                for q in range(130 - len(dets)):
                    if g0 and q % 9 == 0:                            # further copies of ground truths: duplicates are false positives
                        (c, x, y, bw, bh, crowd, m) = g0[q // 9 % len(g0)]
                        dets.append((0, sc(), [x, y, x + bw, y + bh], m.copy()))
                    else:
                        x, y = int(g.integers(0, w - 8)), int(g.integers(0, h - 8))
                        dm = np.zeros((h, w), np.uint8)
                        dm[y:y + 8, x:x + 8] = 1
                        dets.append((0, sc(), [x, y, x + 8, y + 8], dm))
            order = g.permutation(len(dets))
            dets = [dets[k] for k in order]
        per_image[img_id] = dets
    dataset = {"images": images[::-1], "annotations": anns, "categories": [{"id": c, "name": n} for c, n in zip(CATS, NAMES)][::-1]}
    return dataset, per_image


def _instances(dets, size, boxes=True, masks=True):
    inst = Instances(size)
    n = len(dets)
    if boxes:
        inst.pred_boxes = Boxes(_dev(np.asarray([d[2] for d in dets], np.float32).reshape(n, 4)))
    if masks:
        inst.pred_masks = _dev(np.stack([d[3] for d in dets]).astype(bool) if n else np.zeros((0,) + size, bool))
    inst.scores = _dev(np.asarray([d[1] for d in dets], np.float32))
    inst.pred_classes = _dev(np.asarray([d[0] for d in dets], np.int64))
    return inst


def _ref_results(per_image):
    """what instances_to_coco_json + loadRes hand to COCOeval: XYXY -> XYWH in float32, widened to double"""
    bbox, segm = [], []
    for img_id, dets in per_image.items():
        for c, s, b, m in dets:
            b = np.asarray(b, np.float32).copy()
            b[2] -= b[0]
            b[3] -= b[1]
            bbox.append({"image_id": img_id, "category_id": CATS[c], "score": float(s), "bbox": b.tolist()})
            segm.append({"image_id": img_id, "category_id": CATS[c], "score": float(s), "mask": m})
    return bbox, segm


@pytest.fixture(scope="module")
def case():
    dataset, per_image = _make_case()
    bbox, segm = _ref_results(per_image)
    ref = {"bbox": R.evaluate(dataset, bbox, "bbox", class_names=NAMES),
           "segm": R.evaluate(dataset, segm, "segm", polygon_fn=P.instance_mask, class_names=NAMES)}
    size = {im["id"]: (im["height"], im["width"]) for im in dataset["images"]}
    return types.SimpleNamespace(dataset=dataset, per_image=per_image, ref=ref, size=size)


def _feed(ev, case, batch=5, **kw):
    ids = [i for i in case.per_image if case.per_image[i]]          # image 121 has no detection: it is never processed
    for k in range(0, len(ids), batch):
        chunk = ids[k:k + batch]
        ev.process([{"image_id": i} for i in chunk], [{"instances": _instances(case.per_image[i], case.size[i], **kw)} for i in chunk])


def test_the_fixture_exercises_what_it_should(case):
    """on the restatement's output alone"""
    dets = case.per_image
    assert len(dets) == 12 and len(case.dataset["categories"]) == 7
    n = {i: len(d) for i, d in dets.items()}
    assert n[41] == 130 and sum(1 for d in dets[41] if d[0] == 0) == 110 and n[121] == 0 and n[111] > 0
    gt_imgs = set(a["image_id"] for a in case.dataset["annotations"])
    assert 111 not in gt_imgs and 121 in gt_imgs
    assert max(sum(1 for a in case.dataset["annotations"] if a["image_id"] == i) for i in gt_imgs) == 30
    gt_cats = set(a["category_id"] for a in case.dataset["annotations"])
    det_cls = set(d[0] for ds in dets.values() for d in ds)
    assert 13 not in gt_cats and 21 in gt_cats and 5 in det_cls and 6 not in det_cls
    areas = [a["area"] for a in case.dataset["annotations"]]
    assert 1024.0 in areas and 9216.0 in areas
    assert any(isinstance(a["segmentation"], list) and len(a["segmentation"]) > 1 for a in case.dataset["annotations"])
    enc = set(type(a["segmentation"]["counts"]) for a in case.dataset["annotations"] if a["iscrowd"])
    assert enc == {str, list}
    scores = [float(d[1]) for ds in dets.values() for d in ds]
    assert len(set(scores)) <= 19 < len(scores)
    for task, ref in case.ref.items():
        pr, rc = ref["precision"], ref["recall"]
        for a in range(4):
            for m in range(3):
                assert (pr[:, :, :, a, m] > -1).any() and (rc[:, :, a, m] > -1).any(), (task, a, m)
        assert (pr == -1).any() and (pr[:, :, 5] == -1).all() and (pr[:, :, 6, 0] == 0).all()
        assert ref["n_crowd_ignored"] > 0, task
        assert 0 < ref["stats"][0] < 1 and ref["stats"][6] < ref["stats"][7] <= ref["stats"][8]
        assert ref["stats"][2] < ref["stats"][1]                     # matches that hold at 0.5 and not at 0.75
        # IoUs exactly on thresholds: detections matched at t = 0.5 (0.75) and not at the next threshold
        on = [0, 0]
        for k in range(7):
            for e in ref["evalImgs"][k][0]:
                if e is not None and e["dtMatches"].size:
                    on[0] += int((e["dtMatches"][0] & ~e["dtMatches"][1]).sum())
                    on[1] += int((e["dtMatches"][5] & ~e["dtMatches"][6]).sum())
        assert on[0] > 0 and on[1] > 0, (task, on)


def _assert_equal(ev, task, ref):
    got = ev.eval[task]
    for name in ("precision", "recall", "scores"):
        assert got[name].dtype == np.float64 and got[name].shape == ref[name].shape
        assert np.array_equal(got[name], ref[name]), (task, name, int((got[name] != ref[name]).sum()))
    assert got["counts"] == [10, 101, 7, 4, 3]
    assert np.array_equal(ev.stats[task], ref["stats"])


@pytest.fixture(scope="module")
def evaluated(case):
    ev = E.COCOEvaluator(case.dataset, tasks=("bbox", "segm"), class_names=NAMES)
    _feed(ev, case)
    return ev, ev.evaluate()


def test_end_to_end_equals_the_restatement(case, evaluated):
    ev, res = evaluated
    assert list(res) == ["bbox", "segm"]
    for task in ("bbox", "segm"):
        _assert_equal(ev, task, case.ref[task])
        want = case.ref[task]["results"]
        assert list(res[task])[:6] == ["AP", "AP50", "AP75", "APs", "APm", "APl"] and set(res[task]) == set(want)
        for k, v in want.items():
            assert res[task][k] == v or (np.isnan(v) and np.isnan(res[task][k])), (task, k)
        assert np.isnan(res[task]["AP-c13"]) and res[task]["AP-c21"] == 0


def test_reset_and_a_second_run_give_identical_arrays(case, evaluated):
    ev, _ = evaluated
    first = {t: {k: ev.eval[t][k].copy() for k in ("precision", "recall", "scores")} for t in ("bbox", "segm")}
    ev.reset()
    assert ev.eval == {} and all(not d for d in ev._dets.values())
    _feed(ev, case, batch=3)
    ev.evaluate()
    for t in first:
        for k, v in first[t].items():
            assert np.array_equal(ev.eval[t][k], v)
    with pytest.raises(ValueError, match="twice"):
        _feed(ev, case)


def test_mask_evaluator_with_a_dataset(case, evaluated):
    _, res = evaluated
    plain, full = E.COCOMaskEvaluator(), E.COCOMaskEvaluator(dataset=case.dataset, class_names=NAMES)
    _feed(plain, case)
    _feed(full, case)
    assert plain._predictions == full._predictions and len(plain._predictions) == 11
    with pytest.raises(L.MI355Error, match="no ground truth"):
        plain.evaluate()
    got = full.evaluate()
    assert list(got) == ["bbox", "segm"]
    for t in got:
        assert all(got[t][k] == v or (np.isnan(v) and np.isnan(got[t][k])) for k, v in res[t].items()) and set(got[t]) == set(res[t])
    # one task: the arrays are also at the top of .eval
    one = E.COCOMaskEvaluator(dataset=case.dataset, tasks=("bbox",))
    _feed(one, case, masks=False)
    one.evaluate()
    assert np.array_equal(one.eval["precision"], case.ref["bbox"]["precision"]) and one.eval["counts"] == [10, 101, 7, 4, 3]


def test_after_a_model_forward():
    """SparseInst in eval mode on a 64 x 96 batch (sparseinst_inference_batched): its Instances go into the evaluator as they
    are, and - read back - into the restatement"""
    torch.manual_seed(0)
    cfg = M.sparse_inst_r50_giam_cfg(device=DEV)
    cfg.MODEL.YOLO.CONF_THRESHOLD = 0.005
    model = M.build_model(cfg).eval()
    gen = torch.Generator().manual_seed(1)
    inputs = [dict(image=torch.randint(0, 256, (3, 64, 96), generator=gen).float(), height=64, width=96, image_id=7 - 2 * k)
              for k in range(2)]
    with torch.no_grad():
        out = model(inputs)
    ncls = int(cfg.MODEL.SPARSE_INST.DECODER.NUM_CLASSES)
    dataset = {"images": [{"id": 5, "height": 64, "width": 96}, {"id": 7, "height": 64, "width": 96}],
               "categories": [{"id": c + 1, "name": str(c)} for c in range(ncls)], "annotations": []}
    results = []
    for inp, o in zip(inputs, out):
        inst = o["instances"]
        assert inst.pred_masks.is_cuda and tuple(inst.pred_masks.shape[1:]) == (64, 96) and not inst.has("pred_boxes")
        cls, sc, ms = inst.pred_classes.cpu().numpy(), inst.scores.cpu().numpy(), inst.pred_masks.cpu().numpy().astype(np.uint8)
        for k in range(len(cls)):
            results.append({"image_id": inp["image_id"], "category_id": int(cls[k]) + 1, "score": float(sc[k]), "mask": ms[k]})
        for k in range(0, min(len(cls), 6), 2):                      # ground truth where some predictions are: a box around them
            ys, xs = np.nonzero(ms[k])
            if ys.size:
                x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1
                dataset["annotations"].append({"id": len(dataset["annotations"]) + 1, "image_id": inp["image_id"], "iscrowd": 0,
                                               "category_id": int(cls[k]) + 1, "area": float((x1 - x0) * (y1 - y0)),
                                               "bbox": [x0, y0, x1 - x0, y1 - y0], "segmentation": [_rect(x0, y0, x1 - x0, y1 - y0)]})
    assert len(results) > 0 and len(dataset["annotations"]) > 0
    ev = E.COCOMaskEvaluator(dataset=dataset)
    ev.process(inputs, out)
    res = ev.evaluate()
    assert list(res) == ["segm"] and len(ev._predictions) == 2
    ref = R.evaluate(dataset, results, "segm", polygon_fn=P.instance_mask)
    for name in ("precision", "recall", "scores"):
        assert np.array_equal(ev.eval[name], ref[name]), name
    assert np.array_equal(ev.stats["segm"], ref["stats"]) and (ref["precision"] > 0).any()
