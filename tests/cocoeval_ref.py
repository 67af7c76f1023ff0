"""YARDSTICK (test infrastructure, not product): a plain numpy / float64 restatement, in loop form, of cocoapi's COCO
evaluation - PythonAPI/pycocotools/cocoeval.py `COCOeval.evaluate` (`_prepare`, `computeIoU`, `evaluateImg`), `accumulate`,
`summarize`, the parts of coco.py `loadRes` / `annToRLE` they depend on, and common/maskApi.c `bbIou`, `rleIou`, `rleArea`,
`rleFrString`, `rleDecode` - with detectron2's `_derive_coco_results` on top.  pycocotools is an un-vendored dependency of
the reference and absent here: *parity unpinned against pycocotools itself* - the algorithm is restated from the published
source, and tests/test_cocoeval_ref.py checks it against cases worked by hand.

It imports nothing from yolov7_d2_amd.  Ids: cocoapi tests `gtm > 0` / `dtm == 0` on annotation ids, which it can because
COCO ids start at 1; matched-ness is a boolean here.

A detection is {"image_id", "category_id", "score", and "bbox": [x, y, w, h] (bbox) or "mask": uint8 [H, W] (segm)}."""
from collections import defaultdict

import numpy as np


# ------------------------------------------------------------------------------------------------------------ Params
class Params:
    """cocoeval.py Params.setDetParams"""

    def __init__(self):
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ["all", "small", "medium", "large"]
        self.useCats = 1


# ------------------------------------------------------------------------------------------------------------ maskApi.c
def bb_iou(dt, gt, iscrowd):
    """bbIou: dt [D, 4], gt [G, 4] XYWH float64 -> [D, G]"""
    dt, gt = np.asarray(dt, np.float64).reshape(-1, 4), np.asarray(gt, np.float64).reshape(-1, 4)
    o = np.zeros((len(dt), len(gt)), np.float64)
    for g in range(len(gt)):
        G = gt[g]
        ga = G[2] * G[3]
        crowd = bool(iscrowd[g])
        for d in range(len(dt)):
            D = dt[d]
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else da + ga - i
            o[d, g] = i / u
    return o


def rle_counts(mask):
    """rleEncode: mask [H, W] -> run lengths of the column-major scan, starting with a run of zeros"""
    m = (np.asarray(mask) != 0).astype(np.int8).flatten(order="F")
    starts = np.concatenate([[0], np.flatnonzero(np.diff(np.concatenate([[0], m])) != 0)])
    return np.diff(np.concatenate([starts, [m.size]])).astype(np.int64)


def rle_from_string(s):
    """rleFrString"""
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return np.array(cnts, dtype=np.int64)


def rle_decode(cnts, H, W):
    """rleDecode: -> uint8 [H, W]"""
    assert int(np.sum(cnts)) == H * W, (int(np.sum(cnts)), H, W)
    m = np.zeros(H * W, dtype=np.uint8)
    p, v = 0, 0
    for c in cnts:
        m[p:p + int(c)] = v
        p += int(c)
        v = 1 - v
    return m.reshape((H, W), order="F")


def rle_area(cnts):
    """rleArea: the odd runs"""
    return int(sum(int(c) for c in cnts[1::2]))


def rle_iou_pair(a, b, crowd):
    """rleIou for one pair of run-length lists, the merge walk of maskApi.c (its bounding-box shortcut only skips pairs
    whose intersection is empty, which give i == 0 -> 0 here as well)"""
    a, b = [int(v) for v in a], [int(v) for v in b]
    ka, kb = len(a), len(b)
    ca, cb, va, vb = a[0], b[0], 0, 0
    ia, ib, i, u, ct = 1, 1, 0, 0, 1
    while ct > 0:
        c = min(ca, cb)
        if va or vb:
            u += c
            if va and vb:
                i += c
        ct = 0
        ca -= c
        if not ca and ia < ka:
            ca = a[ia]
            ia += 1
            va = 1 - va
        ct += ca
        cb -= c
        if not cb and ib < kb:
            cb = b[ib]
            ib += 1
            vb = 1 - vb
        ct += cb
    if i == 0:
        u = 1
    elif crowd:
        u = rle_area(a)
    return float(i) / float(u)


def mask_iou(dm, gm, iscrowd):
    """rleIou on dense masks dm [D, H, W], gm [G, H, W]: the same integers i, |d|, |g| counted on pixels
    -> (iou [D, G] float64, inter [D, G], darea [D], garea [G])"""
    dm, gm = np.asarray(dm) != 0, np.asarray(gm) != 0
    D, G = len(dm), len(gm)
    da = dm.reshape(D, -1).sum(1).astype(np.int64)
    ga = gm.reshape(G, -1).sum(1).astype(np.int64)
    inter = np.zeros((D, G), np.int64)
    o = np.zeros((D, G), np.float64)
    for d in range(D):
        for g in range(G):
            i = int(np.count_nonzero(dm[d] & gm[g]))
            inter[d, g] = i
            if i == 0:
                u = 1
            elif iscrowd[g]:
                u = int(da[d])
            else:
                u = int(da[d]) + int(ga[g]) - i
            o[d, g] = float(i) / float(u)
    return o, inter, da, ga


def ann_to_mask(ann, h, w, polygon_fn=None):
    """coco.py annToRLE + decode: polygons (the union of the parts: frPyObjects + merge), an uncompressed RLE (counts a list)
    or a compressed one (counts a string).  polygon_fn(rings, h, w) -> uint8 [h, w] rasterises; it is the caller's
    (tests/polygon_raster_ref.instance_mask restates rleFrPoly)."""
    segm = ann["segmentation"]
    if isinstance(segm, list):
        return polygon_fn(segm, h, w)
    cnts = segm["counts"]
    cnts = rle_from_string(cnts if isinstance(cnts, str) else cnts.decode("ascii")) if isinstance(cnts, (str, bytes)) else np.asarray(cnts, np.int64)
    assert [int(v) for v in segm["size"]] == [h, w]
    return rle_decode(cnts, h, w)


# ------------------------------------------------------------------------------------------------------------ COCOeval
def evaluate_img(gt, dt, ious, aRng, maxDet, p):
    """COCOeval.evaluateImg for one (image, category, area range).  gt: list of {"area", "iscrowd"}; dt: list of {"score",
    "area"} ALREADY in computeIoU's order (score descending, stable, cut to maxDets[-1]); ious [len(dt), len(gt)] in those
    orders.  -> None, or dtMatches / dtIgnore [T, D] (bool), gtIgnore [G], dtScores [D]"""
    if len(gt) == 0 and len(dt) == 0:
        return None
    g_ig = [1 if (g["ignore"] or g["area"] < aRng[0] or g["area"] > aRng[1]) else 0 for g in gt]
    gtind = np.argsort(g_ig, kind="mergesort")          # sort dt highest score first, sort gt ignore last
    gt = [gt[i] for i in gtind]
    dt = dt[0:maxDet]
    iscrowd = [int(o["iscrowd"]) for o in gt]
    ious = ious[:, gtind] if len(ious) > 0 else ious
    T, G, D = len(p.iouThrs), len(gt), len(dt)
    gtm, dtm = np.zeros((T, G), bool), np.zeros((T, D), bool)
    gtIg = np.array([g_ig[i] for i in gtind])
    dtIg = np.zeros((T, D), bool)
    if not len(ious) == 0:
        for tind, t in enumerate(p.iouThrs):
            for dind, d in enumerate(dt):
                iou = min([t, 1 - 1e-10])            # information about best match so far (m=-1 -> unmatched)
                m = -1
                for gind, g in enumerate(gt):
                    if gtm[tind, gind] and not iscrowd[gind]:      # if this gt already matched, and not a crowd, continue
                        continue
                    if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:  # if dt matched to reg gt, and on ignore gt, stop
                        break
                    if ious[dind, gind] < iou:                     # continue to next gt unless better match made
                        continue
                    iou = ious[dind, gind]                         # if match successful and best so far, store appropriately
                    m = gind
                if m == -1:
                    continue
                dtIg[tind, dind] = gtIg[m]
                dtm[tind, dind] = True
                gtm[tind, m] = True
    a = np.array([d["area"] < aRng[0] or d["area"] > aRng[1] for d in dt], bool).reshape((1, len(dt)))
    dtIg = np.logical_or(dtIg, np.logical_and(~dtm, np.repeat(a, T, 0)))       # set unmatched detections outside of area range to ignore
    return {"dtMatches": dtm, "dtIgnore": dtIg, "gtIgnore": gtIg, "dtScores": [d["score"] for d in dt], "gtOrder": gtind}


def accumulate(evalImgs, p, K, I):
    """COCOeval.accumulate.  evalImgs[k][a][i] as evaluate_img returned them (images ascending)"""
    T, R, A, M = len(p.iouThrs), len(p.recThrs), len(p.areaRng), len(p.maxDets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        for a in range(A):
            for m, maxDet in enumerate(p.maxDets):
                E = [e for e in evalImgs[k][a] if e is not None]
                if len(E) == 0:
                    continue
                dtScores = np.concatenate([e["dtScores"][0:maxDet] for e in E])
                inds = np.argsort(-dtScores, kind="mergesort")
                dtScoresSorted = dtScores[inds]
                dtm = np.concatenate([e["dtMatches"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                dtIg = np.concatenate([e["dtIgnore"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                gtIg = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gtIg == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q, ss = np.zeros((R,)), np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds2 = np.searchsorted(rc, p.recThrs, side="left")
                    try:
                        for ri, pi in enumerate(inds2):
                            q[ri] = pr[pi]
                            ss[ri] = dtScoresSorted[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    return precision, recall, scores


def summarize(precision, recall, p):
    """COCOeval.summarize / _summarizeDets: the twelve stats"""
    def _s(ap=1, iouThr=None, areaRng="all", maxDets=100):
        aind = [i for i, aR in enumerate(p.areaRngLbl) if aR == areaRng]
        mind = [i for i, mD in enumerate(p.maxDets) if mD == maxDets]
        s = precision if ap == 1 else recall
        if iouThr is not None:
            s = s[np.where(iouThr == p.iouThrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    stats = np.zeros((12,))
    stats[0] = _s(1)
    stats[1] = _s(1, iouThr=.5, maxDets=p.maxDets[2])
    stats[2] = _s(1, iouThr=.75, maxDets=p.maxDets[2])
    stats[3] = _s(1, areaRng="small", maxDets=p.maxDets[2])
    stats[4] = _s(1, areaRng="medium", maxDets=p.maxDets[2])
    stats[5] = _s(1, areaRng="large", maxDets=p.maxDets[2])
    stats[6] = _s(0, maxDets=p.maxDets[0])
    stats[7] = _s(0, maxDets=p.maxDets[1])
    stats[8] = _s(0, maxDets=p.maxDets[2])
    stats[9] = _s(0, areaRng="small", maxDets=p.maxDets[2])
    stats[10] = _s(0, areaRng="medium", maxDets=p.maxDets[2])
    stats[11] = _s(0, areaRng="large", maxDets=p.maxDets[2])
    return stats


def derive_results(stats, precision, class_names=None):
    """detectron2 COCOEvaluator._derive_coco_results (bbox / segm)"""
    names = ["AP", "AP50", "AP75", "APs", "APm", "APl"]
    res = {n: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, n in enumerate(names)}
    if class_names is not None:
        for idx, name in enumerate(class_names):
            pr = precision[:, :, idx, 0, -1]
            pr = pr[pr > -1]
            res["AP-" + name] = float(np.mean(pr) * 100) if pr.size else float("nan")
    return res


def evaluate(dataset, results, iou_type="bbox", polygon_fn=None, img_ids=None, class_names=None):
    """the whole of COCOeval(cocoGt, cocoGt.loadRes(results), iou_type): evaluate(); accumulate(); summarize()
    -> dict(precision, recall, scores, stats, results, evalImgs, n_crowd_ignored)"""
    p = Params()
    imgs = {im["id"]: im for im in dataset["images"]}
    imgIds = sorted(set(imgs if img_ids is None else img_ids))
    catIds = sorted(set(c["id"] for c in dataset["categories"]))
    gts, dts = defaultdict(list), defaultdict(list)
    for ann in dataset["annotations"]:                       # _prepare
        g = dict(ann)
        g["ignore"] = int("iscrowd" in g and g["iscrowd"])
        g["iscrowd"] = int(g.get("iscrowd", 0))
        gts[g["image_id"], g["category_id"]].append(g)
    for r in results:                                        # loadRes
        assert r["image_id"] in imgs
        d = dict(r)
        if iou_type == "bbox":
            bb = [float(v) for v in d["bbox"]]
            d["bbox"], d["area"] = bb, bb[2] * bb[3]
        else:
            d["area"] = int(np.count_nonzero(d["mask"]))
        d["score"] = float(d["score"])
        dts[d["image_id"], d["category_id"]].append(d)
    K, A = len(catIds), len(p.areaRng)
    evalImgs = [[[] for _ in range(A)] for _ in range(K)]
    n_crowd_ignored = 0
    for k, catId in enumerate(catIds):
        for imgId in imgIds:
            gt, dt = gts[imgId, catId], dts[imgId, catId]
            inds = np.argsort([-d["score"] for d in dt], kind="mergesort")        # computeIoU
            dt = [dt[i] for i in inds][0:p.maxDets[-1]]
            iscrowd = [g["iscrowd"] for g in gt]
            if len(gt) == 0 or len(dt) == 0:
                ious = np.zeros((0,))                        # maskUtils.iou returns [] when either side is empty
            elif iou_type == "bbox":
                ious = bb_iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], iscrowd)
            else:
                h, w = imgs[imgId]["height"], imgs[imgId]["width"]
                gm = np.stack([ann_to_mask(g, h, w, polygon_fn) for g in gt])
                ious = mask_iou(np.stack([d["mask"] for d in dt]), gm, iscrowd)[0]
            for a in range(A):
                e = evaluate_img(gt, dt, ious, p.areaRng[a], p.maxDets[-1], p)
                evalImgs[k][a].append(e)
                if a == 0 and e is not None and len(gt) and len(dt):
                    n_crowd_ignored += int(np.logical_and(e["dtMatches"][0], e["dtIgnore"][0]).sum())
    precision, recall, scores = accumulate(evalImgs, p, K, len(imgIds))
    stats = summarize(precision, recall, p)
    return {"precision": precision, "recall": recall, "scores": scores, "stats": stats, "params": p, "evalImgs": evalImgs,
            "results": derive_results(stats, precision, class_names), "n_crowd_ignored": n_crowd_ignored}
