"""COCO-format evaluation output — drop-in for yolov7/evaluation/coco_evaluation.py:14-100
(`instances_to_coco_json`, `COCOMaskEvaluator.process`): Instances -> list of COCO json dicts, masks as COCO RLE.

The reference encodes every mask on the CPU with pycocotools (`mask_util.encode` on an np.array per mask).  Here the
run-length encoding runs on the GPU (`mi_rle_encode`: one block per mask, column-major scan) and only the run lengths
(a few hundred integers per mask instead of H x W bytes) cross PCIe; the compact ASCII `counts` string is produced by
host code in the same library (`mi_rle_to_string`).  pycocotools is un-vendored (and absent from this image): the byte
format is restated from cocoapi's maskApi.c and checked against an independent numpy restatement + a decoder round trip
(tests/test_gpu_eval.py) - *parity unpinned* against pycocotools itself.

`COCOEvaluator` takes the leg to its number: COCO bbox / segm AP and AR as cocoapi's COCOeval (evaluate -> accumulate ->
summarize) defines them, with IoU, matching and accumulation as HIP kernels (csrc/coco_eval.hip).  This stack has neither
detectron2 nor pycocotools, so the semantics are restated from cocoapi's cocoeval.py / maskApi.c and checked, element for
element, against the loop-form restatement tests/cocoeval_ref.py - again *parity unpinned against pycocotools itself*."""
import ctypes as C
import json
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from .d2shim import Boxes


def rle_encode(masks):
    """masks: bool / uint8 tensor [n, H, W] on the HIP device -> list of {"size": [H, W], "counts": str} (COCO RLE)"""
    if masks.dim() != 3:
        raise ValueError("rle_encode: masks [n, H, W]")
    n, H, W = masks.shape
    if n == 0:
        return []
    if not masks.is_cuda:
        raise L.MI355Error("rle_encode: the MI355X path needs device tensors (no CPU fallback)")
    m = masks.to(torch.uint8).contiguous()
    max_runs = 2048
    while True:
        counts = torch.empty(n, max_runs, dtype=torch.int32, device=m.device)
        nruns = torch.empty(n, dtype=torch.int32, device=m.device)
        L.check(L.lib().mi_rle_encode(m.data_ptr(), n, H, W, max_runs, counts.data_ptr(), nruns.data_ptr(), L.stream_ptr()),
                "mi_rle_encode")
        nr = nruns.cpu().numpy()
        if (nr > 0).all():
            break
        max_runs = int(-nr.min()) + 1          # a very fragmented mask: once more with room for it
    cnt = counts.cpu().numpy().view(np.uint32)
    out, buf = [], C.create_string_buffer(7 * int(nr.max()) + 8)
    for k in range(n):
        row = np.ascontiguousarray(cnt[k, : nr[k]])
        ln = L.check(L.lib().mi_rle_to_string(row.ctypes.data, int(nr[k]), buf, len(buf)), "mi_rle_to_string")
        out.append({"size": [int(H), int(W)], "counts": buf.raw[:ln].decode("ascii")})
    return out


def instances_to_coco_json(instances, img_id):
    """coco_evaluation.py:14-76: an Instances object (boxes optional: SparseInst predicts masks only) -> COCO json dicts"""
    num_instance = len(instances)
    if num_instance == 0:
        return []
    has_box = instances.has("pred_boxes")
    if has_box:
        b = instances.pred_boxes.tensor.detach().float().cpu().numpy().copy()
        b[:, 2] -= b[:, 0]                      # BoxMode.convert(XYXY_ABS -> XYWH_ABS)
        b[:, 3] -= b[:, 1]
        boxes = b.tolist()
    scores = instances.scores.tolist()
    classes = instances.pred_classes.tolist()
    has_mask = instances.has("pred_masks")
    if has_mask:
        rles = rle_encode(instances.pred_masks)
    has_keypoints = instances.has("pred_keypoints")
    if has_keypoints:
        keypoints = instances.pred_keypoints.detach().float().cpu().clone()
    results = []
    for k in range(num_instance):
        result = {"image_id": img_id, "category_id": classes[k], "score": scores[k]}
        if has_box:
            result["bbox"] = boxes[k]
        if has_mask:
            result["segmentation"] = rles[k]
        if has_keypoints:
            keypoints[k][:, :2] -= 0.5          # :66-71: predictions are float coordinates, annotations pixel indices
            result["keypoints"] = keypoints[k].flatten().tolist()
        results.append(result)
    return results


def rle_from_string(s):
    """compressed COCO RLE `counts` string -> run lengths (uint32 ndarray); host code of the library (mi_rle_from_string)"""
    raw = s.encode("ascii") if isinstance(s, str) else bytes(s)
    out = np.empty(max(len(raw), 1), np.uint32)
    n = L.check(L.lib().mi_rle_from_string(raw, out.ctypes.data, len(out)), "mi_rle_from_string")
    return out[:n].copy()


def rle_decode(counts, H, W, device, wait=True):
    """run-length lists (one per mask; column-major runs, first a run of zeros) -> uint8 [n, H, W] of 0 / 1 on `device`
    (mi_rle_decode).  wait=True: a mask whose runs do not sum to H * W raises MI355Error (the call waits for the device);
    wait=False never synchronises - for callers that have checked the sums themselves."""
    device = torch.device(device)
    if device.type != "cuda":
        raise L.MI355Error(f"rle_decode on {device}: the decoder is a HIP kernel (no CPU fallback)")
    n = len(counts)
    out = torch.empty((n, H, W), dtype=torch.uint8, device=device)
    if n == 0:
        return out
    rows = [np.asarray(c, np.int64).ravel() for c in counts]
    if any(r.size and (r.min() < 0 or r.max() >= 1 << 32) for r in rows):
        raise ValueError("rle_decode: a run length outside [0, 2^32)")
    max_runs = max(1, max(r.size for r in rows))
    host = np.zeros((n, max_runs), np.uint32)
    for k, r in enumerate(rows):
        host[k, : r.size] = r
    with torch.cuda.device(device):
        cnt = torch.from_numpy(host.view(np.int32)).to(device)
        nr = torch.tensor([r.size for r in rows], dtype=torch.int32).to(device)
        cum = torch.empty((n, max_runs), dtype=torch.int32, device=device)
        err = torch.empty(n, dtype=torch.int32, device=device)
        L.check(L.lib().mi_rle_decode(cnt.data_ptr(), nr.data_ptr(), n, max_runs, H, W, cum.data_ptr(), out.data_ptr(), err.data_ptr(),
                                      1 if wait else 0, L.stream_ptr()), "mi_rle_decode")
    return out


def coco_box_iou(dt, gt, crowd):
    """dt [D, 4], gt [G, 4] XYWH float64, crowd [G] uint8, all on the device -> IoU [D, G] float64 (maskApi.c bbIou)"""
    D, G = dt.shape[0], gt.shape[0]
    out = torch.empty((D, G), dtype=torch.float64, device=dt.device)
    if not (dt.is_cuda and gt.is_cuda and crowd.is_cuda):
        raise L.MI355Error("coco_box_iou: the MI355X path needs device tensors (no CPU fallback)")
    assert dt.dtype == torch.float64 and gt.dtype == torch.float64 and crowd.dtype == torch.uint8 and crowd.numel() == G
    dt, gt, crowd = dt.contiguous(), gt.contiguous(), crowd.contiguous()
    with torch.cuda.device(dt.device):
        L.check(L.lib().mi_coco_box_iou(dt.data_ptr(), D, gt.data_ptr(), G, crowd.data_ptr(), out.data_ptr(), L.stream_ptr()),
                "mi_coco_box_iou")
    return out


def coco_mask_iou(dm, gm, crowd):
    """dm [D, H, W], gm [G, H, W] uint8 / bool masks, crowd [G] uint8, on the device -> (IoU [D, G] float64, intersections
    [D, G], detection areas [D], ground-truth areas [G] - int64 pixel counts) (maskApi.c rleIou on dense masks)"""
    if not (dm.is_cuda and gm.is_cuda and crowd.is_cuda):
        raise L.MI355Error("coco_mask_iou: the MI355X path needs device tensors (no CPU fallback)")
    if dm.dim() != 3 or gm.dim() != 3 or dm.shape[1:] != gm.shape[1:]:
        raise ValueError(f"coco_mask_iou: masks {tuple(dm.shape)} against {tuple(gm.shape)}")
    D, G, (H, W) = dm.shape[0], gm.shape[0], dm.shape[1:]
    dev = dm.device
    dm = (dm.view(torch.uint8) if dm.dtype == torch.bool else dm.to(torch.uint8)).contiguous()
    gm = (gm.view(torch.uint8) if gm.dtype == torch.bool else gm.to(torch.uint8)).contiguous()
    crowd = crowd.contiguous()
    assert crowd.dtype == torch.uint8 and crowd.numel() == G
    iou = torch.empty((D, G), dtype=torch.float64, device=dev)
    inter = torch.empty((D, G), dtype=torch.int64, device=dev)
    da = torch.empty(D, dtype=torch.int64, device=dev)
    ga = torch.empty(G, dtype=torch.int64, device=dev)
    nbytes = L.lib().mi_coco_mask_iou_ws_bytes(D, G, H, W)
    if nbytes < 0:
        raise ValueError(f"coco_mask_iou: sizes D {D}, G {G}, H {H}, W {W}")
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().mi_coco_mask_iou(dm.data_ptr(), D, gm.data_ptr(), G, H, W, crowd.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                         inter.data_ptr(), da.data_ptr(), ga.data_ptr(), iou.data_ptr(), L.stream_ptr()), "mi_coco_mask_iou")
    return iou, inter, da, ga


class COCOEvaluator:
    """COCO bbox / segm AP and AR on the device - the numbers of cocoapi's COCOeval(cocoGt, cocoGt.loadRes(results), task)
    .evaluate() / .accumulate() / .summarize() as detectron2's COCOEvaluator reports them (Params defaults: ten IoU
    thresholds, 101 recall thresholds, maxDets 1 / 10 / 100, four area ranges, useCats; every image of the dataset counts).

    dataset: a COCO dict (`images`, `annotations`, `categories`) or the path of its JSON.  class_ids[c] is the dataset
    category id of contiguous class c (default: the sorted category ids, detectron2's convention); class_names[c] its name
    for the per-category `AP-<name>` entries.

    `process` computes, per image, the IoU matrix of all detections against all ground truths and the detections' areas ON
    THE DEVICE and keeps only those (dense masks are not held across images); it reads nothing back.  `evaluate` runs
    match -> sort -> accumulate on the device, reads precision / recall / scores back in one transfer and takes the twelve
    means in numpy."""

    METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl")

    def __init__(self, dataset, tasks=("bbox",), class_ids=None, class_names=None):
        if isinstance(dataset, (str, bytes)) or hasattr(dataset, "__fspath__"):
            with open(dataset) as f:
                dataset = json.load(f)
        tasks = tuple(tasks)
        if not tasks or any(t not in ("bbox", "segm") for t in tasks):
            raise ValueError(f"COCOEvaluator: tasks {tasks} (bbox and / or segm; keypoints are not evaluated here)")
        self.tasks = tasks
        self._size = {im["id"]: (int(im["height"]), int(im["width"])) for im in dataset["images"]}
        self._cat_ids = sorted(set(c["id"] for c in dataset["categories"]))
        kof = {c: k for k, c in enumerate(self._cat_ids)}
        K = len(self._cat_ids)
        self._class_ids = list(self._cat_ids if class_ids is None else class_ids)
        self._kmap = [kof.get(c, K) for c in self._class_ids] + [K]         # class index -> category index; K: evaluated nowhere
        self._class_names = None if class_names is None else list(class_names)
        self._gt = {i: [] for i in self._size}
        for ann in dataset["annotations"]:
            if ann["image_id"] in self._gt and ann["category_id"] in kof:
                self._gt[ann["image_id"]].append(ann)
        # cocoeval.py Params.setDetParams: numpy's own values go down as doubles (iouThrs[8] is 0.8999999999999999)
        self.params = {"iouThrs": np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
                       "recThrs": np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
                       "maxDets": [1, 10, 100],
                       "areaRng": [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]],
                       "areaRngLbl": ["all", "small", "medium", "large"], "useCats": 1}
        self.timing = False
        self.reset()

    def reset(self):
        self._dets = {t: {} for t in self.tasks}
        self._device = None
        self.eval = {}
        self.stats = {}
        self.timings = {}                       # task -> {stage: ms} of the last evaluate(), when self.timing is set (tools/)

    # ------------------------------------------------------------------------------------------------------------ process
    def _gt_boxes(self, anns, dev):
        bb = torch.tensor([[float(v) for v in a["bbox"]] for a in anns], dtype=torch.float64).reshape(-1, 4)
        crowd = torch.tensor([int(a.get("iscrowd", 0)) for a in anns], dtype=torch.uint8)
        return bb.to(dev), crowd.to(dev)

    def _gt_masks(self, anns, h, w, dev):
        """annToRLE as dense masks [G, h, w]: polygons rasterised by mi_polygon_masks (the union of an object's parts), crowd
        regions - compressed strings or count lists - decoded by mi_rle_decode"""
        from . import ops
        poly, rle, where = [], [], []
        for a in anns:
            segm = a["segmentation"]
            if isinstance(segm, (list, tuple)):
                where.append((0, len(poly)))
                poly.append([np.asarray(r, np.float64) for r in segm])
            else:
                if [int(v) for v in segm["size"]] != [h, w]:
                    raise ValueError(f"annotation {a.get('id')}: RLE of size {segm['size']} in an image of {(h, w)}")
                cnt = segm["counts"]
                cnt = rle_from_string(cnt) if isinstance(cnt, (str, bytes)) else np.asarray(cnt, np.int64)
                if int(np.asarray(cnt, np.int64).sum()) != h * w:      # checked here, so the decoder need not wait for the device
                    raise ValueError(f"annotation {a.get('id')}: RLE counts sum to {int(cnt.sum())}, the image has {h * w} pixels")
                where.append((1, len(rle)))
                rle.append(cnt)
        pm = ops.polygon_masks_batch([poly], [(h, w)], dev)[0]
        rm = rle_decode(rle, h, w, dev, wait=False)
        if not rle:
            return pm
        if not poly:
            return rm
        idx = torch.tensor([j + (len(poly) if kind else 0) for kind, j in where], dtype=torch.int64).to(dev)
        return torch.cat([pm, rm]).index_select(0, idx)

    def process(self, inputs, outputs):
        for inp, output in zip(inputs, outputs):
            if "instances" not in output:
                continue
            inst, img_id = output["instances"], inp["image_id"]
            if img_id not in self._size:
                raise ValueError(f"COCOEvaluator: image_id {img_id} is not in the dataset")
            scores, classes = inst.scores, inst.pred_classes
            if not (scores.is_cuda and classes.is_cuda):
                raise L.MI355Error("COCOEvaluator.process: the MI355X path needs device tensors (no CPU fallback)")
            dev = scores.device
            self._device = self._device or dev
            anns = self._gt[img_id]
            D, G = len(inst), len(anns)
            for task in self.tasks:
                if img_id in self._dets[task]:
                    raise ValueError(f"COCOEvaluator: image_id {img_id} processed twice")
                field = "pred_boxes" if task == "bbox" else "pred_masks"
                if D and not inst.has(field):
                    raise ValueError(f"COCOEvaluator: task {task} needs instances.{field}")
                rec = {"D": D, "G": G}
                if D:
                    rec["score"] = scores.detach().float().reshape(-1)
                    rec["cls"] = classes.detach().to(torch.int64).reshape(-1)
                    if task == "bbox":
                        b = inst.pred_boxes.tensor.detach().float()
                        if not b.is_cuda:
                            raise L.MI355Error("COCOEvaluator.process: pred_boxes on the host (no CPU fallback)")
                        # instances_to_coco_json: XYXY -> XYWH in float32, then python floats (doubles)
                        xywh = torch.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).double()
                        gb, crowd = self._gt_boxes(anns, dev)
                        rec["iou"] = coco_box_iou(xywh, gb, crowd).reshape(-1)
                        rec["area"] = xywh[:, 2] * xywh[:, 3]                     # loadRes: bb[2] * bb[3]
                    else:
                        m = inst.pred_masks.detach()
                        if not m.is_cuda:
                            raise L.MI355Error("COCOEvaluator.process: pred_masks on the host (no CPU fallback)")
                        h, w = self._size[img_id]
                        if m.dim() != 3 or tuple(m.shape[1:]) != (h, w):
                            raise ValueError(f"COCOEvaluator: pred_masks {tuple(m.shape)} for image {img_id} of {(h, w)}: masks at the "
                                             "image's original size are evaluated")
                        if m.dtype != torch.bool:
                            m = m != 0
                        crowd = torch.tensor([int(a.get("iscrowd", 0)) for a in anns], dtype=torch.uint8).to(dev)
                        iou, _, da, _ = coco_mask_iou(m, self._gt_masks(anns, h, w, dev), crowd)
                        rec["iou"] = iou.reshape(-1)
                        rec["area"] = da.double()                                 # loadRes: maskUtils.area
                self._dets[task][img_id] = rec

    # ----------------------------------------------------------------------------------------------------------- evaluate
    def _gt_tables(self, img_ids):
        """ground truths sorted by (cell = image index * K + category index, annotation order)"""
        K, kof = len(self._cat_ids), {c: k for k, c in enumerate(self._cat_ids)}
        cell, col, area, crowd = [], [], [], []
        for i, img in enumerate(img_ids):
            for c, a in enumerate(self._gt[img]):
                cell.append(i * K + kof[a["category_id"]])
                col.append(c)
                area.append(float(a["area"]))
                crowd.append(int(a.get("iscrowd", 0)))
        cell = np.asarray(cell, np.int64)
        o = np.argsort(cell, kind="stable")
        start = np.searchsorted(cell[o], np.arange(len(img_ids) * K + 1), side="left").astype(np.int64)
        return start, np.asarray(col, np.int32)[o], np.asarray(area, np.float64)[o], np.asarray(crowd, np.uint8)[o]

    def _evaluate_task(self, task, img_ids, dev):
        p, lib = self.params, L.lib()
        T, R, A, M = len(p["iouThrs"]), len(p["recThrs"]), len(p["areaRng"]), len(p["maxDets"])
        K, I = len(self._cat_ids), len(img_ids)
        ncell = I * K
        gt_start, gt_col, gt_area, gt_crowd = self._gt_tables(img_ids)
        Gt = int(gt_col.size)
        recs = [(i, self._dets[task].get(img)) for i, img in enumerate(img_ids)]
        recs = [(i, r) for i, r in recs if r is not None and r["D"] > 0]
        rows, imgs, base = [], [], 0
        for i, r in recs:                                         # shapes only: nothing here waits for the device
            rows.append(base + np.arange(r["D"], dtype=np.int64) * r["G"])
            imgs.append(np.full(r["D"], i, np.int64))
            base += r["D"] * r["G"]
        N = int(sum(r["D"] for _, r in recs))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        f64 = lambda v: up(np.asarray(v, np.float64).reshape(-1))
        marks = []

        def mark(name):
            if self.timing:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append((name, e))
        with torch.cuda.device(dev):
            st = L.stream_ptr()
            mark("")
            if N:
                iou = torch.cat([r["iou"] for _, r in recs]) if base else torch.zeros(1, dtype=torch.float64, device=dev)
                score = torch.cat([r["score"] for _, r in recs]).double()
                cls = torch.cat([r["cls"] for _, r in recs])
                area = torch.cat([r["area"] for _, r in recs])
                ncls = len(self._class_ids)
                k = up(np.asarray(self._kmap, np.int64))[torch.where((cls >= 0) & (cls < ncls), cls, torch.full_like(cls, ncls))]
                cell = torch.where(k < K, up(np.concatenate(imgs)) * K + k, torch.full_like(k, ncell))
                # (cell, -score, stable): the order of computeIoU's argsort(-score, kind='mergesort') inside every cell
                o = torch.sort(score, descending=True, stable=True)[1]
                o = o[torch.sort(cell[o], stable=True)[1]]
                cell, score, area, row = cell[o], score[o], area[o].contiguous(), up(np.concatenate(rows))[o].contiguous()
                det_start = torch.searchsorted(cell, torch.arange(ncell + 1, device=dev)).contiguous()
                rank = (torch.arange(N, device=dev) - det_start[cell]).to(torch.int32)
            else:
                iou = score = area = row = rank = cell = None
                det_start = torch.zeros(ncell + 1, dtype=torch.int64, device=dev)
            dtm = torch.empty((A, T, N), dtype=torch.uint8, device=dev)
            dtig = torch.empty((A, T, N), dtype=torch.uint8, device=dev)
            gtig = torch.empty((A, Gt), dtype=torch.uint8, device=dev)
            gtm = torch.empty((A, T, Gt), dtype=torch.uint8, device=dev)
            npig = torch.zeros((max(ncell, 1), A), dtype=torch.int32, device=dev)
            mark("concat + sort 1")
            d_gs, d_gc, d_ga, d_gw = up(gt_start), up(gt_col), up(gt_area), up(gt_crowd)
            thr, rec, rng = f64(p["iouThrs"]), f64(p["recThrs"]), f64(p["areaRng"])
            L.check(lib.mi_coco_match(L.ptr(iou), L.ptr(row), L.ptr(area), det_start.data_ptr(), d_gs.data_ptr(), d_gc.data_ptr(),
                                      d_ga.data_ptr(), d_gw.data_ptr(), thr.data_ptr(), T, rng.data_ptr(), A, int(p["maxDets"][-1]), ncell, N,
                                      Gt, dtm.data_ptr(), dtig.data_ptr(), gtig.data_ptr(), gtm.data_ptr(), npig.data_ptr(), st),
                    "mi_coco_match")
            mark("mi_coco_match")
            # (category, -score, stable over (image ascending, rank)): accumulate's concatenation + mergesort, once for all maxDets
            if N:
                kk = torch.where(cell < ncell, cell % K, torch.full_like(cell, K))
                o = torch.sort(score, descending=True, stable=True)[1]
                o = o[torch.sort(kk[o], stable=True)[1]]
                dtm2, dtig2 = dtm.index_select(2, o).contiguous(), dtig.index_select(2, o).contiguous()
                score2, rank2 = score[o].contiguous(), rank[o].contiguous()
                cat_start = torch.searchsorted(kk[o].contiguous(), torch.arange(K + 1, device=dev)).contiguous()
            else:
                dtm2 = dtig2 = score2 = rank2 = None
                cat_start = torch.zeros(K + 1, dtype=torch.int64, device=dev)
            npig_ka = npig[:ncell].view(I, K, A).sum(0, dtype=torch.int64).contiguous()
            out = torch.empty(2 * T * R * K * A * M + T * K * A * M, dtype=torch.float64, device=dev)
            n5 = T * R * K * A * M
            md = up(np.asarray(p["maxDets"], np.int32))
            mark("sort 2 + gather")
            L.check(lib.mi_coco_accumulate(L.ptr(dtm2), L.ptr(dtig2), L.ptr(score2), L.ptr(rank2), cat_start.data_ptr(), npig_ka.data_ptr(),
                                           md.data_ptr(), rec.data_ptr(), T, R, K, A, M, N, out.data_ptr(), out[2 * n5:].data_ptr(),
                                           out[n5:].data_ptr(), st), "mi_coco_accumulate")
            mark("mi_coco_accumulate")
            host = out.cpu().numpy()                                # the one read-back
        if self.timing:
            self.timings[task] = OrderedDict((n, a.elapsed_time(b)) for (_, a), (n, b) in zip(marks, marks[1:]))
        ev = {"precision": host[:n5].reshape(T, R, K, A, M), "scores": host[n5:2 * n5].reshape(T, R, K, A, M),
              "recall": host[2 * n5:].reshape(T, K, A, M), "counts": [T, R, K, A, M], "params": p}
        return ev

    def _summarize(self, ev):
        """COCOeval.summarize (_summarizeDets): the twelve stats, in numpy on the host"""
        p = self.params

        def one(ap=1, iouThr=None, areaRng="all", maxDets=100):
            aind = [i for i, a in enumerate(p["areaRngLbl"]) if a == areaRng]
            mind = [i for i, m in enumerate(p["maxDets"]) if m == maxDets]
            s = ev["precision"] if ap == 1 else ev["recall"]
            if iouThr is not None:
                s = s[np.where(iouThr == p["iouThrs"])[0]]
            s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
            return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        md = p["maxDets"]
        calls = [(1, None, "all", md[2]), (1, .5, "all", md[2]), (1, .75, "all", md[2]), (1, None, "small", md[2]),
                 (1, None, "medium", md[2]), (1, None, "large", md[2]), (0, None, "all", md[0]), (0, None, "all", md[1]),
                 (0, None, "all", md[2]), (0, None, "small", md[2]), (0, None, "medium", md[2]), (0, None, "large", md[2])]
        return np.array([one(*c) for c in calls], np.float64)

    def _derive(self, stats, ev):
        """detectron2's _derive_coco_results"""
        res = {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(self.METRICS)}
        if self._class_names is not None:
            K = len(self._cat_ids)
            for c, name in enumerate(self._class_names):
                k = self._kmap[c] if c < len(self._class_ids) else K
                pr = ev["precision"][:, :, k, 0, -1] if k < K else np.zeros(0)
                pr = pr[pr > -1]
                res["AP-" + name] = float(np.mean(pr) * 100) if pr.size else float("nan")
        return res

    def evaluate(self, img_ids=None):
        """-> OrderedDict(task -> {"AP", "AP50", "AP75", "APs", "APm", "APl" (x 100, NaN where undefined) [, "AP-<name>"]});
        self.eval[task] keeps precision / recall / scores / counts / params, self.stats[task] the twelve stats.  With one
        task, self.eval is also that task's dict itself (self.eval["precision"] ...)."""
        L.require_device()
        dev = self._device or torch.device("cuda", torch.cuda.current_device())
        ids = sorted(set(self._size if img_ids is None else img_ids))
        for i in ids:
            if i not in self._size:
                raise ValueError(f"COCOEvaluator.evaluate: image_id {i} is not in the dataset")
        results, self.eval, self.stats = OrderedDict(), {}, {}
        for task in self.tasks:
            ev = self._evaluate_task(task, ids, dev)
            self.eval[task] = ev
            self.stats[task] = self._summarize(ev)
            results[task] = self._derive(self.stats[task], ev)
        if len(self.tasks) == 1:
            self.eval.update(self.eval[self.tasks[0]])
        return results


class COCOMaskEvaluator:
    """the `process` override of coco_evaluation.py:79-100: collects {"image_id", "instances": [json dicts]} per image.
    The base class's dataset loading and COCOeval are detectron2's; here, given `dataset` (a COCO dict or the path of its
    JSON), `process` also feeds a COCOEvaluator and `evaluate()` returns its AP dict.  tasks=None: bbox and / or segm after
    the fields of the first instances seen (detectron2's _tasks_from_predictions)."""

    def __init__(self, dataset=None, tasks=None, class_ids=None, class_names=None):
        self._predictions = []
        self._dataset, self._tasks, self._class_ids, self._class_names = dataset, tasks, class_ids, class_names
        self._coco = None
        if dataset is not None and tasks is not None:
            self._coco = COCOEvaluator(dataset, tasks, class_ids, class_names)

    def reset(self):
        self._predictions = []
        if self._coco is not None:
            self._coco.reset()

    def process(self, inputs, outputs):
        for inp, output in zip(inputs, outputs):
            prediction = {"image_id": inp["image_id"]}
            if "instances" in output:
                prediction["instances"] = instances_to_coco_json(output["instances"], inp["image_id"])
            if "proposals" in output:
                prediction["proposals"] = output["proposals"]
            if len(prediction) > 1:
                self._predictions.append(prediction)
        if self._dataset is None:
            return
        if self._coco is None:
            inst = next((o["instances"] for o in outputs if "instances" in o), None)
            if inst is None:
                return
            tasks = tuple(t for t, f in (("bbox", "pred_boxes"), ("segm", "pred_masks")) if inst.has(f))
            self._coco = COCOEvaluator(self._dataset, tasks, self._class_ids, self._class_names)
        self._coco.process(inputs, outputs)

    def evaluate(self, img_ids=None):
        if self._dataset is None:
            raise L.MI355Error("COCOMaskEvaluator.evaluate: no ground truth was given (COCOMaskEvaluator(dataset=...)); "
                               "process() only collects the COCO json predictions")
        if self._coco is None:
            raise L.MI355Error("COCOMaskEvaluator.evaluate: no instances were processed, so there is no task to evaluate")
        res = self._coco.evaluate(img_ids)
        self.eval, self.stats = self._coco.eval, self._coco.stats
        return res
