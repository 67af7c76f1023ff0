"""CPU: the yardstick of the COCO evaluator (tests/cocoeval_ref.py, an unpinned restatement of cocoapi's COCOeval) is itself
checked here against cases worked by hand - the kernels are compared with the restatement exactly (test_gpu_cocoeval.py)."""
import numpy as np

import cocoeval_ref as R


def _ds(boxes, n_images=1, cats=(1,)):
    """boxes: (image_id, category_id, [x, y, w, h], iscrowd) -> COCO dict; area = w * h"""
    anns = [{"id": i + 1, "image_id": im, "category_id": c, "bbox": list(map(float, b)), "area": float(b[2] * b[3]), "iscrowd": crowd}
            for i, (im, c, b, crowd) in enumerate(boxes)]
    return {"images": [{"id": i + 1, "height": 200, "width": 200} for i in range(n_images)], "annotations": anns,
            "categories": [{"id": c, "name": f"c{c}"} for c in cats]}


def _det(im, c, b, s):
    return {"image_id": im, "category_id": c, "bbox": list(map(float, b)), "score": s}


def test_params_are_numpys_own_values():
    p = R.Params()
    assert len(p.iouThrs) == 10 and len(p.recThrs) == 101
    assert p.iouThrs[8] == 0.8999999999999999 and p.iouThrs[8] != 0.9 and p.iouThrs[5] == 0.75 and p.iouThrs[0] == 0.5
    assert p.areaRng == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]


def test_case_1_tp_fp_tp():
    ds = _ds([(1, 1, [0, 0, 10, 10], 0), (1, 1, [20, 20, 10, 10], 0)])
    dets = [_det(1, 1, [0, 0, 10, 10], 0.9), _det(1, 1, [100, 100, 10, 10], 0.8), _det(1, 1, [20, 20, 10, 10], 0.7)]
    ev = R.evaluate(ds, dets)
    e = ev["evalImgs"][0][0][0]
    assert e["dtMatches"].tolist() == [[True, False, True]] * 10 and not e["dtIgnore"].any()
    # precision envelope 1, 2/3, 2/3 at recall 1/2, 1/2, 1: thresholds 0 .. 0.5 (51 of them) read 1, the other 50 read 2/3
    want = 253 / 303
    assert abs(want - (51 + 50 * 2 / 3) / 101) < 1e-15
    s = ev["stats"]
    for i in (0, 1, 2, 3):                                   # AP, AP50, AP75, APs (both ground truths have area 100)
        assert abs(s[i] - want) < 1e-12, (i, s[i])
    assert s[4] == -1 and s[5] == -1                         # APm, APl: no ground truth in those ranges
    assert s[6] == 0.5 and s[7] == 1 and s[8] == 1           # AR@1, AR@10, AR@100
    assert s[9] == 1 and s[10] == -1 and s[11] == -1
    pr = ev["precision"][0, :, 0, 0, 2]
    assert np.allclose(pr[:51], 1, atol=1e-12, rtol=0) and np.allclose(pr[51:], 2 / 3, atol=1e-12, rtol=0)
    assert (ev["scores"][0, :51, 0, 0, 2] == 0.9).all() and (ev["scores"][0, 51:, 0, 0, 2] == 0.7).all()
    r = ev["results"]
    assert abs(r["AP"] - 100 * want) < 1e-10 and np.isnan(r["APm"]) and np.isnan(r["APl"])


def test_case_2_iou_exactly_at_the_threshold_matches():
    ds = _ds([(1, 1, [0, 0, 10, 10], 0)])
    ev = R.evaluate(ds, [_det(1, 1, [0, 0, 10, 5], 0.9)])
    assert R.bb_iou([[0, 0, 10, 5]], [[0, 0, 10, 10]], [0])[0, 0] == 0.5
    e = ev["evalImgs"][0][0][0]
    assert e["dtMatches"][:, 0].tolist() == [True] + [False] * 9
    assert abs(ev["stats"][1] - 1) < 1e-12 and ev["stats"][2] == 0
    assert abs(ev["stats"][0] - 0.1) < 1e-12


def test_case_3_detections_on_a_crowd_are_ignored():
    ds = _ds([(1, 1, [0, 0, 20, 20], 1), (1, 1, [50, 50, 10, 10], 0)])
    dets = [_det(1, 1, [1, 1, 5, 5], 0.95), _det(1, 1, [10, 10, 5, 5], 0.9), _det(1, 1, [50, 50, 10, 10], 0.8)]
    assert R.bb_iou([[1, 1, 5, 5]], [[0, 0, 20, 20]], [1])[0, 0] == 1.0          # crowd: intersection over the DETECTION
    assert R.bb_iou([[1, 1, 5, 5]], [[0, 0, 20, 20]], [0])[0, 0] == 25 / 400
    ev = R.evaluate(ds, dets)
    e = ev["evalImgs"][0][0][0]
    assert e["gtIgnore"].tolist() == [0, 1] and e["gtOrder"].tolist() == [1, 0]      # the crowd goes last
    assert e["dtMatches"].all() and e["dtIgnore"][:, :2].all() and not e["dtIgnore"][:, 2].any()
    assert ev["n_crowd_ignored"] == 2
    assert abs(ev["stats"][0] - 1) < 1e-12 and ev["stats"][8] == 1
    # the same detections without the crowd flag are two false positives in front of the true one
    ds2 = _ds([(1, 1, [0, 0, 20, 20], 0), (1, 1, [50, 50, 10, 10], 0)])
    assert R.evaluate(ds2, dets)["stats"][0] < 0.2


def test_area_on_a_boundary_counts_in_both_ranges():
    ds = _ds([(1, 1, [0, 0, 32, 32], 0)])
    ev = R.evaluate(ds, [_det(1, 1, [0, 0, 32, 32], 0.9)])
    s = ev["stats"]
    assert abs(s[3] - 1) < 1e-12 and abs(s[4] - 1) < 1e-12 and s[5] == -1      # small AND medium, not large
    ds = _ds([(1, 1, [0, 0, 96, 96], 0)])
    s = R.evaluate(ds, [_det(1, 1, [0, 0, 96, 96], 0.9)])["stats"]
    assert s[3] == -1 and abs(s[4] - 1) < 1e-12 and abs(s[5] - 1) < 1e-12


def test_only_the_hundred_best_detections_of_a_cell_enter():
    # the ground truth is found by the detection with the LOWEST of 110 scores: it never enters
    ds = _ds([(1, 1, [0, 0, 10, 10], 0)])
    dets = [_det(1, 1, [100, 100, 5, 5], 0.9 - 0.001 * i) for i in range(109)] + [_det(1, 1, [0, 0, 10, 10], 0.1)]
    ev = R.evaluate(ds, dets)
    assert len(ev["evalImgs"][0][0][0]["dtScores"]) == 100 and ev["stats"][8] == 0 and ev["stats"][0] == 0
    dets[-1]["score"] = 0.85                                  # now it is among them
    assert R.evaluate(ds, dets)["stats"][8] == 1


def test_equal_scores_keep_image_order():
    """image 1: a false positive, image 2: a true positive, same score: the mergesort keeps ascending image_id, so the false
    positive comes first and precision at the only recall step is 1/2 - not 1"""
    ds = _ds([(2, 1, [0, 0, 10, 10], 0)], n_images=2)
    dets = [_det(2, 1, [0, 0, 10, 10], 0.5), _det(1, 1, [50, 50, 10, 10], 0.5)]      # given in the other order
    ev = R.evaluate(ds, dets)
    assert np.allclose(ev["precision"][:, :, 0, 0, 2], 0.5, atol=1e-12, rtol=0)
    ds = _ds([(1, 1, [0, 0, 10, 10], 0)], n_images=2)
    dets = [_det(2, 1, [50, 50, 10, 10], 0.5), _det(1, 1, [0, 0, 10, 10], 0.5)]
    assert np.allclose(R.evaluate(ds, dets)["precision"][:, :, 0, 0, 2], 1, atol=1e-12, rtol=0)


def test_a_category_without_ground_truth_gives_minus_one():
    ds = _ds([(1, 1, [0, 0, 10, 10], 0)], cats=(1, 2))
    ev = R.evaluate(ds, [_det(1, 1, [0, 0, 10, 10], 0.9), _det(1, 2, [0, 0, 10, 10], 0.9)], class_names=["a", "b"])
    assert (ev["precision"][:, :, 1] == -1).all() and (ev["recall"][:, 1] == -1).all() and (ev["scores"][:, :, 1] == -1).all()
    assert abs(ev["stats"][0] - 1) < 1e-12                   # the mean runs over the entries > -1 only
    assert abs(ev["results"]["AP-a"] - 100) < 1e-10 and np.isnan(ev["results"]["AP-b"])


def test_rle_walk_equals_pixel_counts():
    g = np.random.default_rng(0)
    ms = (g.uniform(size=(6, 9, 7)) < 0.4).astype(np.uint8)
    ms[0] = 0
    ms[1] = 1
    crowd = [0, 1, 0, 1, 0, 1]
    want, inter, da, ga = R.mask_iou(ms, ms[::-1], crowd)
    cn = [R.rle_counts(m) for m in ms]
    for d in range(6):
        assert R.rle_area(cn[d]) == da[d] and np.array_equal(R.rle_decode(cn[d], 9, 7), ms[d])
        for k in range(6):
            assert R.rle_iou_pair(cn[d], cn[5 - k], crowd[k]) == want[d, k]
    assert want[0].tolist() == [0] * 6 and want[1, 4] == 1.0          # empty against anything; full against full


def test_segm_uses_pixel_areas_and_mask_iou():
    h = w = 40
    gm = np.zeros((h, w), np.uint8)
    gm[0:10, 0:10] = 1
    ds = {"images": [{"id": 1, "height": h, "width": w}], "categories": [{"id": 1, "name": "a"}],
          "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "iscrowd": 0, "area": 100.0, "bbox": [0, 0, 10, 10],
                           "segmentation": {"size": [h, w], "counts": [int(v) for v in R.rle_counts(gm)]}}]}
    dm = np.zeros((h, w), np.uint8)
    dm[0:10, 0:5] = 1                                          # IoU 50 / 100 exactly
    ev = R.evaluate(ds, [{"image_id": 1, "category_id": 1, "score": 0.9, "mask": dm}], "segm")
    assert abs(ev["stats"][1] - 1) < 1e-12 and ev["stats"][2] == 0
