"""CPU, no device: the C ABI of the COCO evaluator (csrc/coco_eval.hip) - the entry points exist with the declared
signatures, argument errors come back as codes with a text and launch nothing, the Python surface refuses host tensors and
an evaluation without ground truth, and mi_rle_from_string inverts mi_rle_to_string."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import coco_rle_oracle as RO
import yolov7_d2_amd as M
from test_eval_rle import _masks
from yolov7_d2_amd import _lib as L
from yolov7_d2_amd import evaluation as E
from yolov7_d2_amd.d2shim import Boxes, Instances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mi_coco_box_iou", "mi_coco_mask_iou_ws_bytes", "mi_coco_mask_iou", "mi_rle_decode", "mi_rle_from_string", "mi_coco_match",
         "mi_coco_accumulate"]


def _err():
    return L.lib().mi_last_error().decode()


def test_entry_points_and_signatures():
    hdr = open(os.path.join(ROOT, "include", "mi355_det.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = L.lib()
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(lib, name)
        decl = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\((.*?)\)\s*;", hdr, re.S)
        assert decl, name
        res, args = L._PROTOS[name]
        assert res == (C.c_int64 if decl.group(1) == "int64_t" else C.c_int)
        params = [a.strip() for a in decl.group(2).split(",")]
        assert len(params) == len(args), (name, params)
        for par, a in zip(params, args):               # pointers are pointers, int64_t is 64 bits wide, int is int
            if "*" in par or "mi_stream_t" in par:
                assert a in (C.c_void_p, C.c_char_p), (name, par)
            elif par.startswith("int64_t"):
                assert a == C.c_int64, (name, par)
            else:
                assert par.startswith("int ") and a == C.c_int, (name, par)
    assert M.COCOEvaluator is E.COCOEvaluator and M.COCOMaskEvaluator is E.COCOMaskEvaluator


def test_argument_errors_return_codes():
    lib = L.lib()
    p = 4096                                            # non-null dummy: every check comes before a launch
    assert lib.mi_coco_box_iou(None, 3, None, 2, None, None, None) == -1 and "null" in _err()
    assert lib.mi_coco_box_iou(p, -1, p, 2, None, p, None) == -1 and "negative" in _err()
    assert lib.mi_coco_box_iou(None, 0, None, 5, None, None, None) == 0        # nothing to do is no error
    assert lib.mi_coco_mask_iou_ws_bytes(2, 3, 5, 13) == 5 * 2 * 8 and lib.mi_coco_mask_iou_ws_bytes(1, 1, 0, 4) == -1
    assert lib.mi_coco_mask_iou(p, 1, p, 1, 0, 8, None, p, 64, p, p, p, p, None) == -1 and "sizes" in _err()
    assert lib.mi_coco_mask_iou(p, 1, p, 1, 8, 8, None, p, 8, p, p, p, p, None) == -1 and "workspace" in _err()
    assert lib.mi_coco_mask_iou(None, 1, p, 1, 8, 8, None, p, 64, p, p, p, p, None) == -1 and "null" in _err()
    assert lib.mi_coco_mask_iou(p, -2, p, 1, 8, 8, None, p, 64, p, p, p, p, None) == -1
    assert lib.mi_rle_decode(p, p, 1, 0, 8, 8, p, p, p, 1, None) == -1 and "max_runs" in _err()
    assert lib.mi_rle_decode(None, p, 1, 4, 8, 8, p, p, p, 1, None) == -1 and "null" in _err()
    assert lib.mi_rle_decode(p, p, -1, 4, 8, 8, p, p, p, 1, None) == -1 and "sizes" in _err()
    assert lib.mi_rle_decode(p, p, 1, 4, 0, 8, p, p, p, 1, None) == -1
    assert lib.mi_coco_match(p, p, p, None, p, p, p, p, p, 10, p, 4, 100, 5, 3, 3, p, p, p, p, p, None) == -1 and "null" in _err()
    assert lib.mi_coco_match(p, p, p, p, p, p, p, p, p, 65, p, 4, 100, 5, 3, 3, p, p, p, p, p, None) == -1 and "at most 64" in _err()
    assert lib.mi_coco_match(p, p, p, p, p, p, p, p, p, 10, p, 4, 100, 5, -3, 3, p, p, p, p, p, None) == -1
    assert lib.mi_coco_match(p, None, p, p, p, p, p, p, p, 10, p, 4, 100, 5, 3, 3, p, p, p, p, p, None) == -1
    assert lib.mi_coco_accumulate(p, p, p, p, None, p, p, p, 10, 101, 3, 4, 3, 7, p, p, p, None) == -1 and "null" in _err()
    assert lib.mi_coco_accumulate(p, p, p, p, p, p, p, p, 10, 0, 3, 4, 3, 7, p, p, p, None) == -1 and "sizes" in _err()
    assert lib.mi_coco_accumulate(None, p, p, p, p, p, p, p, 10, 101, 3, 4, 3, 7, p, p, p, None) == -1
    buf = (C.c_uint32 * 4)()
    assert lib.mi_rle_from_string(None, buf, 4) == -1 and lib.mi_rle_from_string(b"13", None, 4) == -1
    assert lib.mi_rle_from_string(b"1357", buf, 3) == -1 and "max_runs" in _err()
    assert lib.mi_rle_from_string(b"1X", buf, 4) == -1 and "ends inside" in _err()      # 'X' promises another group


def test_rle_from_string_inverts_to_string():
    lib = L.lib()
    assert E.rle_from_string("13").tolist() == [1, 3] and E.rle_from_string("06").tolist() == [0, 6]
    assert E.rle_from_string("X1").tolist() == [40] and E.rle_from_string("").tolist() == []
    cases = [np.array(c, np.uint32) for c in ([5, 7, 9, 2], [0, 1, 0, 1, 100000, 3], [2 ** 31 - 1], [7, 300, 2, 1, 900, 1])]
    for n, H, W in ((8, 37, 53), (5, 1, 1), (5, 3, 1000)):
        cases += [RO.rle_counts_fast(m) for m in _masks(n, H, W, H * W + n)]
    buf = C.create_string_buffer(7 * max(len(c) for c in cases) + 8)
    for c in cases:
        c = np.ascontiguousarray(c, np.uint32)
        ln = L.check(lib.mi_rle_to_string(c.ctypes.data, len(c), buf, len(buf)), "mi_rle_to_string")
        s = buf.raw[:ln].decode("ascii")
        assert s == RO.rle_to_string(c)
        got = E.rle_from_string(s)
        assert got.dtype == np.uint32 and np.array_equal(got, c) and np.array_equal(got, RO.rle_from_string(s))


def _dataset():
    return {"images": [{"id": 1, "height": 20, "width": 30}], "categories": [{"id": 3, "name": "a"}, {"id": 1, "name": "b"}],
            "annotations": [{"id": 1, "image_id": 1, "category_id": 3, "bbox": [0, 0, 10, 10], "area": 100, "iscrowd": 0,
                             "segmentation": [[0, 0, 10, 0, 10, 10, 0, 10]]}]}


def _instances():
    inst = Instances((20, 30))
    inst.pred_boxes = Boxes(torch.tensor([[0.0, 0.0, 10.0, 10.0]]))
    inst.scores, inst.pred_classes = torch.tensor([0.9]), torch.tensor([1])
    inst.pred_masks = torch.zeros(1, 20, 30, dtype=torch.bool)
    return inst


def test_python_surface_refuses_what_it_cannot_do(tmp_path):
    with pytest.raises(L.MI355Error, match="no ground truth"):
        E.COCOMaskEvaluator().evaluate()
    assert E.COCOMaskEvaluator()._predictions == []
    ev = E.COCOEvaluator(_dataset(), tasks=("bbox", "segm"))
    assert ev._cat_ids == [1, 3] and ev._class_ids == [1, 3] and ev._kmap == [0, 1, 2]
    assert ev.params["iouThrs"][8] == 0.8999999999999999 and len(ev.params["recThrs"]) == 101
    with pytest.raises(L.MI355Error, match="device tensors"):
        ev.process([{"image_id": 1}], [{"instances": _instances()}])
    with pytest.raises(ValueError, match="not in the dataset"):
        ev.process([{"image_id": 2}], [{"instances": _instances()}])
    with pytest.raises(ValueError, match="tasks"):
        E.COCOEvaluator(_dataset(), tasks=("keypoints",))
    import json
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(_dataset()))
    assert E.COCOEvaluator(str(path), class_ids=[3, 1, 9])._kmap == [1, 0, 2, 2]     # a class the dataset lacks is evaluated nowhere
    for fn, args in ((E.coco_box_iou, (torch.zeros(1, 4, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.float64), torch.zeros(1, dtype=torch.uint8))),
                     (E.coco_mask_iou, (torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8))),
                     (E.rle_decode, ([[16]], 4, 4, "cpu"))):
        with pytest.raises(L.MI355Error):
            fn(*args)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_evaluate_fails_loudly_without_device():
    with pytest.raises(L.MI355Error):
        E.COCOEvaluator(_dataset()).evaluate()
