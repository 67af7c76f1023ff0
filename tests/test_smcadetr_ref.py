"""CPU, no device: the `SMCADetr` meta-architecture's host side.  `inference_torch` - the plain-torch restatement of the
reference's inference + detector_postprocess, the yardstick of the GPU tests - reproduces the detections of
tests/golden/smcadetr_meta.npz (the reference's OWN SMCADetr class run by path, tools/gen_smcadetr_golden.py); the numpy
restatement of the kernel (tests/topk_ref.py) agrees with it bit for bit; the model builds on the CPU with the reference's state
keys and shapes; smcadetr_origin.yaml merges where the reference tree is present; the refused configurations raise by name; the
new entry points are exported, declared and bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ref_loader
import topk_ref as R
import yolov7_d2_amd as M
from yolov7_d2_amd import _lib as L
from yolov7_d2_amd.modeling import smca_detr as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mi_focal_topk_postprocess", "mi_box_ref_sigmoid_fwd", "mi_box_ref_sigmoid_bwd")
REF_YAML = "/root/reference/configs/coco/detr/smcadetr_origin.yaml"


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "smcadetr_meta.npz"))


def _fixture_cfg(device="cpu"):
    cfg = M.smca_detr_cfg(device=device)
    cfg.MODEL.DETR.ENC_LAYERS, cfg.MODEL.DETR.DEC_LAYERS, cfg.MODEL.DETR.NUM_OBJECT_QUERIES = 2, 2, 30
    cfg.MODEL.DETR.DROPOUT = 0.0
    return cfg


def test_inference_torch_reproduces_the_reference_detections(gold):
    sizes = [tuple(int(v) for v in s) for s in gold["image_sizes"]]
    dets = S.inference_torch(torch.from_numpy(gold["eval_logits"]), torch.from_numpy(gold["eval_boxes"]), sizes)
    assert len(dets) == len(sizes)
    for i, inst in enumerate(dets):
        assert np.array_equal(inst.pred_classes.numpy(), gold[f"det{i}_classes"])         # classes and order
        np.testing.assert_allclose(inst.scores.numpy(), gold[f"det{i}_scores"], rtol=1e-6, atol=0)
        np.testing.assert_allclose(inst.pred_boxes.tensor.numpy(), gold[f"det{i}_boxes"], rtol=1e-6, atol=0)
        assert inst.image_size == sizes[i]


@pytest.mark.parametrize("out", [None, "smaller", "larger"])
def test_numpy_restatement_equals_inference_torch(gold, out):
    """tests/topk_ref.py against the torch yardstick on logits whose probabilities are pairwise distinct (asserted): same entries
    in the same order, boxes bit-equal, torch's fp32 scores at the float64 sigmoid to fp32 rounding"""
    lg, bx = R.distinct_logits(2, 30, 80, seed=11), R.random_boxes(2, 30, seed=12)
    sizes = [(97, 131), (120, 75)]
    outs = {None: None, "smaller": [(h // 3 + 1, w // 2 + 3) for h, w in sizes], "larger": [(h * 2 + 1, w * 3 - 2) for h, w in sizes]}[out]
    prob = torch.from_numpy(lg).sigmoid().flatten(1)
    assert all(len(torch.unique(p)) == p.numel() for p in prob)
    dets = S.inference_torch(torch.from_numpy(lg), torch.from_numpy(bx), sizes, outs)
    ref = R.postprocess(lg, bx, sizes, outs if outs is not None else sizes, 100)
    for i, inst in enumerate(dets):
        b = ref["boxes"][i]
        keep = ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
        assert np.array_equal(inst.pred_classes.numpy(), ref["labels"][i][keep])
        assert np.array_equal(inst.pred_boxes.tensor.numpy().view(np.uint32), b[keep].view(np.uint32))
        np.testing.assert_allclose(inst.scores.numpy(), ref["score64"][i][keep], rtol=1e-6, atol=0)     # (torch's own fp32 sigmoid)


def test_key_order_and_ties_of_the_restatement():
    x = np.array([[[0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1.0, -1.0, -np.nan, 5e-45, -5e-45]]], np.float32)
    assert R.select(x, 11)[0].tolist() == [4, 8, 2, 5, 6, 9, 0, 1, 10, 7, 3]
    v, i = torch.topk(torch.from_numpy(x).flatten(1), 2)                    # torch.topk: NaN greatest
    assert torch.isnan(v).all()


def test_smcadetr_builds_on_the_cpu_with_the_reference_state_dict(gold):
    model = M.build_model(_fixture_cfg())
    assert type(model).__name__ == "SMCADetr" and M.META_ARCH_REGISTRY.get("SMCADetr") is S.SMCADetr
    sd = model.state_dict()
    assert sorted(sd.keys()) == [str(k) for k in gold["state_keys"]]
    shapes = {str(k): tuple(int(n) for n in str(s).split(",") if n) for k, s in zip(gold["state_keys"], gold["state_shapes"])}
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes
    assert tuple(model.detr.class_embed.weight.shape) == (80, 256)
    assert float(model.detr.class_embed.bias[0].detach()) == pytest.approx(S.bias_init_with_prob(0.01)) == pytest.approx(-4.59511985)
    wd = model.criterion.weight_dict
    assert wd == {"loss_ce": 2, "loss_bbox": 5.0, "loss_giou": 2.0, "loss_ce_0": 2, "loss_bbox_0": 5.0, "loss_giou_0": 2.0}
    assert model.criterion.matcher.cost_class == 1 and model.criterion.losses == ["labels", "boxes", "cardinality"]
    assert all(l.dynamic_scale == "type3" for l in model.detr.transformer.decoder.layers)
    assert model.detr.backbone[0].feature_strides == [32] and model.detr.backbone.num_channels == [2048]
    with pytest.raises(L.MI355Error):           # no CPU fallback
        model([dict(image=torch.zeros(3, 32, 32))])


@pytest.mark.skipif(not (ref_loader.available() and os.path.exists(REF_YAML)), reason="the reference tree is not on this machine")
def test_smcadetr_origin_yaml_merges_and_equals_smca_detr_cfg():
    cfg = M.get_yolox_cfg(REF_YAML, ["MODEL.DEVICE", "cpu"])
    own = M.smca_detr_cfg(device="cpu")
    assert cfg.MODEL.META_ARCHITECTURE == "SMCADetr" and cfg.MODEL.DETR.NUM_OBJECT_QUERIES == 300
    for sec in ("DETR", "RESNETS", "YOLO"):
        assert dict(cfg.MODEL[sec]) == dict(own.MODEL[sec]), sec
    assert cfg.MODEL.PIXEL_MEAN == own.MODEL.PIXEL_MEAN and cfg.MODEL.PIXEL_STD == own.MODEL.PIXEL_STD and cfg.MODEL.MASK_ON is False
    assert cfg.SOLVER.IMS_PER_BATCH == own.SOLVER.IMS_PER_BATCH == 16 and cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE == "full_model"
    assert cfg.SOLVER.LR_MULTIPLIER_OVERWRITE == own.SOLVER.LR_MULTIPLIER_OVERWRITE
    assert cfg.INPUT.CROP.TYPE == own.INPUT.CROP.TYPE == "absolute_range" and cfg.INPUT.FORMAT == own.INPUT.FORMAT == "RGB"
    model = M.build_model(cfg)
    assert type(model).__name__ == "SMCADetr" and len(model.detr.transformer.decoder.layers) == 6
    assert tuple(model.detr.query_embed.weight.shape) == (300, 256)


@pytest.mark.parametrize("key,value,word", [("MODEL.MASK_ON", True, "MASK_ON"), ("MODEL.DETR.NUM_FEATURE_LEVELS", 3, "NUM_FEATURE_LEVELS"),
                                            ("MODEL.DETR.PRE_NORM", True, "PRE_NORM")])
def test_refused_configurations_raise_by_name(key, value, word):
    cfg = _fixture_cfg()
    cfg.merge_from_list([key, value])
    with pytest.raises(NotImplementedError, match=word):
        M.build_model(cfg)


def test_new_names_are_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mi355_det.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in L.EXPORTS, n
    from yolov7_d2_amd import modeling
    for n in ("SMCADetr", "SMCADETR", "focal_topk_postprocess", "box_ref_sigmoid", "inference_torch"):
        assert hasattr(modeling, n), n
    assert hasattr(M, "smca_detr_cfg") and hasattr(M, "SMCADetr")


def test_kernels_refuse_bad_arguments_before_launching():
    lib = L.lib()
    a = [4096] * 4          # non-null dummies: a refused call never touches memory
    o = [4096] * 4
    assert lib.mi_focal_topk_postprocess(*a, 1, 3, 40, 121, *o, None) != 0 and b"K 121 > Q * C" in lib.mi_last_error()
    assert lib.mi_focal_topk_postprocess(*a, 1, 300, 91, 1025, *o, None) != 0 and b"1025" in lib.mi_last_error()
    assert lib.mi_focal_topk_postprocess(*a, 1, 1 << 16, 1 << 15, 100, *o, None) != 0 and b"2^31" in lib.mi_last_error()
    assert lib.mi_focal_topk_postprocess(*a, 1, 3, 40, 0, *o, None) != 0
    assert lib.mi_focal_topk_postprocess(None, 4096, 4096, None, 1, 3, 40, 10, *o, None) != 0 and b"null" in lib.mi_last_error()
    assert lib.mi_box_ref_sigmoid_fwd(None, 4096, 4096, 1, 1, 1, None) != 0 and b"null" in lib.mi_last_error()
    assert lib.mi_box_ref_sigmoid_fwd(4096, 4096, 4096, 0, 1, 1, None) != 0
    assert lib.mi_box_ref_sigmoid_bwd(4096, 4096, 4096, 4096, None, 1, 1, 1, None) != 0 and b"null" in lib.mi_last_error()
    with pytest.raises(L.MI355Error):           # host tensors: no CPU fallback
        S.focal_topk_postprocess(torch.zeros(1, 3, 4), torch.zeros(1, 3, 4), torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(L.MI355Error):
        S.box_ref_sigmoid(torch.zeros(1, 1, 3, 4), torch.zeros(1, 3, 2))
