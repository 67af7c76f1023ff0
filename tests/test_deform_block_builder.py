"""CPU: MODEL.RESNETS.DEFORM_ON_PER_STAGE on detectron2's backbone (build_resnet_backbone) -
sparse_inst_r50_dcn_giam_aug.yaml builds DeformBottleneckBlocks in res4 and res5 with detectron2's state-dict keys, all-False
changes nothing, what is not served is refused by name and the ONNX exporter refuses a DeformConv."""
import os

import pytest
import torch

import ref_loader
import yolov7_d2_amd as M
from yolov7_d2_amd.modeling.resnet import BottleneckBlock, DeformBottleneckBlock, DeformConv

REF_CFG = os.path.join(ref_loader.REF, "configs", "coco", "sparseinst")
ON = [False, False, True, True]


def _cfg(*over):
    path = os.path.join(REF_CFG, "sparse_inst_r50_dcn_giam_aug.yaml")
    if os.path.isfile(path):
        return M.get_yolox_cfg(path, ["MODEL.DEVICE", "cpu", *over])
    cfg = M.sparse_inst_r50_giam_cfg(device="cpu")
    cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = list(ON)
    if over:
        cfg.merge_from_list(list(over))
    return cfg


def test_dcn_yaml_builds_deformable_blocks_in_res4_and_res5_only():
    cfg = _cfg()
    assert cfg.MODEL.BACKBONE.NAME == "build_resnet_backbone" and list(cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE) == ON
    model = M.build_model(cfg)
    bb = model.backbone
    assert type(model).__name__ == "SparseInst" and type(bb).__name__ == "ResNet"
    for name, on, nb in (("res2", False, 3), ("res3", False, 4), ("res4", True, 6), ("res5", True, 3)):
        stage = getattr(bb, name)
        assert len(stage) == nb
        assert all(type(b) is (DeformBottleneckBlock if on else BottleneckBlock) for b in stage), name
        assert all(isinstance(b.conv2, DeformConv) == on for b in stage)
    sd = model.state_dict()
    want = {"res4.0.conv2_offset.weight": (18, 256, 3, 3), "res4.0.conv2_offset.bias": (18,), "res4.0.conv2.weight": (256, 256, 3, 3),
            "res4.0.conv2.norm.weight": (256,), "res4.0.conv2.norm.bias": (256,), "res4.0.conv2.norm.running_mean": (256,),
            "res4.0.conv2.norm.running_var": (256,), "res4.5.conv2_offset.weight": (18, 256, 3, 3),
            "res5.0.conv2_offset.weight": (18, 512, 3, 3), "res5.2.conv2_offset.bias": (18,), "res5.2.conv2.weight": (512, 512, 3, 3),
            "res4.0.conv1.weight": (256, 512, 1, 1), "res4.0.shortcut.weight": (1024, 512, 1, 1), "res5.0.conv3.norm.running_var": (2048,)}
    for k, shp in want.items():
        assert tuple(sd["backbone." + k].shape) == shp, k
    assert not any("conv2_offset" in k for k in sd if ".res2." in k or ".res3." in k)
    assert not any(k.endswith("conv2.bias") or "conv2_offset.norm" in k for k in sd)
    off = [v for k, v in sd.items() if "conv2_offset" in k]
    assert len(off) == 18 and all(float(v.abs().max()) == 0 for v in off)
    # stride on the 3x3 (STRIDE_IN_1X1 False): the first blocks of res4 / res5 carry it on conv2 and conv2_offset
    assert bb.res4[0].conv2.stride == 2 and bb.res4[0].conv2_offset.stride == (2, 2) and bb.res4[1].conv2.stride == 1
    assert bb.stage_modules() == [bb.res2, bb.res3, bb.res4, bb.res5]
    assert all(getattr(b, "input_is_relu", False) for b in bb.res4)
    assert all(p.requires_grad for p in bb.parameters())                  # FREEZE_AT 0
    bb.freeze(4)
    assert not any(p.requires_grad for p in bb.res4.parameters()) and all(p.requires_grad for p in bb.res5.parameters())


def test_all_false_is_exactly_the_model_without_the_key():
    cfg = M.sparse_inst_r50_giam_cfg(device="cpu")
    assert "DEFORM_ON_PER_STAGE" not in cfg.MODEL.RESNETS               # (the package's defaults do not carry the key)
    plain = M.build_model(cfg)
    cfg2 = M.sparse_inst_r50_giam_cfg(device="cpu")
    cfg2.MODEL.RESNETS.DEFORM_ON_PER_STAGE = [False] * 4
    off = M.build_model(cfg2)
    a, b = plain.state_dict(), off.state_dict()
    assert sorted(a) == sorted(b) and all(a[k].shape == b[k].shape for k in a)
    assert [type(m) for m in plain.backbone.modules()] == [type(m) for m in off.backbone.modules()]


def test_refusals_by_name():
    with pytest.raises(NotImplementedError, match="DEFORM_MODULATED"):
        M.build_model(_cfg("MODEL.RESNETS.DEFORM_MODULATED", True))
    with pytest.raises(NotImplementedError, match="DEFORM_NUM_GROUPS"):
        M.build_model(_cfg("MODEL.RESNETS.DEFORM_NUM_GROUPS", 2))
    # neither key matters while no stage is deformable
    cfg = _cfg("MODEL.RESNETS.DEFORM_MODULATED", True)
    cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = [False] * 4
    assert not any(isinstance(m, DeformConv) for m in M.build_backbone(cfg).modules())


def test_export_onnx_refuses_a_deformconv_by_name(tmp_path):
    model = M.build_model(_cfg()).eval()
    with pytest.raises(NotImplementedError, match="DeformConv"):
        M.export_onnx(model, str(tmp_path / "m.onnx"), height=64, width=64)


def test_no_cpu_fallback():
    from yolov7_d2_amd import _lib as L
    blk = DeformBottleneckBlock(64, 128, 32, stride=2)
    with pytest.raises(L.MI355Error):
        blk(torch.zeros(1, 64, 8, 8))
