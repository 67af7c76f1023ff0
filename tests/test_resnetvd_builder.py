"""CPU: build_resnet_vd_backbone through the registry - the three r50vd SparseInst YAMLs without deformable convolution
build (from the reference's files where they are on the machine, from the package's SparseInst config with the backbone
name overridden otherwise), what is not served is refused by name, and the ONNX exporter refuses the backbone."""
import os

import pytest
import torch

import ref_loader
import yolov7_d2_amd as M

REF_CFG = os.path.join(ref_loader.REF, "configs", "coco", "sparseinst")
YAMLS = ["sparse_inst_r50vd_base.yaml", "sparse_inst_r50vd_giam.yaml", "sparse_inst_r50vd_giam_aug.yaml"]


def _cfg(name, *over):
    path = os.path.join(REF_CFG, name)
    if os.path.isfile(path):
        return M.get_yolox_cfg(path, ["MODEL.DEVICE", "cpu", *over])
    cfg = M.sparse_inst_r50_giam_cfg(device="cpu")
    cfg.MODEL.BACKBONE.NAME = "build_resnet_vd_backbone"
    if "base" in name:
        cfg.MODEL.SPARSE_INST.DECODER.NAME = "BaseIAMDecoder"
    if over:
        cfg.merge_from_list(list(over))
    return cfg


@pytest.mark.parametrize("name", YAMLS)
def test_r50vd_yaml_builds(name):
    cfg = _cfg(name)
    assert cfg.MODEL.BACKBONE.NAME == "build_resnet_vd_backbone" and "build_resnet_vd_backbone" in M.BACKBONE_REGISTRY
    model = M.build_model(cfg)
    assert type(model).__name__ == "SparseInst" and type(model.backbone).__name__ == "ResNetVD"
    sd = model.state_dict()
    assert "backbone.layer2.0.downsample.1.weight" in sd and "backbone.conv1.4.running_var" in sd
    assert tuple(sd["backbone.conv1.0.weight"].shape) == (32, 3, 3, 3) and tuple(sd["backbone.layer4.2.conv3.weight"].shape) == (2048, 512, 1, 1)
    bb = model.backbone
    assert bb.size_divisibility == 32 and model.size_divisibility == 32
    shp = bb.output_shape()
    assert [(k, v.channels, v.stride) for k, v in shp.items()] == [("res2", 256, 4), ("res3", 512, 8), ("res4", 1024, 16), ("res5", 2048, 32)]
    assert bb.stage_modules() == [bb.layer1, bb.layer2, bb.layer3, bb.layer4]
    assert [len(s) for s in bb.stage_modules()] == [3, 4, 6, 3]
    assert all(p.requires_grad for p in bb.parameters())              # FREEZE_AT is not read: everything trains
    assert isinstance(bb.layer1[0].downsample[0], torch.nn.Identity) and not list(bb.layer2[0].downsample[0].parameters())


def test_depth_101_and_refusals():
    bb = M.build_backbone(_cfg(YAMLS[1], "MODEL.RESNETS.DEPTH", 101))
    assert [len(s) for s in bb.stage_modules()] == [3, 4, 23, 3]
    with pytest.raises(NotImplementedError, match="DEPTH"):
        M.build_backbone(_cfg(YAMLS[1], "MODEL.RESNETS.DEPTH", 34))
    with pytest.raises(NotImplementedError, match="NORM"):
        M.build_model(_cfg(YAMLS[1], "MODEL.RESNETS.NORM", "BN"))
    cfg = _cfg(YAMLS[1])
    cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = [False, False, True, True]
    with pytest.raises(NotImplementedError, match="DEFORM_ON_PER_STAGE"):
        M.build_model(cfg)
    cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = [False] * 4
    assert type(M.build_backbone(cfg)).__name__ == "ResNetVD"


def test_export_onnx_refuses_the_backbone_by_name(tmp_path):
    model = M.build_model(_cfg(YAMLS[1])).eval()
    with pytest.raises(NotImplementedError, match="ResNet-vd"):
        M.export_onnx(model, str(tmp_path / "m.onnx"), height=64, width=64)


def test_no_cpu_fallback():
    from yolov7_d2_amd import _lib as L
    from yolov7_d2_amd.modeling.resnet_vd import ResNetVD
    with pytest.raises(L.MI355Error):
        ResNetVD((1, 1, 1, 1))(torch.zeros(1, 3, 32, 32))
