"""CPU: build_regnet_backbone (yolov7_d2_amd/modeling/regnet.py) through the registry against the independent fp32
restatement of d2's RegNet (tests/regnet_ref.py): state_dict names and shapes, output_shape(), widths / depths / groups for the
three served X types; every Y type is refused by name; the reference's DETR-on-RegNetX YAML merges and builds (where the
reference tree exists); the ONNX exporter refuses the tree by name; no CPU path."""
import os

import pytest
import torch

import regnet_ref as R
import yolov7_d2_amd as M
from yolov7_d2_amd import _lib as L
from yolov7_d2_amd.config import add_yolo_config, get_cfg
from yolov7_d2_amd.modeling import regnet as P

REF_YAML = "/root/reference/configs/coco/detr/detr_256_6_6_regnetx_0.4g.yaml"


def _cfg(kind, out=("s2", "s3", "s4")):
    cfg = add_yolo_config(get_cfg())
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.BACKBONE.NAME = "build_regnet_backbone"
    cfg.MODEL.REGNETS.TYPE = kind
    cfg.MODEL.REGNETS.OUT_FEATURES = list(out)
    return cfg


def test_config_keys_and_registry():
    cfg = add_yolo_config(get_cfg())
    assert cfg.MODEL.REGNETS.TYPE == "x" and list(cfg.MODEL.REGNETS.OUT_FEATURES) == ["s2", "s3", "s4"]     # the reference's defaults
    assert "build_regnet_backbone" in M.BACKBONE_REGISTRY
    assert M.modeling.build_regnet_backbone is P.build_regnet_backbone


@pytest.mark.parametrize("kind", sorted(R.TYPES))
def test_tree_equals_the_restatement(kind):
    bb = M.build_backbone(_cfg(kind))
    ref = R.RegNetRef(kind)
    sd, rd = bb.state_dict(), ref.state_dict()
    assert list(sd) == list(rd)
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in rd.values()]
    assert [v.dtype for v in sd.values()] == [v.dtype for v in rd.values()]
    exp = R.EXPECTED[kind]
    assert bb.widths == exp["widths"] == ref.widths and bb.depths == exp["depths"] == ref.depths
    assert bb.group_widths == [exp["group_width"]] * 4 == ref.group_widths
    shp = bb.output_shape()
    assert list(shp) == ["s2", "s3", "s4"]
    assert [shp[k].channels for k in shp] == exp["widths"][1:] and [shp[k].stride for k in shp] == [8, 16, 32]
    for i, (w, d) in enumerate(zip(exp["widths"], exp["depths"])):
        stage = getattr(bb, "s%d" % (i + 1))
        assert len(list(stage.children())) == d
        assert stage.b1.f.b.groups == w // exp["group_width"] and stage.b1.f.b.stride == (2, 2) and stage.b1.proj is not None
        if d > 1:
            assert stage.b2.proj is None and stage.b2.bn is None and stage.b2.f.b.stride == (1, 1)
    assert all(p.requires_grad for p in bb.parameters())           # freeze_at 0: everything trains
    bn = bb.s2.b1.f.c_bn
    assert bn.eps == 1e-5 and bn.momentum == 0.1 and float(bn.weight.detach().min()) == 1.0 and float(bn.bias.detach().abs().max()) == 0.0
    for k in ("stem.conv.weight", "stem.bn.num_batches_tracked", "s2.b1.proj.weight", "s2.b1.bn.running_var", "s2.b1.f.a.weight",
              "s2.b1.f.a_bn.weight", "s2.b1.f.b.weight", "s2.b1.f.b_bn.bias", "s2.b1.f.c.weight", "s2.b1.f.c_bn.running_mean"):
        assert k in sd, k
    ref.load_state_dict(sd)                                         # and the restatement takes the product's tensors


def test_output_features_and_strides():
    bb = M.build_backbone(_cfg("RegNetX_200MF", out=("stem", "s1", "s2", "s3", "s4")))
    shp = bb.output_shape()
    assert [(k, v.channels, v.stride) for k, v in shp.items()] == [("stem", 32, 2), ("s1", 24, 4), ("s2", 56, 8), ("s3", 152, 16),
                                                                  ("s4", 368, 32)]
    with pytest.raises(AssertionError, match="does not include"):
        M.build_backbone(_cfg("RegNetX_200MF", out=("s5",)))


@pytest.mark.parametrize("kind", sorted(k for k in P.Regnet_types_config if k.startswith("RegNetY")))
def test_every_y_type_is_refused_by_name(kind):
    with pytest.raises(NotImplementedError, match="squeeze") as e:
        M.build_backbone(_cfg(kind))
    gw = P.Regnet_types_config[kind]["group_width"]
    assert ("group width %d" % gw in str(e.value)) == (gw not in (8, 16, 24))


def test_unknown_type_fails_as_the_reference_does():
    assert len(P.Regnet_types_config) == 15
    with pytest.raises(AssertionError, match="type must be one of"):
        M.build_backbone(_cfg("x"))                                   # the config default itself is no type


def test_no_cpu_path():
    bb = M.build_backbone(_cfg("RegNetX_200MF"))
    with pytest.raises(L.MI355Error):
        bb(torch.zeros(1, 3, 32, 32))
    with pytest.raises(L.MI355Error):
        bb.s1.b1(torch.zeros(1, 32, 8, 8))


def test_onnx_export_refuses_the_tree_by_name(tmp_path):
    from yolov7_d2_amd.export_onnx import _NetEmitter
    bb = M.build_backbone(_cfg("RegNetX_200MF"))
    e = object.__new__(_NetEmitter)             # (the refusal comes before the emitter's graph is touched)
    e.g = None
    with pytest.raises(NotImplementedError, match="no emitter for the RegNet backbone"):
        e.resnet(bb, "x", "backbone")


@pytest.mark.skipif(not os.path.isfile(REF_YAML), reason="the reference tree is not on this machine")
def test_reference_detr_regnetx_yaml_merges_and_builds():
    cfg = M.get_yolox_cfg(REF_YAML, ["MODEL.DEVICE", "cpu"])
    assert cfg.MODEL.BACKBONE.NAME == "build_regnet_backbone" and cfg.MODEL.REGNETS.TYPE == "RegNetX_400MF"
    model = M.build_model(cfg)
    assert type(model).__name__ == "Detr" and model.detr.backbone.num_channels == 384
    assert type(model.detr.backbone[0].backbone).__name__ == "RegNet"


def test_one_warning_about_per_rank_statistics_under_data_parallel(monkeypatch):
    """the reference's SyncBN shares batch statistics across ranks; here they are per rank: said once, at build time"""
    import warnings
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    monkeypatch.setattr(P, "_warned_ranks", False)
    with pytest.warns(UserWarning, match="SyncBN"):
        M.build_backbone(_cfg("RegNetX_200MF"))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        M.build_backbone(_cfg("RegNetX_200MF"))                      # once per process
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 1)
    monkeypatch.setattr(P, "_warned_ranks", False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        M.build_backbone(_cfg("RegNetX_200MF"))                      # a single rank: nothing to say
