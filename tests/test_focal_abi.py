"""CPU, no device: the C ABI and the module surface of the focal matcher / set criterion - the new names are exported by the
library, declared in include/mi355_det.h and bound in _lib.py; the descriptor's ctypes layout is the compiled one; argument
errors are returned before anything is launched; the criteria's state_dict keys are the reference's."""
import ctypes as C
import os
import re

import pytest
import torch

from yolov7_d2_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mi_hungarian_match_focal", "mi_focal_set_loss_fwd", "mi_focal_set_loss_bwd", "mi_focal_loss_desc_sizeof")


def test_new_names_are_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mi355_det.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in L.EXPORTS, n
    assert "typedef struct mi_focal_loss_desc" in hdr


def test_descriptor_layout_is_the_compiled_one():
    """mi_abi_sizeof's id list is closed (15 is mi_bnx and 16 is pinned to "unknown" by tests/test_abi_and_config.py), so the
    new struct has its own self-check entry"""
    assert L.lib().mi_focal_loss_desc_sizeof() == C.sizeof(L.mi_focal_loss_desc)
    assert C.sizeof(L.mi_focal_loss_desc) == C.sizeof(L.mi_detr_loss_desc)        # the sibling's fields, alpha for eos_coef
    assert [f[0] for f in L.mi_focal_loss_desc._fields_] == [("alpha" if f[0] == "eos_coef" else f[0]) for f in L.mi_detr_loss_desc._fields_]


def _desc():
    d = L.mi_focal_loss_desc()
    for f in ("logits", "boxes", "tgt_labels", "tgt_boxes", "tgt_off", "match_q", "match_t", "nmatch", "losses", "rowstate"):
        setattr(d, f, 4096)       # non-null dummies: a refused call never touches memory
    d.B, d.Q, d.NC, d.gmax, d.alpha, d.num_boxes = 2, 5, 1, 1, 0.25, 1.0
    return d


@pytest.mark.parametrize("field,value,word", [("logits", None, b"null"), ("rowstate", None, b"null"), ("B", 0, b"B 0"), ("B", 257, b"B 257"),
                                              ("Q", 0, b"Q 0"), ("NC", 0, b"NC 0"), ("gmax", 0, b"gmax 0"), ("num_boxes", 0.0, b"num_boxes")])
def test_fill_refuses_bad_descriptors_before_launching(field, value, word):
    lib = L.lib()
    d = _desc()
    setattr(d, field, value)
    assert lib.mi_focal_set_loss_fwd(C.byref(d), None) != 0 and word in lib.mi_last_error()
    assert lib.mi_focal_set_loss_bwd(C.byref(d), 4096, 4096, 4096, None) != 0 and word in lib.mi_last_error()


def test_backward_and_matcher_refuse_null_and_oversize():
    lib = L.lib()
    assert lib.mi_focal_set_loss_bwd(C.byref(_desc()), None, 4096, 4096, None) != 0 and b"null" in lib.mi_last_error()
    assert lib.mi_focal_set_loss_fwd(None, None) != 0
    a = [4096] * 5
    assert lib.mi_hungarian_match_focal(*a, 1, 1025, 3, 4, 1.0, 1.0, 1.0, 0.25, 4096, 4096, 4096, 4096, None) != 0 and b"1025" in lib.mi_last_error()
    assert lib.mi_hungarian_match_focal(*a, 1, 10, 3, 1025, 1.0, 1.0, 1.0, 0.25, 4096, 4096, 4096, 4096, None) != 0
    assert lib.mi_hungarian_match_focal(*a, 1, 10, 3, 4, 1.0, 1.0, 1.0, 0.25, None, 4096, 4096, 4096, None) != 0 and b"null" in lib.mi_last_error()


def test_state_dicts_and_constructors_are_the_reference_s():
    from yolov7_d2_amd.modeling import (FocalSetCriterion, HungarianMatcher, HungarianMatcherAnchorDETR, HungarianMatcherFocal,
                                        HungarianMatcherSMCA, SetCriterion, SMCASetCriterion)
    assert HungarianMatcherSMCA is HungarianMatcherFocal and HungarianMatcherAnchorDETR is HungarianMatcherFocal
    m = HungarianMatcherFocal(cost_class=2, cost_bbox=5, cost_giou=2)
    assert isinstance(m, HungarianMatcher) and (m.cost_class, m.cost_bbox, m.cost_giou) == (2, 5, 2)
    with pytest.raises(AssertionError):
        HungarianMatcherFocal(0, 0, 0)
    s = SMCASetCriterion(80, m, {"loss_ce": 2}, 0.1, ["labels", "boxes", "cardinality"])
    sd = s.state_dict()
    assert list(sd) == ["empty_weight"] and tuple(sd["empty_weight"].shape) == (81,) and float(sd["empty_weight"][-1]) == pytest.approx(0.1)
    assert s.focal_alpha == 0.25 and isinstance(s, FocalSetCriterion) and isinstance(s, SetCriterion)
    f = FocalSetCriterion(91, m, {"loss_ce": 2}, ["labels", "boxes"], focal_alpha=0.3)
    assert len(f.state_dict()) == 0 and list(f.parameters()) == [] and list(f.buffers()) == [] and f.focal_alpha == 0.3
    assert FocalSetCriterion(91, m, {}, ["labels"]).focal_alpha == 0.25
    for mk in (lambda: FocalSetCriterion(91, m, {}, ["labels", "masks"]), lambda: SMCASetCriterion(91, m, {}, 0.1, ["masks"])):
        with pytest.raises(NotImplementedError):
            mk()
    with pytest.raises(L.MI355Error):            # host tensors: no CPU fallback
        f({"pred_logits": torch.zeros(1, 4, 91), "pred_boxes": torch.zeros(1, 4, 4)}, [{"labels": torch.zeros(0, dtype=torch.int64), "boxes": torch.zeros(0, 4)}])
