"""Writes tests/golden/smcadetr_meta.npz from the reference's OWN `SMCADetr` class (yolov7/modeling/meta_arch/smca_detr.py) executed
by path on the CPU in float32, the way oracle/gen_golden.py::gold_detr_meta runs `Detr`: oracle/ref_loader.py's stubs,
resnet_oracle.R50Module standing in for the un-vendored detectron2 build_backbone, the product's d2 shim classes as ImageList /
Instances / Boxes / detector_postprocess, synth_detr_batch() as the batch and seeded_tensor_dict(seed=203) as the weights.
2 encoder + 2 decoder layers, 30 queries, dropout 0, DEEP_SUPERVISION on.

Stored: the sorted state_dict keys and their shapes, the training loss dict and its keys, the eval-mode pred_logits / pred_boxes,
the per-image detections (boxes, scores, classes, in the reference's order) and `points` (layer 0's reference points before
the sigmoid).  Data only; the tests never read the reference.  Needs the reference tree.

    python tools/gen_smcadetr_golden.py
"""
import contextlib
import importlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_loader  # noqa: E402


def load_reference():
    """meta_arch/smca_detr.py by path.  Beyond ref_loader.load_detr()'s stubs it imports alfred.dl.torch.common.device and, through
    detr_seg.py, PIL and panopticapi at module level (neither is touched without MASK_ON)"""
    ref_loader.load()
    ref_loader.load_detr()
    ref_loader._stub("alfred.dl").__path__ = []
    ref_loader._stub("alfred.dl.torch").__path__ = []
    ref_loader._stub("alfred.dl.torch.common", device=torch.device("cpu"))
    if "PIL" not in sys.modules:
        try:
            import PIL.Image  # noqa: F401
        except ImportError:
            ref_loader._stub("PIL", Image=None)
    if "panopticapi" not in sys.modules:
        try:
            import panopticapi.utils  # noqa: F401
        except ImportError:
            ref_loader._stub("panopticapi").__path__ = []
            ref_loader._stub("panopticapi.utils", id2rgb=None, rgb2id=None)
    return importlib.import_module("yolov7.modeling.meta_arch.smca_detr")


def main():
    if not ref_loader.available():
        sys.exit("gen_smcadetr_golden.py: the reference tree is not there")
    import resnet_oracle as R
    from gen_golden_inputs import seeded_tensor_dict, synth_detr_batch
    from yolov7_d2_amd import d2shim, smca_detr_cfg
    smca = load_reference()
    smca.build_backbone = lambda cfg: R.R50Module(50, cfg.MODEL.RESNETS.OUT_FEATURES, cfg.MODEL.RESNETS.STRIDE_IN_1X1)
    smca.ImageList, smca.Instances, smca.Boxes = d2shim.ImageList, d2shim.Instances, d2shim.Boxes
    smca.detector_postprocess = d2shim.detector_postprocess
    smca.device = torch.device("cpu")
    cfg = smca_detr_cfg(device="cpu")
    cfg.MODEL.DETR.ENC_LAYERS, cfg.MODEL.DETR.DEC_LAYERS, cfg.MODEL.DETR.NUM_OBJECT_QUERIES = 2, 2, 30
    cfg.MODEL.DETR.DROPOUT = 0.0
    cfg.MODEL.DETR.DEEP_SUPERVISION = True
    torch.manual_seed(0)
    model = smca.SMCADetr(cfg)
    sd = model.state_dict()
    model.load_state_dict(seeded_tensor_dict({k: v.shape for k, v in sd.items()}, seed=203), strict=False)
    batch = synth_detr_batch()
    inputs = [dict(image=b["image"], instances=d2shim.Instances(b["size"], gt_boxes=d2shim.Boxes(b["boxes"]), gt_classes=b["classes"]))
              for b in batch]
    res = {}
    keys = sorted(sd.keys())
    res["state_keys"] = np.array(keys)
    res["state_shapes"] = np.array([",".join(str(int(n)) for n in sd[k].shape) for k in keys])
    points = {}
    hook = model.detr.transformer.register_forward_hook(lambda m, i, o: points.__setitem__("p", o[1].detach().clone()))
    model.train()
    with contextlib.redirect_stdout(io.StringIO()):
        losses = model(inputs)
    for k, v in losses.items():
        res["loss:" + k] = np.float32(v.detach())
    res["loss_keys"] = np.array(sorted(losses.keys()))
    model.eval()
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        images = model.preprocess_image(inputs)
        out = model.detr(images)
        res["points"] = points["p"].numpy()
        dets = model(inputs)
    hook.remove()
    res["eval_logits"] = out["pred_logits"].numpy()
    res["eval_boxes"] = out["pred_boxes"].numpy()
    res["image_sizes"] = np.array([list(s) for s in images.image_sizes], dtype=np.int64)
    for i, d_ in enumerate(dets):
        inst = d_["instances"]
        res[f"det{i}_boxes"] = inst.pred_boxes.tensor.numpy()
        res[f"det{i}_scores"] = inst.scores.numpy()
        res[f"det{i}_classes"] = inst.pred_classes.numpy()
    path = os.path.join(ROOT, "tests", "golden", "smcadetr_meta.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes;", {k: (v.shape if hasattr(v, "shape") else v) for k, v in res.items() if not k.startswith("state")},
          "losses", {k: float(v.detach()) for k, v in losses.items()}, "ndet", [len(d_["instances"]) for d_ in dets])
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
