"""GPU (-m gpu): the `SMCADetr` meta-architecture end to end - ResNet-50 (res5) + padding mask + sine position encoding + SMCA
transformer + box head tail + focal matcher and criterion + top-100 postprocess - against tests/golden/smcadetr_meta.npz, i.e. the
reference's OWN SMCADetr class executed by path on the CPU in fp32 (tools/gen_smcadetr_golden.py): 2 + 2 layers, 30 queries,
dropout 0, deep supervision.  The detections are held to `inference_torch` on the model's own outputs (pinned to the reference by
tests/test_smcadetr_ref.py): near-uniform bf16 logits reorder the top 100 against the fp32 reference, so parity goes reference ->
inference_torch -> kernel.  Then the training step captured as one hipGraph by GraphedTrainStep, unchanged."""
import os

import numpy as np
import pytest
import torch

import topk_ref as R
import yolov7_d2_amd as M
from yolov7_d2_amd.d2shim import Boxes, Instances
from yolov7_d2_amd.graph_step import GraphedTrainStep
from yolov7_d2_amd.modeling import inference_torch
from gen_golden_inputs import seeded_tensor_dict, synth_detr_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _inputs(batch, dev=None):
    return [dict(image=b["image"] if dev is None else b["image"].to(dev),
                 instances=Instances(b["size"], gt_boxes=Boxes(b["boxes"]), gt_classes=b["classes"])) for b in batch]


def _model(g=None):
    cfg = M.smca_detr_cfg(device=DEV)
    cfg.MODEL.DETR.ENC_LAYERS, cfg.MODEL.DETR.DEC_LAYERS, cfg.MODEL.DETR.NUM_OBJECT_QUERIES = 2, 2, 30
    cfg.MODEL.DETR.DROPOUT = 0.0
    model = M.build_model(cfg)
    sd = model.state_dict()
    if g is not None:
        assert sorted(sd.keys()) == [str(k) for k in g["state_keys"]]          # the reference's own state_dict keys
    model.load_state_dict(seeded_tensor_dict({k: v.shape for k, v in sd.items()}, seed=203), strict=False)
    return model


def test_smcadetr_meta_against_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "smcadetr_meta.npz"))
    model = _model(g)
    inputs = _inputs(synth_detr_batch())
    model.train()
    losses = model(inputs)
    assert sorted(losses.keys()) == [str(k) for k in g["loss_keys"]]
    got = {k: float(v) for k, v in losses.items()}
    print("SMCADetr losses (ours, reference, |dev| / (3e-2 |ref| + 1e-2)):",
          {k: (round(got[k], 4), round(float(g["loss:" + k]), 4), round(abs(got[k] - float(g["loss:" + k])) / (3e-2 * abs(float(g["loss:" + k])) + 1e-2), 3))
           for k in got})
    for k in got:
        ref = float(g["loss:" + k])
        if "error" in k:        # (the reference's SMCADetr.forward returns the weighted entries only: none here)
            assert abs(got[k] - ref) <= 0.1 * abs(ref) + 2.0, (k, got[k], ref)
        else:                   # weighted losses: fp32 reference vs the bf16 network
            assert abs(got[k] - ref) <= 3e-2 * abs(ref) + 1e-2, (k, got[k], ref)
    total = sum(v for k, v in losses.items() if k in model.criterion.weight_dict)
    total.backward()
    trainable = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for n, p in trainable), [n for n, p in trainable if p.grad is None][:5]
    assert all(p.grad is None for n, p in model.named_parameters() if not p.requires_grad)    # stem + res2 frozen
    model.eval()
    with torch.no_grad():
        images = model.preprocess_image(inputs)
        out = model.detr(images)
        dets = model(inputs)
        outs = [(s[0] // 2 + 1, s[1] * 2 - 3) for s in images.image_sizes]     # another output size: scale + clip in the launch
        dets2 = model([dict(x, height=o[0], width=o[1]) for x, o in zip(inputs, outs)])
    lg, bx = out["pred_logits"].float().cpu(), out["pred_boxes"].float().cpu()
    print("SMCADetr eval max abs: logits", float(np.abs(lg.numpy() - g["eval_logits"]).max()), "boxes", float(np.abs(bx.numpy() - g["eval_boxes"]).max()))
    assert np.abs(lg.numpy() - g["eval_logits"]).max() < 0.15 and np.abs(bx.numpy() - g["eval_boxes"]).max() < 2e-2
    # Exactly the restatement's answer (tests/topk_ref.py, held to inference_torch bit for bit by tests/test_smcadetr_ref.py), ties
    # included; and inference_torch's own answer wherever it has only one: the class logits leave the head in bf16, so equal
    # probabilities occur, and torch.topk orders those as it likes
    for d_, o_ in ((dets, None), (dets2, outs)):
        want = inference_torch(lg, bx, images.image_sizes, o_)
        r = R.postprocess(lg.numpy(), bx.numpy(), images.image_sizes, o_ if o_ is not None else images.image_sizes, 100)
        for i, (a, w) in enumerate(zip(d_, want)):
            a = a["instances"]
            keep = (r["boxes"][i][:, 2] - r["boxes"][i][:, 0] > 0) & (r["boxes"][i][:, 3] - r["boxes"][i][:, 1] > 0)
            assert a.image_size == w.image_size and len(a) == int(keep.sum())
            assert np.array_equal(a.pred_classes.numpy(), r["labels"][i][keep])                        # classes and order
            assert np.array_equal(a.pred_boxes.tensor.numpy().view(np.uint32), r["boxes"][i][keep].view(np.uint32))
            x, ref64 = r["logit"][i][keep], r["score64"][i][keep]
            own = torch.sigmoid(torch.from_numpy(x).to(DEV)).cpu().numpy()
            err, bound = float(R.ulp_error(a.scores.numpy(), ref64).max()), max(float(R.ulp_error(own, ref64).max()), 1.0)
            assert err <= bound, (i, err, bound)
            top = torch.sort(lg[i].sigmoid().flatten(), descending=True)[0][:101]
            once = torch.tensor([int((top == v).sum()) == 1 for v in w.scores])
            print(f"image {i}: {int(once.sum())} of {len(w)} detections have a probability of their own; score error {err:.3f} ulp (bound {bound:.3f})")
            if len(a) == len(w) == 100:
                assert torch.equal(a.pred_classes[once], w.pred_classes[once])
                assert torch.equal(a.pred_boxes.tensor[once], w.pred_boxes.tensor[once])
                np.testing.assert_allclose(a.scores.numpy(), w.scores.numpy(), rtol=1e-6, atol=0)


def test_graphed_train_step_serves_smcadetr_unchanged():
    """the captured step's loss dict equals the eager forward_prepared result; two replays on the same batch are bit-identical
    (lr 0: the parameters stay put, dropout 0)"""
    model = _model()
    with torch.no_grad():
        model.detr.input_proj.weight.mul_(1e-3)      # (encoder tokens of trained magnitude, as the DETR graph tests)
    model.train()
    inputs = _inputs(synth_detr_batch(), DEV)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=0.0, weight_decay=1e-4, capturable=True)
    eager = {k: v.detach().clone() for k, v in model.forward_prepared(model.prepare_batch(inputs)).items()}
    assert "total" in eager and set(model.criterion.weight_dict) <= set(eager)
    step = GraphedTrainStep(model, opt)
    try:
        a = {k: v.detach().clone() for k, v in step(inputs).items()}
        b = {k: v.detach().clone() for k, v in step(inputs).items()}
        torch.cuda.synchronize()
        assert len(step.graphs) == 1
        assert sorted(a) == sorted(eager)
        dev_ = {k: float((a[k].float() - eager[k].float()).abs()) for k in eager}
        print("SMCADetr captured vs eager forward_prepared, worst |dev|:", max(dev_, key=dev_.get), max(dev_.values()))
        for k in eager:
            assert torch.equal(a[k], eager[k]), (k, float(a[k]), float(eager[k]))
            assert torch.equal(a[k], b[k]), (k, float(a[k]), float(b[k]))
        assert all(torch.isfinite(v).all() for v in a.values())
    finally:
        step.close()
