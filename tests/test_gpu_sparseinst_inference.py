"""The batched SparseInst inference postprocess (csrc/sparseinst_infer.hip, sparseinst_inference_batched,
SparseInst.inference_batched) against the reference's own `inference` outputs (golden sparseinst_inference.npz) and against
the per-image loop (SparseInst.inference) on the same device, with the tolerances of
test_gpu_sparseinst.py::test_sparseinst_inference_against_reference_golden: kept set and classes exact, scores rtol 2e-5 /
atol 1e-7, mask mismatch share < 1e-4, area difference <= 3."""
import os
import types

import numpy as np
import pytest
import torch

import yolov7_d2_amd as M
from yolov7_d2_amd.d2shim import Instances
from yolov7_d2_amd.modeling import sparseinst as S
from gen_golden_inputs import synth_sparseinst_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = np.load(os.path.join(golden_dir, "sparseinst_inference.npz"))
    out = {k: torch.from_numpy(g[k]).to(DEV) for k in ("pred_logits", "pred_scores", "pred_masks")}
    return types.SimpleNamespace(
        g=g, out=out, cls_thr=float(g["cls_threshold"]), mask_thr=float(g["mask_threshold"]),
        out_sizes=[tuple(int(v) for v in s) for s in g["out_sizes"]], image_sizes=[tuple(int(v) for v in s) for s in g["image_sizes"]],
        max_shape=tuple(int(v) for v in g["max_shape"]))


def _stub(gold, cls_thr=None, mask_thr=None):
    return types.SimpleNamespace(cls_threshold=gold.cls_thr if cls_thr is None else cls_thr,
                                 mask_threshold=gold.mask_thr if mask_thr is None else mask_thr)


def _nhwc_form(out, Np=64):
    """the decoder's form of the same prediction: masks bf16 [B, h, w, Np], query = channel, garbage beyond the N queries -
    and the bf16-rounded masks as fp32 NCHW for the loop"""
    B, N, h, w = out["pred_masks"].shape
    gen = torch.Generator().manual_seed(5)
    nhwc = (torch.randn(B, h, w, Np, generator=gen) * 3 + 1).to(DEV, torch.bfloat16)
    nhwc[..., :N] = out["pred_masks"].permute(0, 2, 3, 1).to(torch.bfloat16)
    assert (nhwc[..., N:] != 0).all()
    rounded = nhwc[..., :N].permute(0, 3, 1, 2).float().contiguous()
    return dict(out, _masks_nhwc=nhwc, pred_masks=nhwc.permute(0, 3, 1, 2)[:, :N]), dict(out, pred_masks=rounded)


def _compare(got, ref, what=""):
    """got / ref: lists of Instances"""
    assert len(got) == len(ref)
    for b, (r, o) in enumerate(zip(got, ref)):
        assert tuple(r.image_size) == tuple(o.image_size)
        assert r.scores.dtype == torch.float32 and r.pred_classes.dtype == torch.int64
        assert r.scores.shape == o.scores.shape and np.array_equal(r.pred_classes.cpu().numpy(), o.pred_classes.cpu().numpy())
        np.testing.assert_allclose(r.scores.cpu().numpy(), o.scores.cpu().numpy(), rtol=2e-5, atol=1e-7)
        assert r.has("pred_masks") == o.has("pred_masks")
        if not o.has("pred_masks"):
            assert r.scores.numel() == 0 and r.pred_classes.numel() == 0
            continue
        a, c = r.pred_masks.cpu().numpy(), o.pred_masks.cpu().numpy()
        assert a.shape == c.shape and a.dtype == np.bool_
        mism = float((a != c).mean())
        darea = int(np.abs(a.reshape(len(a), -1).sum(1).astype(np.int64) - c.reshape(len(c), -1).sum(1)).max())
        print(f"{what} image {b}: {len(a)} kept -> {a.shape[1:]}, mask mismatch share {mism:.2e}, area difference {darea}")
        assert mism < 1e-4 and darea <= 3


def _golden_instances(gold):
    res = []
    for b, size in enumerate(gold.out_sizes):
        masks = np.unpackbits(gold.g[f"masks{b}"], axis=-1)[..., : size[1]].astype(bool)
        assert np.array_equal(masks.reshape(len(masks), -1).sum(1), gold.g[f"mask_area{b}"])
        res.append(Instances(size, pred_masks=torch.from_numpy(masks), scores=torch.from_numpy(gold.g[f"scores{b}"]),
                             pred_classes=torch.from_numpy(gold.g[f"classes{b}"])))
    return res


def test_golden_both_input_forms(gold):
    inputs = [dict(height=h, width=w) for h, w in gold.out_sizes]
    stub = _stub(gold)
    got = M.SparseInst.inference_batched(stub, gold.out, inputs, gold.max_shape, gold.image_sizes)
    _compare(got, _golden_instances(gold), "fp32 NCHW vs golden:")
    nhwc, rounded = _nhwc_form(gold.out)
    got = M.SparseInst.inference_batched(stub, nhwc, inputs, gold.max_shape, gold.image_sizes)
    ref = M.SparseInst.inference(stub, rounded, inputs, gold.max_shape, gold.image_sizes)
    _compare(got, ref, "bf16 NHWC vs loop:")
    # the function itself, without `_masks_nhwc`: the strided bf16 `pred_masks` view is read in place as well
    view = {k: v for k, v in nhwc.items() if k != "_masks_nhwc"}
    got2 = S.sparseinst_inference_batched(view, gold.image_sizes, gold.out_sizes, gold.max_shape, gold.cls_thr, gold.mask_thr)
    for a, c in zip(got, got2):
        assert torch.equal(a.scores, c.scores) and torch.equal(a.pred_masks, c.pred_masks)


@pytest.mark.parametrize("size", [(8, 10), (13, 7), (400, 333), (201, 251), None], ids=str)
@pytest.mark.parametrize("form", ["fp32", "bf16"])
def test_against_loop_at_other_output_sizes(gold, size, form):
    """(8, 10) / (13, 7): the whole source plane lies behind one tile - the global-tap path; (400, 333) / (201, 251): the LDS
    stage, tile edges on neither axis; None: no height / width, the output is the image size"""
    inputs = [dict() if size is None else dict(height=size[0], width=size[1]) for _ in gold.image_sizes]
    stub = _stub(gold)
    fast, slow = _nhwc_form(gold.out) if form == "bf16" else (gold.out, gold.out)
    got = M.SparseInst.inference_batched(stub, fast, inputs, gold.max_shape, gold.image_sizes)
    ref = M.SparseInst.inference(stub, slow, inputs, gold.max_shape, gold.image_sizes)
    if size is None:
        assert [tuple(r.image_size) for r in got] == gold.image_sizes
    _compare(got, ref, f"{form} -> {size}:")


def test_single_image_batch(gold):
    out = {k: v[1:] for k, v in gold.out.items()}
    inputs, sizes = [dict(height=80, width=100)], gold.image_sizes[1:]
    got = M.SparseInst.inference_batched(_stub(gold), out, inputs, gold.max_shape, sizes)
    _compare(got, M.SparseInst.inference(_stub(gold), out, inputs, gold.max_shape, sizes), "B = 1:")


def test_image_without_kept_query(gold):
    """image 0 keeps nothing, image 1 everything: counts, offsets, and the Instances without pred_masks"""
    out = dict(gold.out, pred_logits=gold.out["pred_logits"].clone())
    out["pred_logits"][0] = -20.0                     # (image 1 of the golden keeps all its 40 queries as it is)
    inputs = [dict(height=h, width=w) for h, w in gold.out_sizes]
    for o in (out, _nhwc_form(out)[0]):
        got = M.SparseInst.inference_batched(_stub(gold), o, inputs, gold.max_shape, gold.image_sizes)
        assert len(got) == 2 and not got[0].has("pred_masks") and got[0].scores.numel() == 0
        assert got[1].pred_masks.shape == (40,) + gold.out_sizes[1]
    ref = M.SparseInst.inference(_stub(gold), out, inputs, gold.max_shape, gold.image_sizes)
    got = M.SparseInst.inference_batched(_stub(gold), out, inputs, gold.max_shape, gold.image_sizes)
    _compare(got, ref, "image 0 empty:")
    # ... and the other way round: the empty image last
    out["pred_logits"][0], out["pred_logits"][1] = gold.out["pred_logits"][0], -20.0
    got = M.SparseInst.inference_batched(_stub(gold), out, inputs, gold.max_shape, gold.image_sizes)
    _compare(got, M.SparseInst.inference(_stub(gold), out, inputs, gold.max_shape, gold.image_sizes), "image 1 empty:")


def test_mask_threshold_nothing_exceeds(gold):
    """sigmoid < 1: no pixel passes, the rescored scores are 0 / 1e-6 = 0 - no NaN - as in the loop"""
    inputs = [dict(height=h, width=w) for h, w in gold.out_sizes]
    stub = _stub(gold, mask_thr=1.5)
    got = M.SparseInst.inference_batched(stub, gold.out, inputs, gold.max_shape, gold.image_sizes)
    _compare(got, M.SparseInst.inference(stub, gold.out, inputs, gold.max_shape, gold.image_sizes), "threshold 1.5:")
    for r in got:
        assert len(r.scores) > 0 and (r.scores == 0).all() and not r.pred_masks.any()


def test_no_fp32_intermediate_and_one_result_per_image(gold):
    """every query kept, output (200, 250): the call allocates less than ONE fp32 copy of the kept masks at the padded size
    (the loop's first interpolate alone writes that much) - here 80 x 200 x 250 result bytes and a few KB of tables"""
    B, N = gold.out["pred_logits"].shape[:2]
    nhwc, _ = _nhwc_form(gold.out)
    for out in (gold.out, nhwc):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = S.sparseinst_inference_batched(out, gold.image_sizes, [(200, 250)] * B, gold.max_shape, 0.0, gold.mask_thr)
        torch.cuda.synchronize()
        used = torch.cuda.max_memory_allocated() - base
        n = sum(len(r.scores) for r in res)
        print(f"{n} kept: {used} bytes allocated, bound {n * gold.max_shape[0] * gold.max_shape[1] * 4}")
        assert n == B * N and used < n * gold.max_shape[0] * gold.max_shape[1] * 4
        # one flat result: the images' masks are views into the same storage, one after the other
        assert res[0].pred_masks.untyped_storage().data_ptr() == res[1].pred_masks.untyped_storage().data_ptr()
        assert res[1].pred_masks.storage_offset() == res[0].pred_masks.numel()
    out = dict(gold.out, pred_logits=gold.out["pred_logits"].clone())
    out["pred_logits"][1] = -20.0
    res = S.sparseinst_inference_batched(out, gold.image_sizes, gold.out_sizes, gold.max_shape, gold.cls_thr, gold.mask_thr)
    assert len(res) == B and len(res[1].scores) == 0 and len(res[0].scores) == 38


def test_eval_forward_takes_the_batched_path():
    """the model of test_sparseinst_meta_arch_step_and_inference in eval mode: on ONE decoder output the batched method and
    the loop agree, and forward - MI_SPARSEINST_INFER_BATCHED unset - returns what the batched method returns"""
    assert S._INFER_BATCHED == (os.environ.get("MI_SPARSEINST_INFER_BATCHED", "1") != "0")
    torch.manual_seed(0)
    cfg = M.sparse_inst_r50_giam_cfg(device=DEV)
    cfg.MODEL.YOLO.CONF_THRESHOLD = 0.005
    model = M.build_model(cfg).eval()
    _, targets, _ = synth_sparseinst_case(seed=9, H=192, W=224)
    gen = torch.Generator().manual_seed(1)
    inputs = [dict(image=torch.randint(0, 256, (3, t["size"][0], t["size"][1]), generator=gen).float(), height=t["size"][0] + 37,
                   width=t["size"][1] - 11) for t in targets]
    with torch.no_grad():
        images = model.preprocess_inputs(inputs)
        max_shape = images.tensor.shape[2:]
        output = model.decoder(model.encoder(model.backbone(images.tensor)))
        assert output["_masks_nhwc"].dtype == torch.bfloat16
        got = model.inference_batched(output, inputs, max_shape, images.image_sizes)
        ref = model.inference(output, inputs, max_shape, images.image_sizes)
        assert sum(len(r.scores) for r in ref) > 0
        _compare(got, ref, "eval model:")
        called = []
        orig = model.inference_batched
        model.inference_batched = lambda *a, **k: called.append(1) or orig(*a, **k)
        res = model(inputs)
    assert len(res) == 2 and (len(called) == 1) == S._INFER_BATCHED
    for r, t in zip(res, inputs):
        assert r["instances"].image_size == (t["height"], t["width"])
