"""ONNX export of YOLOX (export.py:237-303) in an image with neither `onnx` nor `onnxruntime`:

* the test reader / interpreter (tests/onnx_interp.py) is first checked against a file TORCH's own exporter writes for a small
  module with the same operator kinds (Conv, SiLU, MaxPool, nearest Resize, strided Slice, Concat) - that pins the protobuf
  field numbers the exporter uses and the interpreter's operator semantics to torch's;
* then the exported YOLOX-s graph (weights of the reference's golden, 64 x 96) is executed by that interpreter and compared
  with the REFERENCE's own export-mode output (`yolox_s_onnx_layout_64x96.npz`: head.onnx_export = True) in fp32."""
import io
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import onnx_interp as OI  # noqa: E402


class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.c = torch.nn.Conv2d(12, 8, 3, padding=1)
        self.p = torch.nn.MaxPool2d(5, 1, 2)
        self.u = torch.nn.Upsample(scale_factor=2, mode="nearest")

    def forward(self, x):
        x = x.permute(0, 3, 1, 2)
        x = torch.cat((x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]), 1)
        y = torch.nn.functional.silu(self.c(x))
        y = torch.cat([y, self.p(y)], 1)
        return self.u(y)


def _torch_export(m, x, **kw):
    """torch's TorchScript exporter without the `onnx` package: its C++ serialiser writes the ModelProto, only the
    onnxscript-function post-pass imports onnx - skipped (there are no such functions here)"""
    from torch.onnx._internal.torchscript_exporter import onnx_proto_utils
    keep = onnx_proto_utils._add_onnxscript_fn
    onnx_proto_utils._add_onnxscript_fn = lambda model_bytes, custom_opsets: model_bytes
    try:
        f = io.BytesIO()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.onnx.export(m, x, f, opset_version=11, dynamo=False, **kw)
        return f.getvalue()
    finally:
        onnx_proto_utils._add_onnxscript_fn = keep


def test_reader_and_interpreter_against_torchs_own_exporter():
    torch.manual_seed(0)
    m = _Small().eval()
    x = torch.randn(2, 16, 24, 3)
    try:
        data = _torch_export(m, x, input_names=["images"], output_names=["outs"], dynamic_axes={"images": {0: "batch"}})
    except Exception as e:       # noqa: BLE001  (a torch build whose exporter cannot run without onnx: nothing to pin against)
        pytest.skip("torch's exporter is unavailable here: %r" % (e,))
    model = OI.load(data)
    assert model["opset"] == 11 and model["inputs"] == ["images"] and model["outputs"] == ["outs"]
    assert {n[0] for n in model["nodes"]} >= {"Conv", "Sigmoid", "Mul", "MaxPool", "Resize", "Slice", "Concat", "Transpose"}
    x2 = torch.randn(3, 16, 24, 3)
    (got,) = OI.run(model, {"images": x2.numpy()})
    np.testing.assert_allclose(got, m(x2).detach().numpy(), rtol=1e-5, atol=1e-5)


def _model():
    import yolov7_d2_amd as M
    import yolox_oracle as O
    model = M.build_model(M.yolox_s_cfg(device="cpu"))
    model.load_state_dict(O.init_state_dict(0.33, 0.5, 80, seed=0))
    return model.eval(), O


def test_exported_yolox_graph_reproduces_the_references_export_mode_output(golden_dir):
    from yolov7_d2_amd.export_onnx import export_yolox_onnx
    model, O = _model()
    f = io.BytesIO()
    data = export_yolox_onnx(model, f, height=64, width=96)
    assert f.getvalue() == data and len(data) > 30_000_000        # 8.97 M fp32 parameters
    g = OI.load(data)
    assert g["opset"] == 11 and g["ir_version"] == 6 and g["inputs"] == ["images"] and g["outputs"] == ["outs"]
    ops = [n[0] for n in g["nodes"]]
    assert ops.count("Conv") == 83 and "BatchNormalization" not in ops          # 83 convs, every BN folded
    imgs, _ = O.synth_batch(2, 64, 96, seed=11, max_gt=4)
    (out,) = OI.run(g, {"images": imgs.permute(0, 2, 3, 1).contiguous().numpy()})
    ref = np.load(os.path.join(golden_dir, "yolox_s_onnx_layout_64x96.npz"))["out"]
    assert out.shape == ref.shape == (2, 126, 86)
    np.testing.assert_allclose(out[..., :5], ref[..., :5], rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(out[..., 6:], ref[..., 6:], rtol=2e-4, atol=2e-5)
    assert np.array_equal(out[..., 5], out[..., 6:].argmax(-1).astype(np.float32))
    assert (out[..., 5] == ref[..., 5]).mean() > 0.98
    (one,) = OI.run(g, {"images": imgs.permute(0, 2, 3, 1).contiguous().numpy()[:1]})      # the batch axis is dynamic
    keep = [c for c in range(86) if c != 5]                     # (the class-index column flips on the random-init near-ties)
    np.testing.assert_allclose(one[..., keep], out[:1][..., keep], rtol=1e-4, atol=1e-5)
    model.train()
    with pytest.raises(RuntimeError):
        export_yolox_onnx(model, io.BytesIO(), 64, 96)


@pytest.mark.parametrize("depth,width,depthwise,nc", [(0.33, 0.375, False, 80), (0.33, 0.5, True, 20)], ids=["tiny", "depthwise_20cls"])
def test_exported_variants_against_the_reference_run_by_path(depth, width, depthwise, nc, golden_dir):
    """other widths (YOLOX-tiny, BASELINE configs[0]) and MODEL.DARKNET.DEPTH_WISE: the exported graph against the
    reference's own modules (run by path in export mode: export_traces.npz) on seeded weights with BatchNorm running
    statistics that are not the identity"""
    import yolov7_d2_amd as M
    import yolox_oracle as O
    from gen_golden_inputs import perturbed_bn_state_dict
    from yolov7_d2_amd.export_onnx import export_yolox_onnx
    sd, g = perturbed_bn_state_dict(O.init_state_dict(depth, width, nc, seed=3, depthwise=depthwise))
    cfg = M.yolox_s_cfg(device="cpu")
    cfg.MODEL.YOLO.DEPTH_MUL, cfg.MODEL.YOLO.WIDTH_MUL, cfg.MODEL.YOLO.CLASSES = depth, width, nc
    cfg.MODEL.DARKNET.DEPTH_WISE = depthwise
    model = M.build_model(cfg)
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.missing_keys, missing.missing_keys[:5]
    data = export_yolox_onnx(model.eval(), io.BytesIO(), height=96, width=64)
    x = torch.rand(2, 96, 64, 3, generator=g) * 255
    (out,) = OI.run(OI.load(data), {"images": x.numpy()})
    want = np.load(os.path.join(golden_dir, "export_traces.npz"))[f"variant_{width}_{int(depthwise)}_{nc}"]
    assert out.shape == want.shape == (2, 126, 6 + nc)
    keep = [c for c in range(6 + nc) if c != 5]
    np.testing.assert_allclose(out[..., keep], want[..., keep], rtol=5e-4, atol=5e-4)
    assert (out[..., 5] == want[..., 5]).mean() > 0.97


def _traced_census(gold, name):
    """operator census of a graph torch's exporter traced from the reference's modules (export_traces.npz)"""
    import collections
    return collections.Counter(dict(zip([str(k) for k in gold[f"{name}_ops"]], [int(v) for v in gold[f"{name}_counts"]])))


def test_written_graph_equals_the_file_torchs_exporter_traces_from_the_reference(golden_dir):
    """what export.py itself would write: the REFERENCE's modules (by path, head.onnx_export = True) traced by torch's
    TorchScript exporter at opset 11 with constant folding (its operator census and executed output: export_traces.npz,
    oracle/gen_golden.py::gold_export_traces) - against the graph this package writes from its module tree with the same
    weights: the same operator census where it matters (83 Conv, 80 Sigmoid, 76 Mul, 8 Add, 3 MaxPool, 2 Resize, no
    BatchNormalization in either) and the same output when both files are executed"""
    import collections
    import yolox_oracle as O
    from yolov7_d2_amd.export_onnx import export_yolox_onnx
    gold = np.load(os.path.join(golden_dir, "export_traces.npz"))
    imgs, _ = O.synth_batch(2, 64, 96, seed=11, max_gt=4)
    model, _ = _model()
    mine = export_yolox_onnx(model, io.BytesIO(), height=64, width=96)
    gm = OI.load(mine)
    ct, cm = _traced_census(gold, "yolox"), collections.Counter(n[0] for n in gm["nodes"])
    for op in ("Conv", "Sigmoid", "Mul", "Add", "MaxPool", "Resize", "Exp", "ArgMax", "Split", "BatchNormalization"):
        assert ct[op] == cm[op], (op, ct[op], cm[op])
    a = gold["yolox_out"]                                                         # the traced file took NCHW (the meta-arch's
    (b,) = OI.run(gm, {"images": imgs.permute(0, 2, 3, 1).contiguous().numpy()})  # preprocess_input permute sits outside `ref`)
    keep = [c for c in range(86) if c != 5]
    np.testing.assert_allclose(b[..., keep], a[..., keep], rtol=2e-4, atol=2e-4)
    assert (a[..., 5] == b[..., 5]).mean() > 0.98


# ------------------------------------------------------------------------------------------------ SparseInst
class _SmallSI(torch.nn.Module):
    """the operator kinds of the SparseInst export that the YOLOX one does not have, in the forms torch's exporter writes"""

    def __init__(self):
        super().__init__()
        self.c = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.l = torch.nn.Linear(8, 6)

    def forward(self, x):
        x = (x.permute(0, 3, 1, 2) - 0.5) / 2.0
        y = torch.relu(self.c(x))                                                     # [B, 8, 12, 16]
        p = torch.nn.functional.avg_pool2d(y, kernel_size=(4, 6), ceil_mode=False)
        p = torch.nn.functional.interpolate(p, size=(12, 16), mode="bilinear", align_corners=False)
        y = y + p
        prob = y.sigmoid().view(y.shape[0], 8, -1)                                    # [B, 8, P]
        inst = torch.bmm(prob, y.view(y.shape[0], 8, -1).permute(0, 2, 1))           # [B, 8, 8]
        inst = inst / prob.sum(-1).clamp(min=1e-6, max=1e5)[:, :, None]
        z = self.l(inst)                                                              # [B, 8, 6]
        s = torch.sqrt(z.sigmoid() * z.sigmoid() + 1e-3)
        scores, labels = torch.max(s, dim=s.dim() - 1)                                # [B, 8]
        _, keep = torch.topk(scores, k=4)
        flat = scores.view(-1)[keep.view(-1, 4)]
        m = torch.nn.functional.interpolate(y, scale_factor=2.0, mode="bilinear", align_corners=False)
        hard = (m > 0.3).float()
        return flat * ((m * hard).sum([2, 3]) / (hard.sum([2, 3]) + 1e-6))[:, :4], labels.view(-1)[keep.view(-1, 4)], m > 0.3


def test_interpreter_operators_of_the_sparseinst_export_against_torchs_exporter():
    torch.manual_seed(1)
    m = _SmallSI().eval()
    x = torch.rand(1, 12, 16, 3)
    try:
        data = _torch_export(m, x, input_names=["images"], output_names=["a", "b", "c"], do_constant_folding=True)
    except Exception as e:       # noqa: BLE001
        pytest.skip("torch's exporter is unavailable here: %r" % (e,))
    model = OI.load(data)
    ops = {n[0] for n in model["nodes"]}
    assert ops >= {"Relu", "AveragePool", "Resize", "MatMul", "ReduceSum", "Clip", "Div", "Sqrt", "ReduceMax", "ArgMax", "TopK", "Gather",
                   "Greater", "Sub"}, sorted(ops)
    lin = [n for n in model["nodes"] if n[0] == "Resize"]
    assert all(n[3]["mode"] == "linear" and n[3]["coordinate_transformation_mode"] == "half_pixel" for n in lin)     # (what export_onnx writes too)
    a, b, c = OI.run(model, {"images": x.numpy()})
    wa, wb, wc = m(x)
    np.testing.assert_allclose(a, wa.detach().numpy(), rtol=1e-5, atol=1e-6)
    assert np.array_equal(b, wb.numpy()) and np.array_equal(c, wc.numpy())


def _match_rows(scores, labels, masks, ref_scores, ref_labels, ref_masks):
    """rows of one image matched one to one by (label, rescored score, mask): the order INSIDE the top-k may differ where two
    ranking scores are a few fp32 ulps apart; returns the number of unmatched rows and the worst mask disagreement"""
    used, worst = set(), 0.0
    for k in range(len(scores)):
        best = None
        for j in range(len(ref_scores)):
            if j in used or labels[k] != ref_labels[j] or abs(scores[k] - ref_scores[j]) > 2e-4:
                continue
            d = float((masks[k] != ref_masks[j]).mean())
            if best is None or d < best[1]:
                best = (j, d)
        if best is None:
            return len(scores) - len(used), 1.0
        used.add(best[0])
        worst = max(worst, best[1])
    return 0, worst


def _sparseinst_model():
    import yolov7_d2_amd as M
    from gen_golden_inputs import sparseinst_onnx_weights
    model = M.build_model(M.sparse_inst_r50_giam_cfg(device="cpu"))
    sd = sparseinst_onnx_weights({k: v.shape for k, v in model.state_dict().items()})
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.missing_keys and not missing.unexpected_keys, (missing.missing_keys[:4], missing.unexpected_keys[:4])
    return model.eval()


def test_exported_sparseinst_graph_reproduces_the_references_export_mode_outputs(golden_dir):
    """export.py:237-243 for a sparse_inst config (input "images", outputs "masks", "scores", "labels"): the written graph,
    executed, against what the REFERENCE's own encoder / decoder / inference_onnx produced by path on the same weights and
    images (sparseinst_onnx.npz; backbone = the ResNet restatement) - for the batch of 1 the reference exports with and
    for a batch of 2, where inference_onnx's flattened top-k indexing reads the first image only (reproduced, not fixed)"""
    from gen_golden_inputs import synth_sparseinst_images
    from yolov7_d2_amd.export_onnx import export_sparseinst_onnx
    gold = np.load(os.path.join(golden_dir, "sparseinst_onnx.npz"))
    model = _sparseinst_model()
    H, W = [int(v) for v in gold["hw"]]
    data = export_sparseinst_onnx(model, io.BytesIO(), height=H, width=W)
    g = OI.load(data)
    assert g["opset"] == 11 and g["inputs"] == ["images"] and g["outputs"] == ["masks", "scores", "labels"]
    ops = [n[0] for n in g["nodes"]]
    assert ops.count("Conv") == 53 + 12 + 10 and "BatchNormalization" not in ops      # ResNet-50, encoder, decoder; FrozenBN folded
    for B in (1, 2):
        img = synth_sparseinst_images(B, H, W, int(gold[f"seed{B}"]))
        masks, scores, labels = OI.run(g, {"images": img.numpy()})
        shape = tuple(int(v) for v in gold[f"mask_shape{B}"])
        ref_masks = np.unpackbits(gold[f"masks{B}"], axis=-1)[..., : shape[-1]].astype(bool)
        assert masks.shape == shape and masks.dtype == np.bool_ and scores.shape == (B, 50) and labels.dtype == np.int64
        for b in range(B):
            miss, worst = _match_rows(scores[b], labels[b], masks[b], gold[f"scores{B}"][b], gold[f"labels{B}"][b], ref_masks[b])
            assert miss == 0 and worst < 2e-3, (B, b, miss, worst)
        if B == 2:      # the quirk: both rows index the flattened tensors without a batch offset -> image 0's predictions
            assert len(set(labels[1].tolist()) - set(labels[0].tolist()) - set(gold["labels2"][0].tolist())) == 0
    model.train()
    with pytest.raises(RuntimeError):
        export_sparseinst_onnx(model, io.BytesIO(), H, W)


def test_written_sparseinst_graph_equals_the_trace_of_the_references_modules(golden_dir):
    """what export.py itself would write for the part of the model the reference tree contains: its InstanceContextEncoder
    + GroupIAMDecoder + inference_onnx (loaded by path), traced by torch's exporter under is_in_onnx_export() at opset 11
    (census and executed outputs: export_traces.npz, oracle/gen_golden.py::gold_export_traces), against the graph this
    package writes - same operator census where it matters, same outputs when both are executed (the traced module took
    the ResNet restatement as its backbone)"""
    import collections
    from gen_golden_inputs import synth_sparseinst_images
    from yolov7_d2_amd.export_onnx import export_sparseinst_onnx
    gold = np.load(os.path.join(golden_dir, "export_traces.npz"))
    H, W = 64, 96
    img = synth_sparseinst_images(1, H, W, 600)
    mine = export_sparseinst_onnx(_sparseinst_model(), io.BytesIO(), height=H, width=W)
    gm = OI.load(mine)
    ct, cm = _traced_census(gold, "sparseinst"), collections.Counter(n[0] for n in gm["nodes"])
    for op in ("Conv", "Relu", "MaxPool", "MatMul", "TopK", "ArgMax", "ReduceMax", "Greater", "Sqrt", "Resize", "BatchNormalization"):
        assert ct[op] == cm[op], (op, ct[op], cm[op])
    assert ct["AveragePool"] == 3 and cm["AveragePool"] == 4      # (the 1 x 1 window of the 6-bin stage on a 2 x 3 map: the tracer drops the identity)
    shape = tuple(int(v) for v in gold["sparseinst_mask_shape"])
    ta = np.unpackbits(gold["sparseinst_masks"], axis=-1)[..., : shape[-1]].astype(bool)
    tb, tc = gold["sparseinst_scores"], gold["sparseinst_labels"]
    ma, mb, mc = OI.run(gm, {"images": img.numpy()})
    assert ta.shape == ma.shape and tb.shape == mb.shape and tc.shape == mc.shape
    miss, worst = _match_rows(mb[0], mc[0], ma[0], tb[0], tc[0], ta[0])
    assert miss == 0 and worst < 2e-3, (miss, worst)


# ------------------------------------------------------------------------------------------------ DETR
def _detr_model():
    import yolov7_d2_amd as M
    from gen_golden_inputs import detr_onnx_weights
    model = M.build_model(M.detr_r50_cfg(device="cpu"))
    sd = detr_onnx_weights({k: v.shape for k, v in model.state_dict().items()})
    missing = model.load_state_dict(sd, strict=False)
    assert not [k for k in missing.missing_keys if "empty_weight" not in k] and not missing.unexpected_keys, missing
    return model.eval()


def test_exported_detr_graph_reproduces_the_references_export_mode_output(golden_dir):
    """export.py for a detr config: the written graph, executed, against the REFERENCE's own Detr run by path with
    onnx_export = True on the same weights and images (detr_onnx.npz): [x0, y0, x1, y1, score, label] per query"""
    from gen_golden_inputs import synth_sparseinst_images
    from yolov7_d2_amd.export_onnx import export_detr_onnx, export_onnx
    gold = np.load(os.path.join(golden_dir, "detr_onnx.npz"))
    model = _detr_model()
    H, W = [int(v) for v in gold["hw"]]
    data = export_detr_onnx(model, io.BytesIO(), height=H, width=W)
    assert export_onnx(model, io.BytesIO(), H, W) == data
    g = OI.load(data)
    assert g["opset"] == 11 and g["inputs"] == ["images"] and g["outputs"] == ["outs"]
    ops = [n[0] for n in g["nodes"]]
    assert ops.count("Conv") == 53 + 1 and ops.count("Softmax") == 6 + 12 + 1 and "BatchNormalization" not in ops
    for B in (1, 2):
        x = synth_sparseinst_images(B, H, W, int(gold[f"seed{B}"])).permute(0, 3, 1, 2).contiguous()
        (out,) = OI.run(g, {"images": x.numpy()})
        ref = gold[f"outs{B}"]
        assert out.shape == ref.shape == (B, 100, 6)
        np.testing.assert_allclose(out[..., :5], ref[..., :5], rtol=1e-4, atol=2e-5)
        assert np.array_equal(out[..., 5], ref[..., 5])
    model.train()
    with pytest.raises(RuntimeError):
        export_detr_onnx(model, io.BytesIO(), H, W)


def test_sine_position_embedding_constant_equals_the_oracle():
    """the constant the DETR export bakes in for an all-valid mask == the position-embedding oracle (pinned to the reference's
    PositionEmbeddingSine by pos_embed.npz), normalised and raw"""
    import types
    import detr_net_oracle as DN
    from yolov7_d2_amd.export_onnx import _sine_position_embedding
    for normalize in (True, False):
        pe = types.SimpleNamespace(num_pos_feats=64, temperature=10000, normalize=normalize, scale=2 * np.pi, centered=False)
        got = _sine_position_embedding(pe, 5, 7)
        want = DN.position_embedding_sine(torch.zeros(1, 5, 7, dtype=torch.bool), 64, 10000, normalize, 2 * np.pi).numpy()
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)


def test_written_detr_graph_equals_the_trace_of_the_references_detr(golden_dir):
    """what export.py would write if its detr branch ran: the REFERENCE's Detr (by path, onnx_export = True; its own
    MaskedBackboneTraceFriendly mask resize, PositionEmbeddingSine cumsums, nn.MultiheadAttention, heads and export rows)
    traced by torch's exporter at opset 11 (census and executed output: export_traces.npz,
    oracle/gen_golden.py::gold_export_traces) - against the graph this package writes from its module tree: the same
    census of the operators that carry the model and, executed, the same output"""
    import collections
    from gen_golden_inputs import synth_sparseinst_images
    from yolov7_d2_amd.export_onnx import export_detr_onnx
    gold = np.load(os.path.join(golden_dir, "export_traces.npz"))
    H, W = 64, 96
    x = synth_sparseinst_images(2, H, W, 905).permute(0, 3, 1, 2).contiguous()
    mine = export_detr_onnx(_detr_model(), io.BytesIO(), height=H, width=W)
    gm = OI.load(mine)
    ct, cm = _traced_census(gold, "detr"), collections.Counter(n[0] for n in gm["nodes"])
    for op in ("Conv", "Relu", "MaxPool", "Softmax", "Sigmoid", "ArgMax", "ReduceMax", "BatchNormalization"):
        assert ct[op] == cm[op], (op, ct[op], cm[op])
    # LayerNorms (2 ReduceMean each): 2 per encoder layer, 3 per decoder layer, decoder.norm - which the trace keeps for all six
    # intermediate levels although only hs[-1] reaches the output (dead nodes); the written graph has the live one
    assert ct["ReduceMean"] == 2 * (12 + 18 + 6) and cm["ReduceMean"] == 2 * (12 + 18 + 1)
    a = gold["detr_out"]
    (b,) = OI.run(gm, {"images": x.numpy()})
    assert a.shape == b.shape == (2, 100, 6) and not np.isnan(a).any()
    np.testing.assert_allclose(b[..., :5], a[..., :5], rtol=1e-4, atol=2e-5)
    assert np.array_equal(a[..., 5], b[..., 5])
