"""CPU: the numpy restatement of the batched SparseInst postprocess (tests/sparseinst_infer_ref.py) against the REFERENCE'S
own `inference` outputs (golden sparseinst_inference.npz), with the tolerances of
test_gpu_sparseinst.py::test_sparseinst_inference_against_reference_golden, and against torch's F.interpolate on the CPU at
output sizes the golden lacks."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import sparseinst_infer_ref as R


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sparseinst_inference.npz"))


def test_restatement_against_reference_golden(golden_dir):
    g = _golden(golden_dir)
    res = R.inference(g["pred_logits"], g["pred_scores"], g["pred_masks"], g["image_sizes"].tolist(), g["out_sizes"].tolist(),
                      g["max_shape"].tolist(), float(g["cls_threshold"]), float(g["mask_threshold"]))
    assert len(res) == 2
    for b, (scores, labels, masks) in enumerate(res):
        assert np.array_equal(labels, g[f"classes{b}"])                       # kept set (count, order) and classes
        np.testing.assert_allclose(scores, g[f"scores{b}"], rtol=2e-5, atol=1e-7)
        ref = np.unpackbits(g[f"masks{b}"], axis=-1)[..., : masks.shape[-1]].astype(bool)
        assert masks.shape == ref.shape and masks.dtype == np.bool_
        mism = float((masks != ref).mean())
        darea = int(np.abs(masks.reshape(len(masks), -1).sum(1) - g[f"mask_area{b}"]).max())
        print(f"image {b}: {len(labels)} kept, mask mismatch share {mism:.2e}, area difference {darea}")
        assert mism < 1e-4 and darea <= 3


def test_composed_resize_against_torch_cpu(golden_dir):
    g = _golden(golden_dir)
    thr = float(g["mask_threshold"])
    pad = tuple(g["max_shape"].tolist())
    for b, img in enumerate(g["image_sizes"].tolist()):
        m = R.sigmoid(g["pred_masks"][b])
        for out in ((8, 10), (13, 7), (400, 333), (201, 251), tuple(img)):
            t = F.interpolate(torch.from_numpy(m)[:, None], size=pad, mode="bilinear", align_corners=False)[:, :, : img[0], : img[1]]
            ref = (F.interpolate(t, size=out, mode="bilinear", align_corners=False)[:, 0] > thr).numpy()
            got = R.compose_masks(m, pad, tuple(img), out, thr)
            mism = float((got != ref).mean())
            print(f"image {b} -> {out}: mismatch share {mism:.2e}")
            assert got.shape == ref.shape and mism < 1e-4


def test_select_keeps_ascending_and_handles_empty_denominator():
    rng = np.random.default_rng(0)
    logits = rng.normal(size=(2, 7, 5)).astype(np.float32)
    logits[0] = -20.0                                                          # image 0 keeps nothing
    logits[1, 3, 2] = logits[1, 3, 4] = 9.0                                    # a tie: the first maximum wins
    obj = np.full((2, 7, 1), 3.0, np.float32)
    masks = rng.normal(size=(2, 7, 4, 6)).astype(np.float32)
    (k0, s0, l0), (k1, s1, l1) = R.select_rescore(logits, obj, masks, 0.2, 0.999999)
    assert len(k0) == len(s0) == len(l0) == 0
    assert np.array_equal(k1, np.sort(k1)) and 3 in k1 and l1[list(k1).index(3)] == 2
    assert np.array_equal(s1, np.zeros_like(s1))                               # 0 / 1e-6: zero, not NaN
