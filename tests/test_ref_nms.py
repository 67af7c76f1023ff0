"""The reference's own native greedy NMS (deploy/trt_cc/demo_yolox.cc:53-135, compiled by oracle/Makefile into
oracle/_ref/libref_nms.so) pins the NMS restatement of the oracle (CPU) and the HIP kernel (GPU) on tie-free inputs:
torchvision - whose batched_nms the eval path calls (utils/boxes.py:199) - is neither vendored nor installed, this loop
is the only statement of the suppression rule the reference tree holds (descending score, suppress iff IoU > thr).
Its kept indices on every case below are stored in tests/golden/nms_native.npz (oracle/gen_golden.py::gold_nms_native)."""
import os

import numpy as np
import pytest
import torch

import yolox_oracle as O
from gen_golden_inputs import (NATIVE_BATCHED_CPU_CASES, NATIVE_BATCHED_GPU_CASES, NATIVE_NMS_CASES,
                               synth_tie_free_nms_case as _tie_free)


@pytest.fixture(scope="module")
def native(golden_dir):
    return np.load(os.path.join(golden_dir, "nms_native.npz"))


@pytest.mark.parametrize("n,thr", NATIVE_NMS_CASES)
def test_oracle_nms_against_reference_native(n, thr, native):
    boxes, scores, _ = _tie_free(n, 1, thr, seed=n)
    ref = native[f"nms_{n}_{thr}"]
    got = O.nms(torch.from_numpy(boxes), torch.from_numpy(scores), thr).numpy()
    assert len(ref) >= 1 and np.array_equal(got, ref)


@pytest.mark.parametrize("n,ncls", NATIVE_BATCHED_CPU_CASES)   # 900 x 4 <= 4000 elements: the coordinate trick; 1200: per class
def test_oracle_batched_nms_against_reference_native(n, ncls, native):
    boxes, scores, idxs = _tie_free(n, ncls, 0.65, seed=7 * n)
    ref = native[f"batched_{n}_{ncls}_0.65"]
    got = O.batched_nms(torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(idxs).float(), 0.65).numpy()
    assert np.array_equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n,ncls,thr", NATIVE_BATCHED_GPU_CASES)
def test_hip_batched_nms_against_reference_native(n, ncls, thr, native):
    from yolov7_d2_amd.modeling.postprocess import batched_nms
    boxes, scores, idxs = _tie_free(n, ncls, thr, seed=3 * n + ncls)
    ref = native[f"batched_{n}_{ncls}_{thr}"]
    got = batched_nms(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(idxs).float().cuda(), thr)
    assert torch.equal(got.cpu(), torch.from_numpy(ref))
