#!/usr/bin/env python
"""GPU box: run mi_yolox_loss_fwd / bwd of the loaded library on the three inputs of tests/simota_cases.py and write what
tests/test_gpu_step.py::test_simota_outputs_equal_the_round5_record compares against:
    tools/record_simota_outputs.py [out.npz]        (default tests/golden/simota_round5_record.npz)
Per case: ngt, fg (bit-packed), matched_gt, matched_iou and out in full, SHA-256 of the bytes of cost, iou and dpreds."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np

import simota_cases as S

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", S.RECORD)
rec = {}
for name, raw, labels, anchors, kw in S.record_cases():
    ws = S.loss_call(raw, labels, anchors, **kw)
    for k, v in S.record_of(ws).items():
        rec[f"{name}_{k}"] = v
    print(f"{name}: num_fg {float(ws['out'][6]):.0f}, ngt {int(ws['ngt'].sum())}", flush=True)
np.savez_compressed(out, **rec)
print(f"{out}: {os.path.getsize(out)} bytes")
