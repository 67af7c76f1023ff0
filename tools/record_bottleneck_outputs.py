#!/usr/bin/env python
"""GPU box: run the bottleneck blocks of tests/bottleneck_cases.py (forward + one backward, MI_WGRAD_LAYER_GROUP on and off)
on the checked-out code and write what tests/test_gpu_bottleneck_record.py compares against:
    tools/record_bottleneck_outputs.py [out.npz]        (default tests/golden/bottleneck_parent_record.npz)
Run on the commit BEFORE a change to the blocks' Python layer.  Every case runs twice; nothing is written unless the two
runs agree bit for bit, and unless the output and the input gradient are the same under both settings of the switch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np

import bottleneck_cases as B

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", B.RECORD)
rec = {}
for name in B.CASES:
    runs = {}
    for grouped in B.GROUPED:
        a, b = B.run(name, grouped), B.run(name, grouped)
        diff = [k for k in a if a.keys() != b.keys() or not np.array_equal(a[k], b[k])]
        if diff:
            sys.exit(f"{name} (MI_WGRAD_LAYER_GROUP={grouped}): two runs differ in {diff} - nothing written")
        runs[grouped] = a
        rec.update(B.record_of(name, grouped, a))
    for k in ("out", "dx"):
        if not np.array_equal(runs["1"][k], runs["0"][k]):
            sys.exit(f"{name}: {k} depends on MI_WGRAD_LAYER_GROUP - nothing written")
    print(f"{name}: {len(runs['1'])} tensors, out {runs['1']['out'].shape}, "
          f"{float((runs['1']['dx'] == 0).mean()):.2f} of dx zero", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
np.savez_compressed(out, **rec)
print(f"{out}: {os.path.getsize(out)} bytes")
