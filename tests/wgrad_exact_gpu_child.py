"""child process of tests/test_gpu_wgrad_exact.py::test_switches_read_once_per_process: the weight-gradient switches that
the library reads ONCE per process (MI_WG_V3, MI_WG_RED9, MI_WG_REDSL) come from this process's environment.  Runs matrix (b)
of that file - every tile configuration at both pixel-tile sizes - as single launches and as one grouped launch (reduce grid, then fix-up), and that file's
run_child_extras (geometry and epilogues), every
result compared bit for bit with the float64 reference, and prints one JSON line.  Exit code 0 = it ran to the end (the
parent judges the line)."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ["MI_WG_MULTI"] = "0"      # one grid per tile configuration: the group's meta then names every instantiation
os.environ["MI_WG_FIXUP"] = "0"

import test_gpu_wgrad_exact as T  # noqa: E402

bad = T.run_matrix_b_single()
jobs, labels = T.matrix_b_jobs()
gbad, meta = T.run_group(jobs, labels, runs=2)
bad += gbad
os.environ["MI_WG_FIXUP"] = "1"      # (read per plan) the same table with the split-K sum inside the grids
jobs, labels = T.matrix_b_jobs()
gbad, meta1 = T.run_group(jobs, [(lab, "fixup") for lab in labels], runs=2)
bad += gbad
os.environ["MI_WG_FIXUP"] = "0"
bad += T.run_child_extras()
env = {k: os.environ[k] for k in ("MI_WG_V3", "MI_WG_RED9", "MI_WG_REDSL") if k in os.environ}
print(json.dumps(dict(env=env, single=T.COUNT["single"], group_jobs=T.COUNT["group jobs"],
                      cfgs=sorted(list(c) for c in T.group_cfgs(meta)), red_blocks=int(meta.red_blocks),
                      red9_blocks=int(meta.red9_blocks), fixup_groups=sum(meta1.g[i].fixup for i in range(meta1.ngroups)),
                      bad=[repr(b) for b in bad])))
