"""child process of tests/test_gpu_mha_exact.py::test_version1_kernels_in_a_child: MI_MHA_V2 (0 = the version-1 attention
kernels) is a function-local static of csrc/mha.hip, read ONCE per process, so it comes from this process's environment.
Runs the exact families of tests/mha_ref.py (v1_cases) and the mutants (the v1- cases of mutation_cases) on those kernels,
every result compared bit for bit with the float64 reference, and prints one JSON line.  Exit code 0 = it ran to the end (the
parent judges the line)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import mha_ref as R  # noqa: E402
import test_gpu_mha_exact as T  # noqa: E402

assert os.environ.get("MI_MHA_V2") == "0"
bad = T.run_version1()
cases = R.v1_cases() + [c for c in R.mutation_cases() if c.name.startswith("v1-")]
print(json.dumps(dict(env={k: os.environ[k] for k in ("MI_MHA_V2",) if k in os.environ},
                      kernels=["mha_fwd_kernel", "mha_delta_kernel", "mha_bwd_dq_kernel", "mha_bwd_dkv_kernel"],
                      cases=[c.name for c in cases], families=[[c.family, c.name] for c in cases], bad=bad[:50])))
