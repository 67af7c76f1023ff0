"""child process of tests/test_gpu_bn_exact.py::test_switches_in_a_child: MI_BN_FUSED_MODE (0 = da and y stay in registers as
loaded), MI_BN_BWD_LAST (0 = the legacy phase 2: every block reads every accumulator slot), MI_BN_EW_ITEMS (items per block of
the streaming kernels) and MI_BN_FUSED_ITEMS (items per thread of the one-launch backward) are function-local statics of
csrc/bn_act.hip, read ONCE per process, so they come from this process's environment.  Runs the exact families of
tests/bn_ref.py on the entry points the switch reaches and the mutants, every result compared bit for bit with the float64
reference, and prints one JSON line.  Exit code 0 = it ran to the end (the parent judges the line)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_bn_exact as T  # noqa: E402

env = {k: os.environ[k] for k in T.ENV_KEYS if os.environ.get(k)}
assert len(env) == 1, env
bad = T.run_exact_sweep()
print(json.dumps(dict(env=env, seen=dict(T.SEEN), bad=bad[:50])))
