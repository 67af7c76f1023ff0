"""child process of tests/test_gpu_conv_exact.py::test_tile_kernel_four_wave_forms_in_a_child: MI_CONV_W8 (the largest grid
that takes the 8-wave form of a tile) is read ONCE per process, so it comes from this process's environment.  Runs the rows of
that file's tile matrix whose (pixel tile, cout tile) the 8-wave rule shadows - every k-chunk, taps class and epilogue - with
every result compared bit for bit with the float64 reference, and prints one JSON line.  Exit code 0 = it ran to the end (the
parent judges the line)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_conv_exact as T  # noqa: E402

bad = T.run_tile_matrix([16, 32, 64, 128], only_shadowed=True)
seen = sorted(T.seen_instantiations())
env = {k: os.environ[k] for k in ("MI_CONV_W8", "MI_CONV_W8MASK") if k in os.environ}
print(json.dumps(dict(env=env, seen=[[kc, list(form), tps, epi] for kc, form, tps, epi in seen],
                      launches=sum(v for k, v in T.COUNT.items() if isinstance(k, tuple)),
                      refused=T.REFUSED, bad=[repr(b) for b in bad[:50]])))
