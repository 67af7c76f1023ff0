"""GPU (-m gpu): the d2 and the vd bottleneck block through their shared autograd node (modeling/resnet.py _BottleneckFn)
against what the commit before the merge computed with its two separate nodes - tests/golden/bottleneck_parent_record.npz,
written there by tools/record_bottleneck_outputs.py from the cases of tests/bottleneck_cases.py.  The merge moved no launch
and no argument, so every tensor - output, input gradient, each weight gradient, with the weight gradients grouped into one
launch and as single launches - has the recorded BITS; nothing here is a tolerance."""
import os

import numpy as np
import pytest

import bottleneck_cases as B
from yolov7_d2_amd.modeling import resnet as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", B.RECORD)) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("grouped", B.GROUPED, ids=["wgrad_grouped", "wgrad_single"])
@pytest.mark.parametrize("name", list(B.CASES))
def test_bottleneck_outputs_equal_the_parent_record(name, grouped, record, monkeypatch):
    """every recorded tensor bit for bit (SHA-256 of all of them; under the default, grouped setting also the tensors
    themselves, so that a difference is located).  Each block's backward asks _premask_take once: in the stacks the first
    answer (the identity block, handed the test's own output gradient) is no, the second - the projection block BEFORE it,
    handed the input gradient the identity block masked in its last epilogue and noted - is yes."""
    takes = []
    take = R._premask_take
    monkeypatch.setattr(R, "_premask_take", lambda t: takes.append(take(t)) or takes[-1])
    res = B.run(name, grouped)
    prefix = f"{name}/g{grouped}/sha256/"
    assert {prefix + k for k in res} == {k for k in record if k.startswith(prefix)}
    for k, v in res.items():
        full = record.get(f"{name}/g{grouped}/bits/{k}")
        if full is not None:
            assert v.shape == full.shape and v.dtype == full.dtype, (k, v.shape, full.shape)
            assert np.array_equal(v, full), (k, f"{int((v != full).sum())} of {v.size} words differ")
        assert np.array_equal(B.digest(v), record[prefix + k]), k
    assert takes == [False] + [True] * (len(B.CASES[name][1]) - 1), takes
