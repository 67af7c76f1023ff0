"""Writes tests/golden/resnetvd.npz from the reference's OWN ResNet-vd (yolov7/modeling/backbone/resnetvd.py, loaded by
path as tests/test_resnetvd_ref.py does; needs the reference tree): depth 50, fp32, on the CPU.

Stored: the image [2, 3, 64, 96], the three outputs, and the gradients, for the loss sum(out * fixed random cotangent), of
the weights named in resnetvd_ref.GOLDEN_GRADS - the three large ones as every STEP-th element of the flattened tensor, so
that the file stays well under the size limit for a committed file.  Weights and norm buffers are NOT stored: the tests
regenerate them with resnetvd_ref.random_state(shapes, GOLDEN_SEED), the cotangents with resnetvd_ref.golden_cotangents.

    python tools/gen_resnetvd_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import resnetvd_ref as V  # noqa: E402


def main():
    net = V.build_reference(V.GOLDEN_LAYERS)
    net.load_state_dict(V.random_state({k: tuple(v.shape) for k, v in net.state_dict().items()}, V.GOLDEN_SEED))
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.standard_normal((2, 3, 64, 96)).astype(np.float32))
    out = net(x)
    cot = V.golden_cotangents({k: tuple(v.shape) for k, v in out.items()})
    sum((out[k] * cot[k]).sum() for k in out).backward()
    params = dict(net.named_parameters())
    data = {"image": x.numpy()}
    for k in out:
        data["out/" + k] = out[k].detach().numpy()
    for k, step in V.GOLDEN_GRADS.items():
        data["grad/" + k] = params[k].grad.flatten()[::step].contiguous().numpy()
    path = os.path.join(ROOT, "tests", "golden", "resnetvd.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in data.items()})
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
