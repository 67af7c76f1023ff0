"""Writes tests/golden/rcda.npz from the reference's OWN MultiheadRCDA
(yolov7/modeling/backbone/layers/row_column_decoupled_attention.py, loaded by path; needs the reference tree), in float64 on
the CPU: one small case - B 2, L 70, H 5, W 7, E 64, 2 heads, image 1 with columns 5.. and rows 4.. padded - with the
module's parameters, the inputs (bf16-representable numbers, so that a device test feeds exactly these), the mask, a random
cotangent, the output and the gradient of every input and parameter.  Data only; the tests never read the reference.

    python tools/gen_rcda_golden.py [path of the reference tree]
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = os.path.join("yolov7", "modeling", "backbone", "layers", "row_column_decoupled_attention.py")
B, LQ, H, W, E, HEADS = 2, 70, 5, 7, 64, 2
INPUTS = ("query_row", "query_col", "key_row", "key_col", "value")


def load_reference(tree):
    spec = importlib.util.spec_from_file_location("reference_rcda", os.path.join(tree, REL))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MultiheadRCDA


def main():
    tree = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT")
    if not tree or not os.path.exists(os.path.join(tree, REL)):
        sys.exit("usage: gen_rcda_golden.py <reference tree>  (or REFERENCE_ROOT): " + REL + " not found")
    torch.manual_seed(20)
    net = load_reference(tree)(E, HEADS, dropout=0.0).double()
    with torch.no_grad():       # the biases are 0 after the reference's initialisation: make them count
        net.in_proj_bias.normal_(0, 0.1)
        net.out_proj.bias.normal_(0, 0.1)
    bf = lambda x: x.to(torch.bfloat16).double()
    shapes = dict(query_row=(B, LQ, E), query_col=(B, LQ, E), key_row=(B, H, W, E), key_col=(B, H, W, E), value=(B, H, W, E))
    xs = {k: bf(torch.randn(*s, dtype=torch.float64)).requires_grad_(True) for k, s in shapes.items()}
    mask = torch.zeros(B, H, W, dtype=torch.bool)
    mask[1, :, 5:] = True
    mask[1, 4:, :] = True
    dout = bf(torch.randn(LQ, B, E, dtype=torch.float64))
    out, weights = net(*[xs[k] for k in INPUTS], key_padding_mask=mask)
    assert weights is None and out.shape == (LQ, B, E)
    out.backward(dout)
    data = {"mask": mask.numpy(), "dout": dout.numpy(), "out": out.detach().numpy(), "heads": np.int64(HEADS)}
    for k, x in xs.items():
        data["in/" + k] = x.detach().numpy()
        data["grad_in/" + k] = x.grad.numpy()
    for k, p in net.named_parameters():
        data["param/" + k] = p.detach().numpy()
        data["grad_param/" + k] = p.grad.numpy()
    path = os.path.join(ROOT, "tests", "golden", "rcda.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in data.items()})
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
