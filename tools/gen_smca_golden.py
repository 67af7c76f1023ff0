"""Writes tests/golden/smca.npz from the reference's OWN SMCA transformer (yolov7/modeling/backbone/smcadetr_backbone.py and
layers/smca_attention.py, loaded by path through oracle/ref_loader.py's stubs; needs the reference tree), in float64 on the CPU.

One fixed case for each of the four dynamic_scale types (tests/smca_ref.py GOLD_CASE): d_model 256 / 8 heads (the reference
hard-codes them), no encoder layer (memory = src), two decoder layers, dim_feedforward 32, dropout 0, B 2, 9 queries, a 5 x 7
map, image 1 with columns 5.. padded, h_w not square.  The parameters and inputs are NOT stored: they are the integer recipe of
tests/smca_ref.py, loaded into the reference here and into this project's modules by the tests.  Stored per type: hs, points, the
dense `gaussian` of layer 0 (captured at the attention call), the gradients of src (= memory), query_embed and pos_embed under
the recipe's cotangent, the state_dict names / shapes and the parameter gradients smca_ref.holds_param_grad names (every parameter
for type3 and type4, the point2 / point3 heads for type1 and type2: 1 MiB does not hold all four), all as smca_ref.reduce_grad
keeps them.
Data only; the tests never read the reference.

    python tools/gen_smca_golden.py
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_loader  # noqa: E402
import smca_ref as R  # noqa: E402


def load_reference():
    ref_loader.load()
    return importlib.import_module("yolov7.modeling.backbone.smcadetr_backbone")


def main():
    if not ref_loader.available():
        sys.exit("gen_smca_golden.py: the reference tree is not there")
    ref = load_reference()
    c = R.GOLD_CASE
    data = {}
    for kind in R.TYPES:
        net = ref.Transformer(d_model=c["d_model"], nhead=c["nhead"], num_encoder_layers=0, num_decoder_layers=c["layers"],
                              dim_feedforward=c["dim_feedforward"], dropout=0.0, return_intermediate_dec=True, smooth=c["smooth"],
                              dynamic_scale=kind).double()
        R.fill(net)
        src, mask, qe, pos, h_w, dhs = R.gold_inputs()
        src, qe, pos = (t.clone().requires_grad_(True) for t in (src, qe, pos))
        seen = []
        attn = net.decoder.layers[0].multihead_attn
        hook = attn.register_forward_pre_hook(lambda m, a, kw: seen.append(kw["gaussian"][0].detach().clone()), with_kwargs=True)
        hs, points = net(src, mask, qe, pos, h_w)
        hook.remove()
        assert hs.shape == (c["layers"], c["B"], c["Q"], c["d_model"]) and points.shape == (c["B"], c["Q"], 2) and len(seen) == 1
        hs.backward(dhs)
        p = kind + "/"
        data[p + "hs"], data[p + "points"], data[p + "gaussian"] = hs.detach().numpy(), points.detach().numpy(), seen[0].numpy()
        data[p + "grad_in/query_embed"] = qe.grad.numpy()
        for n, t in (("src", src), ("pos_embed", pos)):
            for k, v in R.reduce_grad(t.grad.numpy()).items():
                data[f"{p}grad_in/{n}/{k}"] = v
        names = []
        for n, prm in net.named_parameters():
            names.append(f"{n} {' '.join(str(s) for s in prm.shape)}")
            assert prm.grad is not None, n
            if R.holds_param_grad(kind, n):
                for k, v in R.reduce_grad(prm.grad.numpy()).items():
                    data[f"{p}grad_param/{n}/{k}"] = v
        data[p + "names"] = np.array("\n".join(names))
    path = os.path.join(ROOT, "tests", "golden", "smca.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes;", len(data), "arrays")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
