"""CPU, no device: the C ABI of row-column decoupled attention (csrc/rcda.hip: mi_rcda_desc_size / _key_mean / _fwd /
_bwd_ws_bytes / _bwd) is exported, declared and bound, the descriptor's size agrees with the binding, every argument error
returns -1 without launching and names the quantity, the workspace size is what the header says; and the MultiheadRCDA
module on the host: the reference's state_dict keys and shapes (those of tests/golden/rcda.npz), its initialisation, and every
constructor / forward refusal by name."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from yolov7_d2_amd import _lib as L
from yolov7_d2_amd.modeling import MultiheadRCDA, rcda_core

FAKE = 4096     # non-null, aligned dummy pointer: an argument error must return before anything touches memory
NAMES = ["mi_rcda_desc_size", "mi_rcda_key_mean", "mi_rcda_fwd", "mi_rcda_bwd_ws_bytes", "mi_rcda_bwd"]
PTRS = ("q_row", "q_col", "k_row", "k_col", "v", "o", "lse_row", "lse_col", "dout", "dq_row", "dq_col", "dk_row", "dk_col", "dv", "ws")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rcda.npz")


def _desc(**kw):
    d = L.mi_rcda_desc()
    vals = dict({p: FAKE for p in PTRS}, mask_row=None, mask_col=None, ws_bytes=1 << 40, B=2, heads=2, L=70, H=5, W=7, E=64,
                ldq=64, ldk=64, ldv=64, ldo=64, scale=32 ** -0.5)
    vals.update(kw)
    for k, v in vals.items():
        setattr(d, k, v)
    return d


def _entries():
    lib = L.lib()
    return [("fwd", lambda d: lib.mi_rcda_fwd(C.byref(d), None)), ("bwd", lambda d: lib.mi_rcda_bwd(C.byref(d), None))]


def test_symbols_are_exported_declared_and_bound():
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "..", "include", "mi355_det.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.EXPORTS, n
        assert re.search(r"\b(int|int64_t) %s\(" % n, header), n
    assert "typedef struct mi_rcda_desc" in header


def test_descriptor_size_selfcheck():
    assert L.lib().mi_rcda_desc_size() == C.sizeof(L.mi_rcda_desc) == 17 * 8 + 8 + 10 * 4 + 8


GEOMETRY = [(dict(E=48), b"heads *"), (dict(E=128), b"heads *"), (dict(heads=3), b"heads *"), (dict(B=0), b"positive"),
            (dict(heads=0, E=0), b"positive"), (dict(L=0), b"positive"), (dict(L=-4), b"positive"), (dict(H=0), b"positive"),
            (dict(W=-1), b"positive"), (dict(H=97), b"served size"), (dict(W=128), b"served size"), (dict(H=200, W=200), b"served size")]


def test_unserved_geometry_returns_the_error_status_without_launch():
    lib = L.lib()
    for name, fn in _entries():
        for kw, word in GEOMETRY:
            assert fn(_desc(**kw)) == -1, (name, kw)
            assert word in lib.mi_last_error(), (name, kw, lib.mi_last_error())
            # the geometry is refused before any pointer is looked at
            assert fn(_desc(**dict({p: None for p in PTRS}, **kw))) == -1 and word in lib.mi_last_error(), (name, kw)
    for kw, word in GEOMETRY:
        assert lib.mi_rcda_bwd_ws_bytes(C.byref(_desc(**kw))) == -1 and word in lib.mi_last_error(), kw


def test_pointer_stride_and_workspace_errors_without_launch():
    lib = L.lib()
    fwd, bwd = (fn for _, fn in _entries())
    for fn in (fwd, bwd):
        for p in ("q_row", "q_col", "k_row", "k_col", "v", "lse_row", "lse_col"):
            assert fn(_desc(**{p: None})) == -1 and b"null" in lib.mi_last_error(), p
        for p in ("q_row", "q_col", "k_row", "k_col", "v"):
            assert fn(_desc(**{p: FAKE + 8})) == -1 and b"aligned" in lib.mi_last_error(), p
        assert fn(_desc(lse_row=FAKE + 2)) == -1 and b"aligned" in lib.mi_last_error()
        for s in ("ldq", "ldk", "ldv", "ldo"):
            assert fn(_desc(**{s: 32})) == -1 and s.encode() in lib.mi_last_error(), s
            assert fn(_desc(**{s: 68})) == -1 and b"multiples of 8" in lib.mi_last_error(), s
    assert fwd(_desc(o=None)) == -1 and b"null" in lib.mi_last_error()
    assert fwd(_desc(o=FAKE + 2)) == -1 and b"aligned" in lib.mi_last_error()
    for p in ("dout", "dq_row", "dq_col", "dk_row", "dk_col", "dv", "ws"):
        assert bwd(_desc(**{p: None})) == -1 and b"null" in lib.mi_last_error(), p
        assert bwd(_desc(**{p: FAKE + 4})) == -1 and b"aligned" in lib.mi_last_error(), p
    need = lib.mi_rcda_bwd_ws_bytes(C.byref(_desc()))
    assert bwd(_desc(ws_bytes=need - 1)) == -1 and b"workspace" in lib.mi_last_error()
    assert bwd(_desc(ws_bytes=0)) == -1 and b"workspace" in lib.mi_last_error()
    assert lib.mi_rcda_fwd(None, None) == -1 and b"null" in lib.mi_last_error()


def test_key_mean_argument_errors_without_launch():
    lib = L.lib()
    km = lambda kr=FAKE, kc=FAKE, mr=FAKE, mc=FAKE, B=2, H=5, W=7, E=64: lib.mi_rcda_key_mean(kr, kc, mr, mc, B, H, W, E, None)
    for kw in (dict(B=0), dict(H=0), dict(W=-2), dict(E=0)):
        assert km(**kw) == -1 and b"positive" in lib.mi_last_error(), kw
    assert km(E=36) == -1 and b"multiple of 8" in lib.mi_last_error()
    assert km(kr=None, kc=None) == -1 and b"null" in lib.mi_last_error()
    assert km(mr=None) == -1 and b"null" in lib.mi_last_error()
    assert km(mc=None) == -1 and b"null" in lib.mi_last_error()
    for kw in (dict(kr=FAKE + 2), dict(kc=FAKE + 8), dict(mr=FAKE + 4), dict(mc=FAKE + 2)):
        assert km(**kw) == -1 and b"aligned" in lib.mi_last_error(), kw


def test_workspace_sizes():
    """the two softmax gradients in bf16, queries padded to the 32-query step of the key-side reduction; pointers are not read"""
    lib = L.lib()
    for B, heads, Lq, H, W in ((2, 2, 70, 5, 7), (4, 8, 900, 25, 42), (4, 8, 4200, 50, 84), (1, 1, 1, 1, 1), (1, 8, 32, 96, 96)):
        d = _desc(**dict({p: None for p in PTRS}, B=B, heads=heads, L=Lq, H=H, W=W, E=heads * 32, ldq=heads * 32, ldk=heads * 32,
                         ldv=heads * 32, ldo=heads * 32))
        assert lib.mi_rcda_bwd_ws_bytes(C.byref(d)) == B * heads * (H + W) * ((Lq + 31) // 32 * 32) * 2


# ------------------------------------------------------------------ the module on the host
def test_module_state_dict_is_the_reference_s():
    gold = np.load(GOLD)
    m = MultiheadRCDA(64, 2)
    sd = m.state_dict()
    want = {k[len("param/"):]: gold[k].shape for k in gold.files if k.startswith("param/")}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert list(sd) == ["in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"]
    m.load_state_dict({k: torch.from_numpy(gold["param/" + k]).float() for k in want})
    nb = MultiheadRCDA(64, 2, bias=False)
    assert list(nb.state_dict()) == ["in_proj_weight", "out_proj.weight"] and nb.in_proj_bias is None
    assert m.embed_dim == 64 and m.num_heads == 2 and m.head_dim == 32 and m.kdim == 64 and m.vdim == 64 and m._qkv_same_embed_dim
    assert m.bias_k_row is None and m.bias_k_col is None and m.bias_v is None and m.add_zero_attn is False and m.dropout == 0.


def test_module_initialisation_statistics():
    """xavier_uniform_ over the whole [5E, E] in_proj_weight (bound sqrt(6 / (5E + E))), zero biases"""
    torch.manual_seed(0)
    m = MultiheadRCDA(256, 8)
    bound = math.sqrt(6.0 / (6 * 256))
    w = m.in_proj_weight.detach()
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.99 * bound
    assert abs(float(w.mean())) < 1e-3 and abs(float(w.std()) - bound / math.sqrt(3)) < 1e-3
    assert float(m.in_proj_bias.abs().max()) == 0 and float(m.out_proj.bias.abs().max()) == 0
    assert float(m.out_proj.weight.abs().max()) <= 1.0 / math.sqrt(256) + 1e-6       # nn.Linear's own default


def test_module_refusals_by_name():
    for kw, word in ((dict(add_bias_kv=True), "add_bias_kv"), (dict(add_zero_attn=True), "add_zero_attn"), (dict(kdim=32), "kdim"),
                     (dict(vdim=128), "vdim")):
        with pytest.raises(NotImplementedError, match=word):
            MultiheadRCDA(64, 2, **kw)
    with pytest.raises(NotImplementedError, match="head_dim"):
        MultiheadRCDA(64, 4)
    MultiheadRCDA(64, 2, kdim=64, vdim=64)
    x, k = torch.zeros(1, 3, 64), torch.zeros(1, 2, 2, 64)
    m = MultiheadRCDA(64, 2)
    with pytest.raises(NotImplementedError, match="need_weights"):
        m(x, x, k, k, k, need_weights=True)
    with pytest.raises(NotImplementedError, match="attn_mask"):
        m(x, x, k, k, k, attn_mask=torch.zeros(3, 4))
    d = MultiheadRCDA(64, 2, dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        d(x, x, k, k, k)
    # host tensors: no CPU fallback (eval mode with dropout gets as far as this)
    for mod in (m, d.eval()):
        with pytest.raises(L.MI355Error, match="device tensors"):
            mod(x, x, k, k, k)
    with pytest.raises(L.MI355Error, match="device tensors"):
        rcda_core(x, x, torch.zeros(1, 2, 64), torch.zeros(1, 2, 64), k, None, None, 2)
