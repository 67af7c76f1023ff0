"""CPU, no device: the C ABI of the SMCA attention (csrc/mha.hip: mi_smca_desc_size / _fwd / _bwd) is exported, declared and
bound, the descriptor's size agrees with the binding, and every argument error returns -1 without launching and names the
quantity; smca_core refuses host tensors by name (its shape refusals need device tensors: tests/test_gpu_smca_exact.py)."""
import ctypes as C
import os
import re

import pytest
import torch

from yolov7_d2_amd import _lib as L
from yolov7_d2_amd.modeling import smca_core

FAKE = 4096     # non-null, aligned dummy pointer: an argument error must return before anything touches memory
NAMES = ["mi_smca_desc_size", "mi_smca_fwd", "mi_smca_bwd"]
FWD_PTRS = ("q", "k", "v", "point", "coef", "o", "lse")
BWD_PTRS = ("dout", "delta", "dq", "dk", "dv", "dpoint", "dcoef")


def _desc(**kw):
    d = L.mi_smca_desc()
    vals = dict({p: FAKE for p in FWD_PTRS + BWD_PTRS}, mask=None, o_f32=None, seed=0, B=2, H=2, Lq=21, Lk=135, E=64, ldq=64, ldk=64,
                map_h=5, map_w=27, scale=32 ** -0.5, inv_smooth=0.125, drop_p=0.0)
    vals.update(kw)
    for k, v in vals.items():
        setattr(d, k, v)
    return d


def _entries():
    lib = L.lib()
    return [("fwd", lambda d: lib.mi_smca_fwd(C.byref(d), None)), ("bwd", lambda d: lib.mi_smca_bwd(C.byref(d), None))]


def test_symbols_are_exported_declared_and_bound():
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "..", "include", "mi355_det.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.EXPORTS, n
        assert re.search(r"\bint %s\(" % n, header), n
    assert "typedef struct mi_smca_desc" in header


def test_descriptor_size_selfcheck():
    assert L.lib().mi_smca_desc_size() == C.sizeof(L.mi_smca_desc) == 16 * 8 + 8 + 10 * 4 + 4 * 4


ERRORS = [(dict(E=48), b"must be H*32"), (dict(H=3), b"must be H*32"), (dict(B=0), b"must be H*32"), (dict(Lq=0), b"must be H*32"),
          (dict(map_h=5, map_w=26), b"map_h * map_w"), (dict(map_h=0, map_w=135), b"map_h * map_w"), (dict(Lk=136), b"map_h * map_w"),
          (dict(q=FAKE + 8), b"aligned"), (dict(k=FAKE + 2), b"aligned"), (dict(v=FAKE + 4), b"aligned"),
          (dict(point=FAKE + 2), b"aligned"), (dict(coef=FAKE + 1), b"aligned"), (dict(lse=FAKE + 2), b"aligned"),
          (dict(o_f32=FAKE + 4), b"aligned"),
          (dict(Lq=1 << 16, Lk=1 << 16, map_h=1 << 8, map_w=1 << 8), b"below 2^32"),
          (dict(ldq=32), b"ldq"), (dict(ldk=68), b"multiples of 8"),
          (dict(drop_p=1.0), b"dropout p"), (dict(drop_p=-0.1), b"dropout p"), (dict(drop_p=1.5), b"dropout p"),
          (dict(drop_p=float("nan")), b"dropout p"), (dict(drop_p=float("inf")), b"dropout p"), (dict(drop_p=float("-inf")), b"dropout p"),
          (dict(inv_smooth=0.0), b"inv_smooth"), (dict(inv_smooth=-1.0), b"inv_smooth"), (dict(inv_smooth=float("inf")), b"inv_smooth"),
          (dict(inv_smooth=float("nan")), b"inv_smooth")]


def test_argument_errors_return_the_error_status_without_launch():
    lib = L.lib()
    for name, fn in _entries():
        for kw, word in ERRORS:
            assert fn(_desc(**kw)) == -1, (name, kw)
            assert word in lib.mi_last_error(), (name, kw, lib.mi_last_error())
        for p in ("q", "k", "v", "point", "coef", "lse", "o"):
            assert fn(_desc(**{p: None})) == -1 and b"null" in lib.mi_last_error(), (name, p)
    bwd = _entries()[1][1]
    for p in BWD_PTRS:
        assert bwd(_desc(**{p: None})) == -1 and b"null" in lib.mi_last_error(), p
    for p in ("dout", "dq", "dk", "o"):
        assert bwd(_desc(**{p: FAKE + 8})) == -1 and b"aligned" in lib.mi_last_error(), p
    for p in ("delta", "dpoint", "dcoef"):
        assert bwd(_desc(**{p: FAKE + 2})) == -1 and b"aligned" in lib.mi_last_error(), p
    assert lib.mi_smca_fwd(None, None) == -1 and b"null" in lib.mi_last_error()
    assert lib.mi_smca_bwd(None, None) == -1 and b"null" in lib.mi_last_error()


def test_core_refuses_host_tensors_by_name():
    q, k = torch.zeros(3, 1, 64), torch.zeros(6, 1, 64)
    with pytest.raises(L.MI355Error, match="device tensors"):
        smca_core(q, k, k, torch.zeros(3, 1, 2, 2), torch.zeros(3, 1, 2, 3), (2, 3), 8.0, None, 2)
