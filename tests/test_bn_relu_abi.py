"""CPU: the C-ABI of the BatchNorm + ReLU kernels (mi_bn_stats, mi_bn_relu_fwd, mi_bn_relu_bwd_reduce / _apply,
mi_bn_relu_desc_size) is exported, declared and bound, the descriptor's size agrees with the binding, and every argument error
returns -1 without launching, naming the quantity."""
import ctypes as C
import os
import re

from yolov7_d2_amd import _lib as L

FAKE = 4096     # non-null, aligned dummy pointer: an argument error must return before anything touches memory
NAMES = ["mi_bn_relu_desc_size", "mi_bn_stats", "mi_bn_relu_fwd", "mi_bn_relu_bwd_reduce", "mi_bn_relu_bwd_apply"]
NORM_PTRS = ("y", "acc", "gamma", "beta", "running_mean", "running_var", "num_batches_tracked", "scale", "shift", "mean", "invstd",
             "dacc", "dy", "dgamma", "dbeta")


def _desc(two=False, res=False, n1=None, n2=None, res_ptr=None, **kw):
    d = L.mi_bn_relu_desc()
    for i, (n, over) in enumerate(((d.n1, n1), (d.n2, n2))):
        if i == 1 and not two and not over:
            continue
        for f in NORM_PTRS:
            setattr(n, f, FAKE)
        n.count, n.ldy, n.lddy, n.nslots, n.eps, n.momentum = 128, 24, 32, 16, 1e-5, 0.1
        for k, v in (over or {}).items():
            setattr(n, k, v)
    vals = dict(res=FAKE if res else None, a=FAKE, da=FAKE, dres=FAKE if res else None, npix=128, ldres=24, lda=24, ldda=24,
                lddres=24, C=24, relu=1, accumulate=0)
    vals.update(kw)
    if res_ptr is not None:
        vals["res"] = res_ptr
    for k, v in vals.items():
        setattr(d, k, v)
    return d


def _entries():
    lib = L.lib()
    return [("fwd", lambda d: lib.mi_bn_relu_fwd(C.byref(d), None)), ("reduce", lambda d: lib.mi_bn_relu_bwd_reduce(C.byref(d), None)),
            ("apply", lambda d: lib.mi_bn_relu_bwd_apply(C.byref(d), None))]


def test_symbols_are_exported_declared_and_bound():
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "..", "include", "mi355_det.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.EXPORTS, n
        assert re.search(r"\bint %s\(" % n, header), n
    assert "typedef struct mi_bn_relu_desc" in header and "typedef struct mi_bn_relu_norm" in header


def test_descriptor_size_selfcheck():
    assert L.lib().mi_bn_relu_desc_size() == C.sizeof(L.mi_bn_relu_desc)
    assert C.sizeof(L.mi_bn_relu_desc) == 2 * C.sizeof(L.mi_bn_relu_norm) + 4 * 8 + 8 + 8 * 4
    assert C.sizeof(L.mi_bn_relu_norm) == 15 * 8 + 8 + 4 * 4 + 2 * 4


def test_argument_errors_without_launch():
    lib = L.lib()
    for name, fn in _entries():
        why = lambda: (name, lib.mi_last_error())
        assert fn(_desc(C=20)) == -1 and b"C 20" in lib.mi_last_error(), why()
        assert fn(_desc(C=0)) == -1 and b"C 0" in lib.mi_last_error(), why()
        assert fn(_desc(C=2056)) == -1 and b"C 2056" in lib.mi_last_error(), why()
        assert fn(_desc(npix=0)) == -1 and b"npix" in lib.mi_last_error(), why()
        assert fn(_desc(n1=dict(y=None))) == -1 and b"null" in lib.mi_last_error(), why()
        assert fn(_desc(n1=dict(y=FAKE + 2))) == -1 and b"aligned" in lib.mi_last_error(), why()
        assert fn(_desc(n1=dict(ldy=28))) == -1 and b"multiple of 8" in lib.mi_last_error(), why()
        assert fn(_desc(n1=dict(ldy=16))) == -1 and b"n1.y" in lib.mi_last_error(), why()
        assert fn(_desc(two=True, res=True)) == -1 and b"both" in lib.mi_last_error(), why()
        assert fn(_desc(two=True, n2=dict(ldy=36))) == -1 and b"n2.y" in lib.mi_last_error(), why()
        assert fn(_desc(two=True, n2=dict(y=FAKE + 8))) == -1 and b"aligned" in lib.mi_last_error(), why()
    fwd, reduce, apply = (fn for _, fn in _entries())
    assert fwd(_desc(a=None)) == -1 and b"null" in lib.mi_last_error()
    assert fwd(_desc(a=FAKE + 4)) == -1 and b"aligned" in lib.mi_last_error()
    assert fwd(_desc(lda=20)) == -1 and b"multiple of 8" in lib.mi_last_error()
    assert fwd(_desc(res=True, ldres=12)) == -1 and b"res" in lib.mi_last_error()
    assert fwd(_desc(res=True, res_ptr=FAKE + 2)) == -1 and b"aligned" in lib.mi_last_error()
    assert fwd(_desc(n1=dict(scale=None))) == -1 and b"scale" in lib.mi_last_error()
    assert fwd(_desc(n1=dict(gamma=None))) == -1 and b"train mode" in lib.mi_last_error()
    assert fwd(_desc(n1=dict(count=0))) == -1 and b"train mode" in lib.mi_last_error()
    for fn in (reduce, apply):
        assert fn(_desc(da=None)) == -1 and b"null da" in lib.mi_last_error()
        assert fn(_desc(da=FAKE + 2)) == -1 and b"aligned" in lib.mi_last_error()
        assert fn(_desc(ldda=12)) == -1 and b"da" in lib.mi_last_error()
        assert fn(_desc(a=None)) == -1 and b"saved output" in lib.mi_last_error()
        assert fn(_desc(n1=dict(dacc=None))) == -1 and b"dacc" in lib.mi_last_error()
        assert fn(_desc(n1=dict(mean=None))) == -1 and b"null" in lib.mi_last_error()
    assert apply(_desc(n1=dict(dy=None))) == -1 and b"dy" in lib.mi_last_error()
    assert apply(_desc(n1=dict(dy=FAKE + 2))) == -1 and b"aligned" in lib.mi_last_error()
    assert apply(_desc(n1=dict(lddy=20))) == -1 and b"multiple of 8" in lib.mi_last_error()
    assert apply(_desc(res=True, lddres=20)) == -1 and b"dres" in lib.mi_last_error()
    assert apply(_desc(n1=dict(count=0))) == -1 and b"count" in lib.mi_last_error()


def test_stats_argument_errors_without_launch():
    lib = L.lib()
    st = lambda x=FAKE, ldx=24, npix=64, Cc=24, acc=FAKE, nslots=16: lib.mi_bn_stats(x, ldx, npix, Cc, acc, nslots, None)
    assert st(Cc=12) == -1 and b"C 12" in lib.mi_last_error()
    assert st(Cc=4096) == -1 and b"C 4096" in lib.mi_last_error()
    assert st(npix=0) == -1 and b"npix" in lib.mi_last_error()
    assert st(x=None) == -1 and b"null" in lib.mi_last_error()
    assert st(acc=None) == -1 and b"null" in lib.mi_last_error()
    assert st(x=FAKE + 6) == -1 and b"aligned" in lib.mi_last_error()
    assert st(ldx=20) == -1 and b"multiple of 8" in lib.mi_last_error()
    assert st(ldx=16) == -1 and b"ldx" in lib.mi_last_error()
    assert st(acc=FAKE + 8) == -1 and b"aligned" in lib.mi_last_error()
