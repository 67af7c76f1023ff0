"""CPU: the C-ABI of the grouped 3x3 convolution (mi_gconv_fwd / _dgrad / _wgrad / _wgrad_plan / _pack_weight /
_weight_image_bytes / _desc_size) is exported, declared and bound, the descriptor's size agrees with the binding, and every
argument error - the geometry it does not serve first of all - returns -1 without launching, naming the quantity."""
import ctypes as C
import os
import re

from yolov7_d2_amd import _lib as L

FAKE = 4096     # non-null, aligned dummy pointer: an argument error must return before anything touches memory
NAMES = ["mi_gconv_desc_size", "mi_gconv_weight_image_bytes", "mi_gconv_pack_weight", "mi_gconv_fwd", "mi_gconv_dgrad",
         "mi_gconv_wgrad_plan", "mi_gconv_wgrad"]


def _desc(**kw):
    d = L.mi_gconv_desc()
    vals = dict(x=FAKE, y=FAKE, w=FAKE, bias=None, gw=FAKE, gbias=None, ws=FAKE, ws_bytes=1 << 40, ldx=64, ldy=64, N=2, H=7, W=9,
                Cin=64, Cout=64, G=4, kh=3, kw=3, stride=1, padding=1, dilation=1)
    vals.update(kw)
    for k, v in vals.items():
        setattr(d, k, v)
    return d


def _entries():
    lib = L.lib()
    return [("fwd", lambda d: lib.mi_gconv_fwd(C.byref(d), None)), ("dgrad", lambda d: lib.mi_gconv_dgrad(C.byref(d), None)),
            ("wgrad", lambda d: lib.mi_gconv_wgrad(C.byref(d), None))]


def test_symbols_are_exported_declared_and_bound():
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "..", "include", "mi355_det.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.EXPORTS, n
        assert re.search(r"\b(int|int64_t) %s\(" % n, header), n
    assert "typedef struct mi_gconv_desc" in header


def test_descriptor_size_selfcheck():
    assert L.lib().mi_gconv_desc_size() == C.sizeof(L.mi_gconv_desc)


GEOMETRY = [(dict(kh=1), b"kernel"), (dict(kw=5), b"kernel"), (dict(kh=1, kw=1), b"kernel"), (dict(stride=0), b"stride"),
            (dict(stride=3), b"stride"), (dict(padding=0), b"padding"), (dict(padding=2), b"padding"), (dict(dilation=2), b"dilation"),
            (dict(Cin=16, Cout=16, G=4), b"Cg 4"), (dict(Cin=48, Cout=48, G=4), b"Cg 12"), (dict(Cin=80, Cout=80, G=2), b"Cg 40"),
            (dict(Cin=64, Cout=128, G=4), b"square"), (dict(Cin=128, Cout=64, G=4), b"square"), (dict(Cin=64, Cout=64, G=3), b"G * Cg"),
            (dict(G=0), b"positive"), (dict(G=-2), b"positive"), (dict(Cin=0, Cout=0), b"positive")]


def test_unserved_geometry_returns_the_error_status_without_launch():
    lib = L.lib()
    for name, fn in _entries():
        for kw, word in GEOMETRY:
            assert fn(_desc(**kw)) == -1, (name, kw)
            assert word in lib.mi_last_error(), (name, kw, lib.mi_last_error())
            # the geometry is refused before any pointer is looked at
            assert fn(_desc(x=None, y=None, w=None, gw=None, ws=None, **kw)) == -1 and word in lib.mi_last_error(), (name, kw)
            assert fn(_desc(x=FAKE + 2, **kw)) == -1 and word in lib.mi_last_error(), (name, kw)
    for kw, word in GEOMETRY:
        assert lib.mi_gconv_wgrad_plan(C.byref(_desc(**kw)), None) == -1 and word in lib.mi_last_error(), kw


def test_other_argument_errors_without_launch():
    lib = L.lib()
    for name, fn in _entries():
        for kw in (dict(N=0), dict(H=0), dict(W=-1), dict(N=-3)):
            assert fn(_desc(**kw)) == -1 and b"positive" in lib.mi_last_error(), (name, kw)
        assert fn(_desc(ldx=56)) == -1 and b"ldx" in lib.mi_last_error(), name
        assert fn(_desc(ldy=32)) == -1 and b"ldy" in lib.mi_last_error(), name
        assert fn(_desc(ldx=68)) == -1 and b"multiple of 8" in lib.mi_last_error(), name
        assert fn(_desc(ldy=76)) == -1 and b"multiple of 8" in lib.mi_last_error(), name
        for kw in (dict(x=None), dict(y=None)):
            assert fn(_desc(**kw)) == -1 and b"null" in lib.mi_last_error(), (name, kw)
        for kw in (dict(x=FAKE + 2), dict(y=FAKE + 8)):
            assert fn(_desc(**kw)) == -1 and b"aligned" in lib.mi_last_error(), (name, kw)
    fwd, dgrad, wgrad = (fn for _, fn in _entries())
    for fn in (fwd, dgrad):
        assert fn(_desc(w=None)) == -1 and b"null" in lib.mi_last_error()
        assert fn(_desc(w=FAKE + 4)) == -1 and b"aligned" in lib.mi_last_error()
    assert fwd(_desc(bias=FAKE + 4)) == -1 and b"aligned" in lib.mi_last_error()
    for kw in (dict(gw=None), dict(ws=None)):
        assert wgrad(_desc(**kw)) == -1 and b"null" in lib.mi_last_error(), kw
    for kw in (dict(gw=FAKE + 2), dict(gbias=FAKE + 1), dict(ws=FAKE + 8)):
        assert wgrad(_desc(**kw)) == -1 and b"aligned" in lib.mi_last_error(), kw
    assert wgrad(_desc(ws_bytes=64)) == -1 and b"workspace" in lib.mi_last_error()


def test_plan_and_image_sizes():
    lib = L.lib()
    ns = C.c_int32(0)
    need = lib.mi_gconv_wgrad_plan(C.byref(_desc(x=None, y=None, gw=None, ws=None)), C.byref(ns))
    assert ns.value >= 1 and need == ns.value * (64 * 16 * 9 + 64) * 4
    for Cg, frags in ((8, 1 * 3), (16, 1 * 5), (24, 2 * 7), (32, 2 * 9)):
        assert lib.mi_gconv_weight_image_bytes(4 * Cg, Cg) == 4 * frags * 64 * 16
    assert lib.mi_gconv_weight_image_bytes(48, 12) == -1 and b"Cg 12" in lib.mi_last_error()
    assert lib.mi_gconv_weight_image_bytes(40, 16) == -1 and b"multiple" in lib.mi_last_error()
    pack = lambda w=FAKE, Cc=64, Cg=16, wf=FAKE, wd=FAKE: lib.mi_gconv_pack_weight(w, Cc, Cg, wf, wd, None)
    assert pack(Cg=12) == -1 and b"Cg 12" in lib.mi_last_error()
    assert pack(Cc=40) == -1 and b"multiple" in lib.mi_last_error()
    assert pack(Cc=0) == -1
    assert pack(w=None) == -1 and b"null" in lib.mi_last_error()
    assert pack(wf=None, wd=None) == -1 and b"null" in lib.mi_last_error()
    assert pack(wf=FAKE + 2) == -1 and b"aligned" in lib.mi_last_error()
