"""CPU: the C-ABI of the deformable convolution (mi_deform_im2col / _col2im / _absmax / _zero_f32 / _dx_finish) is exported, declared
and bound, and returns every argument error - a stride, padding or dilation it does not serve first of all - without launching."""
import os
import re

from yolov7_d2_amd import _lib as L

FAKE = 4096     # non-null, aligned dummy pointer: an argument error must return before anything touches memory
NAMES = ["mi_deform_im2col", "mi_deform_col2im", "mi_deform_absmax", "mi_deform_zero_f32", "mi_deform_dx_finish"]


def _im2col(x=FAKE, ldx=64, off=FAKE, ldoff=32, col=FAKE, N=2, H=7, W=9, C=64, stride=1, pad=1, dil=1):
    return L.lib().mi_deform_im2col(x, ldx, off, ldoff, col, N, H, W, C, stride, pad, dil, None)


def _col2im(dcol=FAKE, x=FAKE, ldx=64, off=FAKE, ldoff=32, dx32=FAKE, doff=FAKE, gmax=None, N=2, H=7, W=9, C=64, stride=1, pad=1, dil=1):
    return L.lib().mi_deform_col2im(dcol, x, ldx, off, ldoff, dx32, doff, gmax, N, H, W, C, stride, pad, dil, None)


def test_symbols_are_exported_declared_and_bound():
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "..", "include", "mi355_det.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.EXPORTS, n
        assert re.search(r"\bint %s\(" % n, header), n


def test_unserved_geometry_returns_the_error_status_without_launch():
    lib = L.lib()
    for fn in (_im2col, _col2im):
        for kw, word in ((dict(stride=3), b"stride"), (dict(stride=0), b"stride"), (dict(stride=4), b"stride"), (dict(pad=0), b"padding"),
                         (dict(pad=2), b"padding"), (dict(dil=2), b"dilation"), (dict(dil=0), b"dilation")):
            assert fn(**kw) == -1, kw
            assert word in lib.mi_last_error(), (kw, lib.mi_last_error())
        # the geometry is refused before anything else is looked at
        assert fn(stride=3, x=None) == -1 and b"stride" in lib.mi_last_error()


def test_other_argument_errors_without_launch():
    lib = L.lib()
    for fn in (_im2col, _col2im):
        for kw in (dict(x=None), dict(off=None)):
            assert fn(**kw) == -1 and b"null" in lib.mi_last_error(), kw
        for kw in (dict(N=0), dict(H=0), dict(W=-1), dict(C=0)):
            assert fn(**kw) == -1 and b"positive" in lib.mi_last_error(), kw
        assert fn(C=48) == -1 and b"multiple of 32" in lib.mi_last_error()
        assert fn(ldx=32) == -1 and b"ldx" in lib.mi_last_error()
        assert fn(ldoff=16) == -1 and b"ldoff" in lib.mi_last_error()
    assert _im2col(col=None) == -1 and b"null" in lib.mi_last_error()
    assert _im2col(ldx=68) == -1 and b"ldx" in lib.mi_last_error()
    assert _im2col(x=FAKE + 2) == -1 and b"aligned" in lib.mi_last_error()
    for kw in (dict(dcol=None), dict(dx32=None), dict(doff=None)):
        assert _col2im(**kw) == -1 and b"null" in lib.mi_last_error(), kw
    assert _col2im(dx32=FAKE + 2) == -1 and b"misaligned" in lib.mi_last_error()
    assert _col2im(gmax=FAKE + 2) == -1 and b"misaligned" in lib.mi_last_error()
    assert lib.mi_deform_absmax(None, 64, FAKE, None) == -1 and lib.mi_deform_absmax(FAKE, 64, None, None) == -1 and b"null" in lib.mi_last_error()
    assert lib.mi_deform_absmax(FAKE, 12, FAKE, None) == -1 and b"multiple of 8" in lib.mi_last_error()
    assert lib.mi_deform_absmax(FAKE + 2, 64, FAKE, None) == -1 and b"aligned" in lib.mi_last_error()
    assert lib.mi_deform_zero_f32(None, 64, None) == -1 and b"null" in lib.mi_last_error()
    assert lib.mi_deform_zero_f32(FAKE, 6, None) == -1 and b"multiple of 4" in lib.mi_last_error()
    assert lib.mi_deform_zero_f32(FAKE, 0, None) == -1
    assert lib.mi_deform_zero_f32(FAKE + 4, 64, None) == -1 and b"aligned" in lib.mi_last_error()
    fin = lambda dx32=FAKE, mask=None, ldmask=0, dx=FAKE, lddx=64, npix=10, C=64: lib.mi_deform_dx_finish(dx32, mask, ldmask, dx, lddx, npix, C, None)
    assert fin(dx32=None) == -1 and fin(dx=None) == -1 and b"null" in lib.mi_last_error()
    assert fin(npix=0) == -1 and b"positive" in lib.mi_last_error()
    assert fin(C=12) == -1 and b"multiple of 8" in lib.mi_last_error()
    assert fin(lddx=32) == -1 and b"lddx" in lib.mi_last_error()
    assert fin(mask=FAKE, ldmask=32) == -1 and b"ldmask" in lib.mi_last_error()
    assert fin(dx=FAKE + 8) == -1 and b"aligned" in lib.mi_last_error()
