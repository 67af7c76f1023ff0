"""CPU: the C-ABI of the ResNet-vd shortcut pool (mi_avgpool2x2s2_fwd / _bwd) returns every argument error without
launching."""
from yolov7_d2_amd import _lib as L

FAKE = 4096     # non-null, aligned dummy pointer: an argument error must return before anything touches memory


def _fwd(x=FAKE, ldx=64, y=FAKE, ldy=64, N=2, H=8, W=12, C=64):
    return L.lib().mi_avgpool2x2s2_fwd(x, ldx, y, ldy, N, H, W, C, None)


def _bwd(dy=FAKE, lddy=64, dx=FAKE, lddx=64, mask=None, ldmask=0, accumulate=0, N=2, H=8, W=12, C=64):
    return L.lib().mi_avgpool2x2s2_bwd(dy, lddy, dx, lddx, mask, ldmask, accumulate, N, H, W, C, None)


def test_forward_argument_errors_without_launch():
    lib = L.lib()
    for kw in (dict(x=None), dict(y=None)):
        assert _fwd(**kw) == -1, kw
        assert b"null" in lib.mi_last_error(), kw
    for kw in (dict(N=0), dict(H=0), dict(W=-1), dict(C=0), dict(N=-2)):
        assert _fwd(**kw) == -1, kw
        assert b"positive" in lib.mi_last_error(), kw
    assert _fwd(C=60, ldx=64, ldy=64) == -1 and b"multiple of 8" in lib.mi_last_error()
    for kw in (dict(ldx=68), dict(ldy=68), dict(ldx=56), dict(ldy=32), dict(ldx=0)):
        assert _fwd(**kw) == -1, kw
        assert b"stride" in lib.mi_last_error(), kw
    assert _fwd(x=FAKE + 2) == -1 and b"aligned" in lib.mi_last_error()
    assert _fwd(y=FAKE + 8) == -1 and b"aligned" in lib.mi_last_error()


def test_backward_argument_errors_without_launch():
    lib = L.lib()
    for kw in (dict(dy=None), dict(dx=None)):
        assert _bwd(**kw) == -1, kw
        assert b"null" in lib.mi_last_error(), kw
    for kw in (dict(N=0), dict(H=-3), dict(W=0), dict(C=0)):
        assert _bwd(**kw) == -1, kw
        assert b"positive" in lib.mi_last_error(), kw
    assert _bwd(C=12, lddy=16, lddx=16) == -1 and b"multiple of 8" in lib.mi_last_error()
    for kw in (dict(lddy=68), dict(lddx=68), dict(lddy=56), dict(lddx=8)):
        assert _bwd(**kw) == -1, kw
        assert b"stride" in lib.mi_last_error(), kw
    for kw in (dict(mask=FAKE, ldmask=0), dict(mask=FAKE, ldmask=60), dict(mask=FAKE, ldmask=32)):
        assert _bwd(**kw) == -1, kw
        assert b"ldmask" in lib.mi_last_error(), kw
    assert _bwd(dx=FAKE + 4) == -1 and b"aligned" in lib.mi_last_error()
    assert _bwd(mask=FAKE + 6, ldmask=64) == -1 and b"aligned" in lib.mi_last_error()
