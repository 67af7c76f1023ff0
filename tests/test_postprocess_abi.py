"""CPU: the C-ABI of the batched YOLOX postprocess (mi_yolox_postprocess) returns argument errors without launching,
and its workspace size follows the formula written in include/mi355_det.h."""
from yolov7_d2_amd import _lib as L

FAKE = 4096     # non-null, aligned dummy pointer: an argument error must return before anything touches memory


def _ws(B, A):
    """include/mi355_det.h: B * (8 * A * ceil(A / 64) + 72 * A + 4 * ceil(A / 256) + 8)"""
    return B * (8 * A * ((A + 63) // 64) + 72 * A + 4 * ((A + 255) // 256) + 8)


def _call(pred=FAKE, B=2, A=100, C=80, ld=85, dets=FAKE, counts=FAKE, ws=FAKE, ws_bytes=None):
    ws_bytes = _ws(max(B, 0), max(A, 1)) if ws_bytes is None else ws_bytes
    return L.lib().mi_yolox_postprocess(pred, B, A, C, ld, 0.3, 0.65, dets, counts, ws, ws_bytes, None)


def test_workspace_size_formula():
    lib = L.lib()
    for B, A in ((1, 1), (1, 64), (2, 65), (16, 8400), (16, 12600), (3, 65536), (1024, 300)):
        assert lib.mi_yolox_postprocess_ws_bytes(B, A, 80) == _ws(B, A), (B, A)
    # the worst-case suppression bitmask the header quotes: ~142 MB and ~318 MB
    assert round(16 * 8400 * 132 * 8 / 1e6) == 142 and round(16 * 12600 * 197 * 8 / 1e6) == 318
    assert lib.mi_yolox_postprocess_ws_bytes(0, 8400, 80) == 0
    for B, A, C in ((-1, 8400, 80), (16, 0, 80), (16, 65537, 80), (16, 8400, 0), (1025, 8400, 80)):
        assert lib.mi_yolox_postprocess_ws_bytes(B, A, C) == -1, (B, A, C)


def test_argument_errors_without_launch():
    lib = L.lib()
    for kw in (dict(pred=None), dict(dets=None), dict(counts=None), dict(ws=None)):
        assert _call(**kw) == -1, kw
        assert b"null" in lib.mi_last_error()
    assert _call(B=-1) == -1
    assert _call(C=0, ld=5) == -1
    assert _call(A=65537) == -1
    assert _call(A=0) == -1
    assert _call(ld=84) == -1                       # a row too short for 5 + C columns
    assert _call(ws_bytes=_ws(2, 100) - 1) == -1    # workspace smaller than the size query
    assert b"workspace" in lib.mi_last_error()
    assert _call(ws=FAKE + 4) == -1                 # not 8-byte aligned
    assert _call(B=1025, ws_bytes=_ws(1025, 100)) == -1
    assert _call(B=0) == 0                          # nothing to do: returns before any launch
