"""CPU: the C-ABI of the batched SparseInst postprocess (mi_sparseinst_infer_select / _masks / _ws_bytes) returns every
argument error without launching, and its workspace size follows the formula written in include/mi355_det.h."""
from yolov7_d2_amd import _lib as L

FAKE = 4096     # non-null, aligned dummy pointer: an argument error must return before anything touches memory


def _ws(B, N, h, w):
    """include/mi355_det.h: B * ceil(h * w / 256) * 2 * N * 4"""
    return B * ((h * w + 255) // 256) * 2 * N * 4


def _select(logits=FAKE, obj=FAKE, masks=FAKE, dtype=1, strides=None, B=2, N=40, C=80, h=16, w=20, counts=FAKE, kept=FAKE,
            scores=FAKE, labels=FAKE, ws=FAKE, ws_bytes=None):
    strides = (h * w * 64, 1, w * 64, 64) if strides is None else strides
    ws_bytes = _ws(max(B, 0), max(N, 1), max(h, 1), max(w, 1)) if ws_bytes is None else ws_bytes
    return L.lib().mi_sparseinst_infer_select(logits, obj, masks, dtype, *strides, B, N, C, h, w, 0.3, 0.45, counts, kept, scores,
                                              labels, ws, ws_bytes, None)


def _desc(n=3, h_img=104, w_img=128, Hout=80, Wout=100, out_off=0):
    d = L.mi_sparseinst_infer_desc()
    d.out_off, d.n, d.h_img, d.w_img, d.Hout, d.Wout = out_off, n, h_img, w_img, Hout, Wout
    return d


def _masks(masks=FAKE, dtype=0, strides=None, B=2, N=40, h=16, w=20, Hpad=128, Wpad=160, kept=FAKE, descs="default", out=FAKE,
           out_bytes=1 << 20, d0=None, d1=None):
    strides = (N * h * w, h * w, w, 1) if strides is None else strides
    if descs == "default":
        descs = (L.mi_sparseinst_infer_desc * 2)(d0 or _desc(), d1 or _desc(out_off=3 * 80 * 100))
    return L.lib().mi_sparseinst_infer_masks(masks, dtype, *strides, B, N, h, w, Hpad, Wpad, kept, descs, 0.45, out, out_bytes, None)


def test_workspace_size_formula():
    lib = L.lib()
    for B, N, h, w in ((1, 1, 1, 1), (2, 40, 16, 20), (8, 100, 160, 160), (3, 7, 17, 15), (0, 100, 160, 160)):
        assert lib.mi_sparseinst_infer_ws_bytes(B, N, h, w) == _ws(B, N, h, w), (B, N, h, w)
    for B, N, h, w in ((-1, 100, 160, 160), (8, 0, 160, 160), (8, 100, 0, 160), (8, 100, 160, 0)):
        assert lib.mi_sparseinst_infer_ws_bytes(B, N, h, w) == -1, (B, N, h, w)


def test_select_argument_errors_without_launch():
    lib = L.lib()
    for kw in (dict(logits=None), dict(obj=None), dict(masks=None), dict(counts=None), dict(kept=None), dict(scores=None),
               dict(labels=None), dict(ws=None)):
        assert _select(**kw) == -1, kw
        assert b"null" in lib.mi_last_error(), kw
    assert _select(B=-1) == -1
    for kw in (dict(N=0), dict(C=0), dict(h=0), dict(w=0), dict(N=-3)):
        assert _select(**kw) == -1, kw
    assert _select(dtype=2) == -1 and b"dtype" in lib.mi_last_error()
    assert _select(strides=(0, 0, 20, 1)) == -1 and b"stride" in lib.mi_last_error()
    assert _select(ws_bytes=_ws(2, 40, 16, 20) - 1) == -1 and b"workspace" in lib.mi_last_error()
    assert _select(ws=FAKE + 2) == -1
    assert _select(B=0) == 0                         # nothing to do: returns before any launch


def test_masks_argument_errors_without_launch():
    lib = L.lib()
    for kw in (dict(masks=None), dict(kept=None), dict(descs=None), dict(out=None)):
        assert _masks(**kw) == -1, kw
        assert b"null" in lib.mi_last_error(), kw
    assert _masks(B=-1) == -1
    for kw in (dict(N=0), dict(h=0), dict(w=0), dict(Hpad=0), dict(Wpad=-1)):
        assert _masks(**kw) == -1, kw
    assert _masks(dtype=3) == -1 and b"dtype" in lib.mi_last_error()
    assert _masks(strides=(0, 320, -20, 1)) == -1 and b"stride" in lib.mi_last_error()
    # descriptors: a non-positive output size, an image beyond the padded shape, counts outside 0 .. N, a result too small
    for d in (_desc(Hout=0), _desc(Wout=-5), _desc(h_img=129), _desc(w_img=161), _desc(h_img=0), _desc(n=-1), _desc(n=41)):
        assert _masks(d0=d) == -1, (d.n, d.h_img, d.w_img, d.Hout, d.Wout)
        assert b"image 0" in lib.mi_last_error()
    assert _masks(d1=_desc(w_img=161, out_off=3 * 80 * 100)) == -1 and b"image 1" in lib.mi_last_error()
    assert _masks(out_bytes=2 * 3 * 80 * 100 - 1) == -1 and b"exceed" in lib.mi_last_error()
    assert _masks(d0=_desc(out_off=-8)) == -1
    assert _masks(B=0) == 0                          # nothing to do: returns before any launch
    assert _masks(d0=_desc(n=0), d1=_desc(n=0, Hout=0)) == 0      # no kept query anywhere: nothing is launched either
