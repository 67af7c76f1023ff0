"""numpy fp32 restatement of the batched SparseInst inference postprocess (csrc/sparseinst_infer.hip), written from the
formulas in include/mi355_det.h: the select / rescore step and the composed 16-tap resize.  torch is used for sigmoid only."""
import numpy as np
import torch

F32 = np.float32


def sigmoid(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).sigmoid().numpy()


def src_index(n_out, n_in, clamp_n=None):
    """ATen's align_corners=False source index for every dst in range(n_out): (i0, i1, l1), all arithmetic in fp32"""
    clamp_n = n_in if clamp_n is None else clamp_n
    scale = F32(n_in) / F32(n_out)
    s = scale * (np.arange(n_out, dtype=F32) + F32(0.5)) - F32(0.5)
    s = np.maximum(s, F32(0)).astype(F32)
    a = s.astype(np.int64)
    i0 = np.minimum(a, clamp_n - 1)
    i1 = np.minimum(a + 1, clamp_n - 1)
    return i0, i1, (s - a.astype(F32)).astype(F32)


def _bilerp(ly, lx, a, b, c, d):
    hy0, wx0 = F32(1) - ly, F32(1) - lx
    return (hy0 * (wx0 * a + lx * b) + ly * (wx0 * c + lx * d)).astype(F32)


def select_rescore(logits, obj, masks, cls_thr, mask_thr):
    """per image (kept query indices ascending, rescored scores fp32, labels int64)"""
    out = []
    so = sigmoid(obj).reshape(obj.shape[0], -1)
    for b in range(logits.shape[0]):
        sc = np.sqrt(sigmoid(logits[b]) * so[b][:, None]).astype(F32)
        lab = sc.argmax(-1)                              # first maximum
        best = sc.max(-1)
        keep = np.nonzero(best > F32(cls_thr))[0]
        m = sigmoid(masks[b][keep])
        k = (m > F32(mask_thr)).astype(F32)
        num = (m * k).sum((1, 2), dtype=F32)
        den = k.sum((1, 2), dtype=F32)
        out.append((keep, (best[keep] * (num / (den + F32(1e-6)))).astype(F32), lab[keep].astype(np.int64)))
    return out


def compose_masks(m, pad_shape, img_shape, out_shape, mask_thr):
    """m: sigmoid(mask) fp32 [n, h, w] -> bool [n, Hout, Wout]: bilinear (h, w) -> pad_shape, crop to img_shape, bilinear ->
    out_shape, > mask_thr - evaluated per output pixel as 2 x 2 outer samples of 2 x 2 inner taps"""
    n, h, w = m.shape
    # inner level, for every intermediate row / column of the padded size
    y0, y1, ly = src_index(pad_shape[0], h)
    x0, x1, lx = src_index(pad_shape[1], w)
    # outer level: in = the cropped size, indices clamped to it
    Y0, Y1, LY = src_index(out_shape[0], img_shape[0])
    X0, X1, LX = src_index(out_shape[1], img_shape[1])

    def inter(iy, ix):
        """intermediate samples at rows iy [Hout] x columns ix [Wout], each a complete fp32 value"""
        ya, yb, l_y = y0[iy][:, None], y1[iy][:, None], ly[iy][:, None]
        xa, xb, l_x = x0[ix][None, :], x1[ix][None, :], lx[ix][None, :]
        return _bilerp(l_y, l_x, m[:, ya, xa], m[:, ya, xb], m[:, yb, xa], m[:, yb, xb])
    v = _bilerp(LY[:, None], LX[None, :], inter(Y0, X0), inter(Y0, X1), inter(Y1, X0), inter(Y1, X1))
    return v > F32(mask_thr)


def inference(logits, obj, masks, image_sizes, out_sizes, max_shape, cls_thr, mask_thr):
    """per image (scores, labels, bool masks or None)"""
    res = []
    for b, (keep, sc, lab) in enumerate(select_rescore(logits, obj, masks, cls_thr, mask_thr)):
        pm = None
        if len(keep):
            pm = compose_masks(sigmoid(masks[b][keep]), tuple(max_shape), tuple(image_sizes[b]), tuple(out_sizes[b]), mask_thr)
        res.append((sc, lab, pm))
    return res
