"""Plain float64 restatement of the forward / data-gradient convolution of include/mi355_det.h (mi_conv_desc), written from
the header's definition - a zero-padded copy of x, shifted once per tap, one matmul per tap; no conv2d, no autograd - so that
it shares nothing with the kernels under test (csrc/conv_igemm*, conv1x1_stream*, conv3x3_ws*):

    r[n][gy][gx][co] = sum over taps t and input channels ci of
                       x[n][gy * in_stride + tap_dy[t]][gx * in_stride + tap_dx[t]][ci] * w[tap_w[t]][co][ci]     (x = 0 outside the map)

for gy < gridH, gx < gridW, stored at the output pixel (gy * out_stride + out_oy, gx * out_stride + out_ox); pixels of y the
grid does not visit keep their value.  The epilogues in the header's order (include/mi355_det.h:52-63): fp32 bias, MI_CONV_RELU,
the store rounding (bf16 unless MI_CONV_OUT_F32), MI_CONV_ACCUM as bf16(bf16(r) + old) (fp32: r + old), MI_CONV_ADDRELU as
max(bf16(bf16(r + bias) + aux), 0), MI_CONV_RELUMASK as (aux > 0 ? value : 0), then the statistics of the STORED values:
(sum v, sum v^2) per channel, or under MI_CONV_BNBWD (sum dz, sum dz * xhat) with dz = v (bn_act = 0) and
xhat = (bn_y - mean) * invstd.

`dgrad_scatter` is the whole-layer data gradient in scatter form, `forward_layer` the whole-layer forward in gather form.
tests/test_conv_ref.py guards all three against float64 torch autograd.

The exact-integer method (tests/test_gpu_conv_exact.py): the bf16 operands hold small integers, every product and every fp32
partial sum is an exact integer whatever the order of k-chunks, taps, waves or tiles, so ANY correct configuration of any of
the three kernel families equals this reference bit for bit.  `assert_exact` states the conditions (they are asserted on the
reference before anything is launched): bf16 values are integers of magnitude <= 256, fp32 values below 2^24, and per channel
sum |v| and sum v^2 over all stored pixels below 2^24 (every fp32 partial sum of the statistics then is, too).

Every function works on CPU or device tensors alike (plain indexing and matmul): the larger shapes are evaluated on the device.
"""
import torch

ACCUM, OUT_F32, BNBWD, RELU, RELUMASK, ADDRELU = 1, 2, 4, 8, 16, 32      # MI_CONV_* of include/mi355_det.h
BF16_INT_MAX = 256            # bf16 holds every integer up to 2^8
F32_INT_MAX = 2 ** 24


def bf16_round(t):
    """the value a bf16 store keeps, as float64"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def square_taps(k, pad=None):
    """forward tap table (tap_dy, tap_dx, tap_w) of a k x k convolution with padding `pad` (default k // 2), row-major"""
    pad = k // 2 if pad is None else pad
    return [(r - pad, s - pad, r * k + s) for r in range(k) for s in range(k)]


def dgrad_taps_s1(k, pad=None):
    """data-gradient table of a stride-1 k x k convolution: the out-gradient pixel of weight (r, s) is input + (pad - r, pad - s)"""
    pad = k // 2 if pad is None else pad
    return [(pad - r, pad - s, r * k + s) for r in range(k) for s in range(k)]


def conv_out(H, W, k, stride, pad=None):
    pad = k // 2 if pad is None else pad
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def fwd_slabs(w_oihw):
    """OIHW master -> the forward descriptor's w[tap][co][ci] (float64)"""
    Co, Ci, KH, KW = w_oihw.shape
    return w_oihw.to(torch.float64).reshape(Co, Ci, KH * KW).permute(2, 0, 1).contiguous()


def dgrad_slabs(w_oihw):
    """OIHW master -> the data-gradient descriptor's w[tap][ci][co]: the roles of the channel counts are swapped"""
    Co, Ci, KH, KW = w_oihw.shape
    return w_oihw.to(torch.float64).reshape(Co, Ci, KH * KW).permute(2, 1, 0).contiguous()


def packed_image(slabs, K8, CoutPad):
    """the packed bf16 image [slab][K8][CoutPad][8] of w[slab][co][ci] as float64, pad entries zero (what
    mi_pack_conv_weight must produce for either image)"""
    S, Co, Ci = slabs.shape
    full = torch.zeros(S, CoutPad, K8 * 8, dtype=torch.float64, device=slabs.device)
    full[:, :Co, :Ci] = slabs
    return full.reshape(S, CoutPad, K8, 8).permute(0, 2, 1, 3).contiguous()


def gather(x, w, taps, gridH, gridW, in_stride):
    """r [N, gridH, gridW, Cout] float64: the sum over taps and channels.  x [N, H, W, K] (K >= w.shape[2]: further channels
    are ignored), w [slabs, Cout, Kw], taps (tap_dy, tap_dx, tap_w)"""
    Kw = w.shape[2]
    x = x[..., :Kw].to(torch.float64)
    w = w.to(torch.float64)
    N, H, W, _ = x.shape
    lo_y = max(0, -min(t[0] for t in taps))
    lo_x = max(0, -min(t[1] for t in taps))
    hi_y = max(0, (gridH - 1) * in_stride + max(t[0] for t in taps) - (H - 1))
    hi_x = max(0, (gridW - 1) * in_stride + max(t[1] for t in taps) - (W - 1))
    xp = torch.zeros(N, H + lo_y + hi_y, W + lo_x + hi_x, Kw, dtype=torch.float64, device=x.device)
    xp[:, lo_y:lo_y + H, lo_x:lo_x + W] = x
    r = torch.zeros(N, gridH, gridW, w.shape[1], dtype=torch.float64, device=x.device)
    for (ty, tx, tw) in taps:
        y0, x0 = ty + lo_y, tx + lo_x
        assert y0 >= 0 and x0 >= 0
        xs = xp[:, y0:y0 + (gridH - 1) * in_stride + 1:in_stride, x0:x0 + (gridW - 1) * in_stride + 1:in_stride]
        assert xs.shape[1:3] == (gridH, gridW), (xs.shape, gridH, gridW)
        r += xs @ w[tw].t()
    return r


def conv_reference(x, w, taps, y_old, gridH, gridW, in_stride=1, out_stride=1, out_oy=0, out_ox=0, flags=0, bias=None,
                   aux=None, bn_y=None, bn_mean=None, bn_invstd=None, want_stats=False):
    """the descriptor-level reference.  y_old [N, outH, outW, Cout] float64: the content of the output view before the launch
    (any values, NaN included, where the launch does not accumulate).  aux: the second tensor of MI_CONV_ADDRELU /
    MI_CONV_RELUMASK, bn_y / bn_mean / bn_invstd: the operands of MI_CONV_BNBWD (bn_act = 0), all [N, outH, outW, Cout] / [Cout]
    float64.  Returns (y_new, stats): y_new = y_old with the visited pixels replaced, stats = None or float64 [Cout][2]."""
    r = gather(x, w, taps, gridH, gridW, in_stride)
    ys = slice(out_oy, out_oy + (gridH - 1) * out_stride + 1, out_stride)
    xs = slice(out_ox, out_ox + (gridW - 1) * out_stride + 1, out_stride)
    assert y_old[:, ys, xs].shape == r.shape, (y_old.shape, r.shape)
    store = (lambda t: t.to(torch.float32).to(torch.float64)) if flags & OUT_F32 else bf16_round
    if bias is not None:
        r = r + bias.to(torch.float64)
    if flags & RELU:
        r = r.clamp(min=0)
    v = store(r)
    if flags & ACCUM:
        v = store(v + y_old[:, ys, xs])
    if flags & ADDRELU:
        v = store(store(v + aux[:, ys, xs]).clamp(min=0))
    if flags & RELUMASK:
        v = torch.where(aux[:, ys, xs] > 0, v, torch.zeros_like(v))
    y_new = y_old.clone()
    y_new[:, ys, xs] = v
    stats = None
    if want_stats:
        C = v.shape[-1]
        if flags & BNBWD:
            xhat = (bn_y[:, ys, xs] - bn_mean) * bn_invstd
            stats = torch.stack([v.reshape(-1, C).sum(0), (v * xhat).reshape(-1, C).sum(0)], 1)
        else:
            stats = torch.stack([v.reshape(-1, C).sum(0), (v * v).reshape(-1, C).sum(0)], 1)
    return y_new, stats


def forward_layer(x, w_oihw, stride, pad=None):
    """whole-layer forward, gather form: y [N, outH, outW, Cout] float64 of x [N, H, W, Cin] and the OIHW weight"""
    k = w_oihw.shape[2]
    oH, oW = conv_out(x.shape[1], x.shape[2], k, stride, pad)
    return gather(x, fwd_slabs(w_oihw), square_taps(k, pad), oH, oW, stride)


def dgrad_scatter(dy, w_oihw, stride, H, W, pad=None):
    """whole-layer data gradient, scatter form: dx[n, oy*s + r - pad, ox*s + c - pad, ci] += dy[n, oy, ox, co] * w[co, ci, r, c].
    dy [N, outH, outW, >= Cout]; returns float64 [N, H, W, Cin]"""
    Co, Ci, KH, KW = w_oihw.shape
    pad = KH // 2 if pad is None else pad
    dy = dy[..., :Co].to(torch.float64)
    w = w_oihw.to(torch.float64).to(dy.device)
    N, oH, oW, _ = dy.shape
    dx = torch.zeros(N, H, W, Ci, dtype=torch.float64, device=dy.device)
    for r in range(KH):
        for c in range(KW):
            contrib = dy @ w[:, :, r, c]                       # [N, oH, oW, Ci]
            oy = [o for o in range(oH) if 0 <= o * stride + r - pad < H]
            ox = [o for o in range(oW) if 0 <= o * stride + c - pad < W]
            if not oy or not ox:
                continue
            iy0, ix0 = oy[0] * stride + r - pad, ox[0] * stride + c - pad
            dx[:, iy0:iy0 + (len(oy) - 1) * stride + 1:stride, ix0:ix0 + (len(ox) - 1) * stride + 1:stride] += \
                contrib[:, oy[0]:oy[-1] + 1, ox[0]:ox[-1] + 1]
    return dx


def dgrad_s2_classes(H, W):
    """the four parity-class launches of a stride-2 3x3 (pad 1) data gradient, as yolov7_d2_amd/plan.py builds them
    (PlanBuilder.dgrad_cmds): [(taps, out_oy, out_ox, gridH, gridW)] - written out a second time here on purpose, from the
    definition: output row iy = 2 * gy + py receives weight row r from out-gradient row (iy + 1 - r) / 2 when that is whole:
    py = 0: r = 1 at gy;  py = 1: r = 0 at gy + 1 and r = 2 at gy"""
    cls = {0: [(1, 0)], 1: [(0, 1), (2, 0)]}
    out = []
    for py in (0, 1):
        for px in (0, 1):
            taps = [(oy, ox, r * 3 + s) for (r, oy) in cls[py] for (s, ox) in cls[px]]
            out.append((taps, py, px, (H - py + 1) // 2, (W - px + 1) // 2))
    return out


def assert_exact(y, stats=None, f32=False):
    """the method's premise for one expected result (NaN = never written, ignored): every stored value is an integer that the
    output format holds exactly, and the statistics' partial sums stay below 2^24"""
    v = y[~y.isnan()]
    assert bool((v == v.round()).all()), "the expected output is not integer-valued: the case breaks the method's premise"
    lim = F32_INT_MAX if f32 else BF16_INT_MAX
    assert float(v.abs().max() if v.numel() else 0) <= (lim - 1 if f32 else lim), \
        "the expected output is not exact in the output format: the case breaks the method's premise"
    if stats is not None:
        assert float(stats.abs().max()) < F32_INT_MAX and bool((stats == stats.round()).all()), \
            "the expected statistics are not exact in fp32: the case breaks the method's premise"


def assert_stats_premise(v, weight=None):
    """per channel, sum |v| and sum v^2 (or sum |v * weight| for the BatchNorm-backward sums) over ALL stored pixels of the
    tensor stay below 2^24: every fp32 partial sum - of a tile, of a persistent block that walks many tiles - is then exact"""
    C = v.shape[-1]
    v = v.nan_to_num(0.0)
    a = v.abs().reshape(-1, C).sum(0).max()
    b = ((v * v) if weight is None else (v * weight).abs()).reshape(-1, C).sum(0).max()
    assert float(a) < F32_INT_MAX and float(b) < F32_INT_MAX, "the statistics would not be exact in fp32"
