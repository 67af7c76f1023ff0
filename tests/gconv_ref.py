"""Plain float64 restatement of the grouped 3x3 convolution of include/mi355_det.h (mi_gconv_desc), written from the header's
three definitions - a zero-padded copy, shifted once per tap, one batched matmul (over the groups) per tap; no conv2d, no
autograd - so that it shares nothing with the kernels under test (csrc/conv_grouped.hip).  Tensors are NHWC; group g owns
channels [g * Cg, (g + 1) * Cg); padding 1, dilation 1, stride 1 or 2; Ho = (H - 1) // stride + 1.

    forward          y[n][oy][ox][g*Cg+co] = bias[g*Cg+co] + sum over (r, s, ci) of
                         x[n][oy*stride-1+r][ox*stride-1+s][g*Cg+ci] * w[g*Cg+co][ci][r][s]          (x = 0 outside the map)
    data gradient    dx[n][oy*stride-1+r][ox*stride-1+s][g*Cg+ci] += dy[n][oy][ox][g*Cg+co] * w[g*Cg+co][ci][r][s]
    weight gradient  gw[g*Cg+co][ci][r][s] = sum over (n, oy, ox) of dy[n][oy][ox][g*Cg+co] * x[n][oy*stride-1+r][ox*stride-1+s][g*Cg+ci]
                     gbias[c] = sum over (n, oy, ox) of dy[n][oy][ox][c]

`packed_images` is the layout mi_gconv_pack_weight must produce (the header's text).  tests/test_gconv_ref.py guards the three
functions against float64 F.conv2d(groups = G) and its autograd gradients.

The exact-integer method (tests/test_gpu_gconv_exact.py): the bf16 operands hold small integers, so every product and every
fp32 partial sum is an exact integer whatever the order of taps, octets, tiles or splits, and ANY correct kernel equals this
reference bit for bit.  `assert_exact` states the conditions, asserted on the reference before anything is launched: values
stored as bf16 are integers of magnitude <= 256, and every fp32 sum stays below 2^24 - bounded by the sum of the magnitudes
of its terms, which the caller passes as `abs_sum` (the same reference evaluated on |operands|).
"""
import torch

BF16_INT_MAX = 256
F32_INT_MAX = 2 ** 24
SERVED_CG = (8, 16, 24, 32)


def out_size(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def _padded(x):
    N, H, W, C = x.shape
    xp = torch.zeros(N, H + 2, W + 2, C, dtype=torch.float64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x.to(torch.float64)
    return xp


def _taps(xp, Ho, Wo, stride, G, Cg):
    """for each tap (r, s): the padded input shifted by the tap, [N, Ho, Wo, G, Cg]"""
    for r in range(3):
        for s in range(3):
            xs = xp[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]
            yield r, s, xs.reshape(xs.shape[0], Ho, Wo, G, Cg)


def forward(x, w, G, stride, bias=None):
    """x [N, H, W, C], w [C, Cg, 3, 3], bias [C] or None -> y [N, Ho, Wo, C] float64 (not rounded)"""
    N, H, W, C = x.shape
    Cg = C // G
    assert w.shape == (C, Cg, 3, 3) and C == G * Cg
    Ho, Wo = out_size(H, W, stride)
    w = w.to(torch.float64).reshape(G, Cg, Cg, 3, 3)                    # [g][co][ci][r][s]
    y = torch.zeros(N, Ho, Wo, G, Cg, dtype=torch.float64, device=x.device)
    for r, s, xs in _taps(_padded(x), Ho, Wo, stride, G, Cg):
        y += torch.einsum("nhwgi,goi->nhwgo", xs, w[:, :, :, r, s])
    y = y.reshape(N, Ho, Wo, C)
    return y if bias is None else y + bias.to(torch.float64)


def dgrad(dy, w, G, stride, H, W):
    """dy [N, Ho, Wo, C] -> dx [N, H, W, C] float64: the scatter form of the definition, on a padded map whose border is dropped"""
    N, Ho, Wo, C = dy.shape
    Cg = C // G
    assert (Ho, Wo) == out_size(H, W, stride)
    w = w.to(torch.float64).reshape(G, Cg, Cg, 3, 3)
    d = dy.to(torch.float64).reshape(N, Ho, Wo, G, Cg)
    dxp = torch.zeros(N, H + 2, W + 2, C, dtype=torch.float64, device=dy.device)
    for r in range(3):
        for s in range(3):
            contrib = torch.einsum("nhwgo,goi->nhwgi", d, w[:, :, :, r, s]).reshape(N, Ho, Wo, C)
            dxp[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride] += contrib
    return dxp[:, 1:H + 1, 1:W + 1].contiguous()


def wgrad(x, dy, G, stride):
    """-> (gw [C, Cg, 3, 3], gbias [C]) float64"""
    N, H, W, C = x.shape
    Cg = C // G
    Ho, Wo = out_size(H, W, stride)
    assert dy.shape == (N, Ho, Wo, C)
    d = dy.to(torch.float64).reshape(N, Ho, Wo, G, Cg)
    gw = torch.zeros(G, Cg, Cg, 3, 3, dtype=torch.float64, device=x.device)
    for r, s, xs in _taps(_padded(x), Ho, Wo, stride, G, Cg):
        gw[:, :, :, r, s] = torch.einsum("nhwgo,nhwgi->goi", d, xs)
    return gw.reshape(C, Cg, 3, 3), dy.to(torch.float64).reshape(-1, C).sum(0)


def image_shape(C, Cg):
    """[G][MT][NK][64 lanes][8]"""
    return (C // Cg, (Cg + 15) // 16, (9 * Cg // 8 + 3) // 4, 64, 8)


def packed_images(w, Cg):
    """(forward image, data-gradient image) of w [C, Cg, 3, 3] as float64 [G][MT][NK][64][8]: entry (g, mt, m, lane, j) has
    row = mt*16 + (lane & 15), octet q = 4*m + (lane >> 4), tap t = q // (Cg/8), k = (q % (Cg/8))*8 + j and holds
    w[g*Cg+row][k][t//3][t%3] (forward) or w[g*Cg+k][row][2-t//3][2-t%3] (data gradient); zero where row >= Cg or q >= 9*Cg/8"""
    C = w.shape[0]
    G, MT, NK, _, _ = image_shape(C, Cg)
    opt = Cg // 8
    w = w.to(torch.float64).reshape(G, Cg, Cg, 9)
    mt, m, lane, j = torch.meshgrid(torch.arange(MT), torch.arange(NK), torch.arange(64), torch.arange(8), indexing="ij")
    row = mt * 16 + (lane & 15)
    q = 4 * m + (lane >> 4)
    t = q // opt
    k = (q % opt) * 8 + j
    live = (row < Cg) & (q < 9 * opt)
    row, t = row.clamp(max=Cg - 1), t.clamp(max=8)
    wf = torch.where(live, w[:, row, k, t], torch.zeros((), dtype=torch.float64))
    wd = torch.where(live, w[:, k, row, 8 - t], torch.zeros((), dtype=torch.float64))
    return wf.contiguous(), wd.contiguous()


def assert_exact(value, abs_sum, bf16):
    """the method's premise for one expected result: `value` is integer-valued, `abs_sum` - the same sums over the magnitudes
    of the terms, a bound on every partial sum in any order - stays below 2^24, and a result stored as bf16 is an integer of
    magnitude <= 256"""
    assert bool((value == value.round()).all()), "the expected result is not integer-valued: the case breaks the method's premise"
    assert float(abs_sum.max()) < F32_INT_MAX, "an fp32 partial sum could reach 2^24: the case breaks the method's premise"
    assert bool((value.abs() <= abs_sum).all())
    if bf16:
        assert float(value.abs().max()) <= BF16_INT_MAX, "the expected result is not exact in bf16: the case breaks the method's premise"
