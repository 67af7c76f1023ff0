"""Float64 restatement, in plain torch, of the deformable 3x3 convolution of csrc/deform_conv.hip (detectron2's DeformConv:
unmodulated, one deformable group, groups 1) and of modeling/resnet.py's DeformBottleneckBlock, written from the definition:

  for tap t = i*3 + j, offset channel 2t is the row offset and 2t + 1 the column offset; the sample point of output pixel
  (ho, wo) is h = ho*stride - pad + i*dil + off_h (w alike), pad = dil = 1; it counts only if h > -1 && w > -1 && h < H && w < W;
  then the cell is floor(h), floor(h) + 1 (w alike), a corner outside [0, H-1] x [0, W-1] contributes zero.

The cells are floor-based and the floor is taken outside the graph, so autograd through these functions yields the backward
rule of mi_deform_col2im: d/dh = hw*(v3 - v1) + lw*(v4 - v2), the right-hand difference at an integer coordinate.
detectron2 and torchvision are not installed here: tests/test_deform_conv_ref.py pins this file with four identities instead
(zero offsets = F.conv2d, integer offsets = a convolution over shifted taps, samples at exactly -1 / H are zero, gradcheck).

`rb` rounds to bf16 where the device path stores bf16 (straight-through for autograd); `rg` rounds a gradient the same way."""
import torch
import torch.nn.functional as F


def rb(t):
    """the value after a bf16 store (float64 again); the gradient passes unchanged"""
    return t + (t.detach().to(torch.bfloat16).to(t.dtype) - t.detach())


def rg(t):
    """identity whose GRADIENT is rounded to bf16 (a gradient tensor the device stores as bf16)"""
    if t.requires_grad:
        t = t.view_as(t)
        t.register_hook(lambda g: g.to(torch.bfloat16).to(g.dtype))
    return t


def out_size(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def sample_points(offset, H, W, stride):
    """offset [N, 18, Ho, Wo] -> (h, w), each [N, Ho, Wo, 9]"""
    N, c18, Ho, Wo = offset.shape
    assert c18 == 18 and (Ho, Wo) == out_size(H, W, stride)
    off = offset.permute(0, 2, 3, 1).reshape(N, Ho, Wo, 9, 2)
    t = torch.arange(9)
    hb = (torch.arange(Ho) * stride - 1).view(1, Ho, 1, 1) + (t // 3).view(1, 1, 1, 9)
    wb = (torch.arange(Wo) * stride - 1).view(1, 1, Wo, 1) + (t % 3).view(1, 1, 1, 9)
    return hb.to(offset.dtype) + off[..., 0], wb.to(offset.dtype) + off[..., 1]


def deform_cols(x, offset, stride):
    """x [N, C, H, W], offset [N, 18, Ho, Wo] -> sampled columns [N, Ho, Wo, 9, C] (tap-major, channels inside a tap)"""
    N, C, H, W = x.shape
    h, w = sample_points(offset, H, W, stride)
    Ho, Wo = h.shape[1:3]
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    h0, w0 = torch.floor(h.detach()), torch.floor(w.detach())
    lh, lw = h - h0, w - w0
    hh, hw = 1 - lh, 1 - lw
    xf = x.permute(0, 2, 3, 1).reshape(N, H * W, C)
    n_idx = torch.arange(N).view(N, 1, 1, 1).expand(N, Ho, Wo, 9)

    def corner(hc, wc):
        ok = inside & (hc >= 0) & (hc <= H - 1) & (wc >= 0) & (wc <= W - 1)
        idx = (hc.clamp(0, H - 1) * W + wc.clamp(0, W - 1)).long()
        return xf[n_idx, idx] * ok.unsqueeze(-1).to(x.dtype)

    v1, v2, v3, v4 = corner(h0, w0), corner(h0, w0 + 1), corner(h0 + 1, w0), corner(h0 + 1, w0 + 1)
    u = lambda a: a.unsqueeze(-1)
    return ((u(hh * hw) * v1 + u(hh * lw) * v2) + u(lh * hw) * v3) + u(lh * lw) * v4


def tap_major(weight):
    """[Cout, C, 3, 3] -> [Cout, 9, C]"""
    return weight.permute(0, 2, 3, 1).reshape(weight.shape[0], 9, weight.shape[1])


def deform_conv(x, offset, weight, stride, scale=None, shift=None, relu=False, device_rounding=False):
    """y [N, Cout, Ho, Wo] = act(sum_t sum_c col[.., t, c] * (weight * scale)[o, c, t] + shift).  device_rounding: the bf16 stores
    of the device path - offsets, columns, the folded weight image, the output; and the bf16 gradient of the columns"""
    r = rb if device_rounding else (lambda t: t)
    col = deform_cols(x, r(offset), stride)
    if device_rounding:
        col = rg(rb(col))
    wf = weight if scale is None else weight * scale.view(-1, 1, 1, 1)
    y = torch.einsum("nhwtc,otc->nohw", col, tap_major(r(wf)))
    if shift is not None:
        y = y + shift.view(1, -1, 1, 1)
    if relu:
        y = torch.relu(y)
    return r(y)


def conv_norm(x, weight, scale, shift, stride, padding, relu=False, device_rounding=True):
    """Conv2d + FrozenBatchNorm2d folded as the device folds it: conv(x, bf16(W * scale)) + shift, one bf16 store"""
    r = rb if device_rounding else (lambda t: t)
    y = F.conv2d(x, r(weight * scale.view(-1, 1, 1, 1)), None, stride, padding) + shift.view(1, -1, 1, 1)
    return r(torch.relu(y) if relu else y)


def deform_block(x, p, stride, device_rounding=True):
    """DeformBottleneckBlock (stride on the 3x3).  p: conv1 / conv2 / conv3 / shortcut -> (weight, scale, shift), shortcut may be
    missing; conv2_offset -> (weight, bias)"""
    r = rb if device_rounding else (lambda t: t)
    out = conv_norm(x, *p["conv1"], 1, 0, relu=True, device_rounding=device_rounding)
    ow, ob = p["conv2_offset"]
    offset = r(F.conv2d(out, r(ow), ob, stride, 1))
    w2, s2, b2 = p["conv2"]
    out = deform_conv(out, offset, w2, stride, s2, b2, relu=True, device_rounding=device_rounding)
    out = conv_norm(out, *p["conv3"], 1, 0, device_rounding=device_rounding)
    sc = conv_norm(x, *p["shortcut"], stride, 0, device_rounding=device_rounding) if p.get("shortcut") is not None else x
    return r(torch.relu(out + sc))
