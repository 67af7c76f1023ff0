"""Plain float64 restatement of the convolution weight gradient of include/mi355_det.h (mi_wgrad_desc):

    g[co][ci][t] = sum over output pixels p of  dy[p][co] * x[p * stride + tap_t][ci],   x = 0 outside the map

written from that definition - a zero-padded copy of x, shifted once per tap, one matmul per tap; no conv2d, no autograd -
so that it shares nothing with the kernel under test (csrc/conv_wgrad.hip) nor with the library the other weight-gradient
tests compare against.  tests/test_wgrad_ref.py guards it: torch autograd's conv2d weight gradient in float64 for 1x1 / 3x3,
stride 1 / 2, odd and even maps, and a brute-force triple loop for the 16-tap table.

The exact-integer method (tests/test_gpu_wgrad_exact.py): `make_operands` fills the bf16 operands with small integers
(|x| <= 3, |dy| <= 2).  Every product is then exact in fp32 and every partial sum - in whatever order a split-K layout, an LDS
ring or a block order adds them - is an integer of magnitude <= 6 * pixels < 2^24, so exact too: ANY correct configuration
of the kernel equals this reference bit for bit, and one wrong pixel, tap, channel or split does not.
"""
import torch

X_MAX, DY_MAX = 3, 2          # operand ranges of make_operands: |dy * x| <= 6 per pixel


def conv_out(H, W, k, stride):
    """output map of a k x k convolution with padding k // 2"""
    pad = k // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def square_taps(k):
    """the (tap_dy, tap_dx) table of a k x k convolution with padding k // 2, row-major (the OIHW order of the gradient)"""
    return [(r - k // 2, s - k // 2) for r in range(k) for s in range(k)]


def wgrad_reference(x, dy, taps, stride, Cin, Cout):
    """x [N, H, W, >= Cin], dy [N, outH, outW, >= Cout] (any dtype; channels past Cin / Cout are ignored), taps a list of
    (tap_dy, tap_dx).  Returns float64 [Cout][Cin][len(taps)] in the order of `taps`."""
    x = x[..., :Cin].to(torch.float64)
    dy = dy[..., :Cout].to(torch.float64)
    N, H, W, _ = x.shape
    _, oH, oW, _ = dy.shape
    lo_y = max(0, -min(t[0] for t in taps))
    lo_x = max(0, -min(t[1] for t in taps))
    hi_y = max(0, (oH - 1) * stride + max(t[0] for t in taps) - (H - 1))
    hi_x = max(0, (oW - 1) * stride + max(t[1] for t in taps) - (W - 1))
    xp = torch.zeros(N, H + lo_y + hi_y, W + lo_x + hi_x, Cin, dtype=torch.float64)
    xp[:, lo_y:lo_y + H, lo_x:lo_x + W] = x
    dyf = dy.reshape(N * oH * oW, Cout)
    g = torch.empty(Cout, Cin, len(taps), dtype=torch.float64)
    for t, (ty, tx) in enumerate(taps):
        y0, x0 = ty + lo_y, tx + lo_x
        xs = xp[:, y0:y0 + (oH - 1) * stride + 1:stride, x0:x0 + (oW - 1) * stride + 1:stride]
        assert xs.shape[1:3] == (oH, oW), (xs.shape, oH, oW)
        g[:, :, t] = dyf.t() @ xs.reshape(N * oH * oW, Cin)
    return g


def bias_reference(dy, Cout):
    """the bias gradient: column sums of dy over all pixels, float64 [Cout]"""
    return dy[..., :Cout].to(torch.float64).reshape(-1, Cout).sum(0)


def make_operands(N, H, W, outH, outW, Cin, Cout, CinPad, CoutPad, seed, ldx=None, x_off=0, ldy=None, dy_off=0,
                  xbuf=None, dybuf=None):
    """bf16 NHWC buffers for one descriptor: xbuf [N, H, W, ldx] and dybuf [N, outH, outW, ldy], the views at channel
    offsets x_off / dy_off.  Inside the views: integers in [-3, 3] (x) and [-2, 2] (dy) in the real channels, ZERO in the pad
    channels [Cin, CinPad) and [Cout, CoutPad) (the header's contract).  Everything else of a buffer allocated here is NaN:
    the channels past the view (ld > CPad) and the neighbouring slices of a wider buffer must never be loaded.  Pass
    xbuf / dybuf to place a further view into buffers of an earlier call (slices that share one map).
    Returns (xbuf, dybuf, x, dy) with x / dy the float64 [.., Cin] / [.., Cout] contents of the views."""
    assert N * outH * outW * (X_MAX * DY_MAX) < 2 ** 24, "the sums would not be exact in fp32"
    ldx = CinPad if ldx is None else ldx
    ldy = CoutPad if ldy is None else ldy
    assert Cin <= CinPad and x_off + CinPad <= ldx and Cout <= CoutPad and dy_off + CoutPad <= ldy
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-X_MAX, X_MAX + 1, (N, H, W, Cin), generator=g).to(torch.float64)
    dy = torch.randint(-DY_MAX, DY_MAX + 1, (N, outH, outW, Cout), generator=g).to(torch.float64)
    if xbuf is None:
        xbuf = torch.full((N, H, W, ldx), float("nan"), dtype=torch.bfloat16)
    if dybuf is None:
        dybuf = torch.full((N, outH, outW, ldy), float("nan"), dtype=torch.bfloat16)
    assert xbuf.shape == (N, H, W, ldx) and dybuf.shape == (N, outH, outW, ldy)
    xbuf[..., x_off:x_off + CinPad] = 0
    xbuf[..., x_off:x_off + Cin] = x.to(torch.bfloat16)
    dybuf[..., dy_off:dy_off + CoutPad] = 0
    dybuf[..., dy_off:dy_off + Cout] = dy.to(torch.bfloat16)
    return xbuf, dybuf, x, dy
