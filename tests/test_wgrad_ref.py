"""CPU: the plain weight-gradient reference of tests/wgrad_ref.py against torch autograd's conv2d weight gradient (float64) and,
for the 16-tap table of the ResNet stem, against a brute-force loop over pixels, taps and channels; and the operand contract
of make_operands (integers, zero pad channels, NaN outside the view, the exactness condition)."""
import pytest
import torch

import wgrad_ref as R
from yolov7_d2_amd.modeling.resnet import _STEM_TAPS


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W", [(6, 8), (7, 9), (6, 9), (7, 8), (1, 5)])
def test_reference_equals_autograd_conv2d(k, stride, H, W):
    N, Cin, Cout = 2, 5, 7
    oH, oW = R.conv_out(H, W, k, stride)
    g = torch.Generator().manual_seed(H * 100 + W * 10 + k + stride)
    x = torch.randn(N, H, W, Cin, generator=g, dtype=torch.float64)
    dy = torch.randn(N, oH, oW, Cout, generator=g, dtype=torch.float64)
    got = R.wgrad_reference(x, dy, R.square_taps(k), stride, Cin, Cout)
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, stride=stride, padding=k // 2).backward(dy.permute(0, 3, 1, 2))
    torch.testing.assert_close(got.view(Cout, Cin, k, k), w.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.bias_reference(dy, Cout), dy.sum((0, 1, 2)), rtol=1e-12, atol=1e-12)


def test_reference_equals_autograd_on_integer_operands_exactly():
    """the operands of the GPU test: integer sums are exact in float64 whatever the order, so the two agree bit for bit"""
    N, H, W, Cin, Cout = 3, 13, 17, 12, 20
    for k, stride in ((3, 1), (3, 2), (1, 1)):
        oH, oW = R.conv_out(H, W, k, stride)
        _, _, x, dy = R.make_operands(N, H, W, oH, oW, Cin, Cout, 16, 32, seed=k + stride)
        got = R.wgrad_reference(x, dy, R.square_taps(k), stride, Cin, Cout)
        w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, stride=stride, padding=k // 2).backward(dy.permute(0, 3, 1, 2))
        assert torch.equal(got.view(Cout, Cin, k, k), w.grad)
        assert torch.equal(got, got.round()) and float(got.abs().max()) <= 6 * N * oH * oW


def test_sixteen_tap_table_equals_a_brute_force_loop():
    """the 7x7 stride-2 stem as a 4x4 convolution over the space-to-depth image (taps -2..1, stride 1, same-size output)"""
    taps = [(a, b) for a, b, _ in _STEM_TAPS]
    assert len(taps) == 16 and taps[0] == (-2, -2) and taps[-1] == (1, 1)
    N, H, W, Cin, Cout = 2, 4, 5, 3, 2
    _, _, x, dy = R.make_operands(N, H, W, H, W, Cin, Cout, 16, 32, seed=5)
    got = R.wgrad_reference(x, dy, taps, 1, Cin, Cout)
    ref = torch.zeros(Cout, Cin, 16, dtype=torch.float64)
    for n in range(N):
        for oy in range(H):
            for ox in range(W):
                for t, (ty, tx) in enumerate(taps):
                    iy, ix = oy + ty, ox + tx
                    if 0 <= iy < H and 0 <= ix < W:
                        ref[:, :, t] += dy[n, oy, ox][:, None] * x[n, iy, ix][None, :]
    assert torch.equal(got, ref)


def test_stride_two_brute_force_and_tap_order():
    """stride 2 with an odd map and a permuted tap table: the output follows the order of `taps`"""
    N, H, W, Cin, Cout = 1, 5, 7, 2, 3
    oH, oW = R.conv_out(H, W, 3, 2)
    _, _, x, dy = R.make_operands(N, H, W, oH, oW, Cin, Cout, 16, 32, seed=9)
    taps = [(b, a) for a, b in R.square_taps(3)]
    got = R.wgrad_reference(x, dy, taps, 2, Cin, Cout)
    ref = torch.zeros(Cout, Cin, 9, dtype=torch.float64)
    for oy in range(oH):
        for ox in range(oW):
            for t, (ty, tx) in enumerate(taps):
                iy, ix = oy * 2 + ty, ox * 2 + tx
                if 0 <= iy < H and 0 <= ix < W:
                    ref[:, :, t] += dy[0, oy, ox][:, None] * x[0, iy, ix][None, :]
    assert torch.equal(got, ref)
    true = R.wgrad_reference(x, dy, R.square_taps(3), 2, Cin, Cout)
    assert torch.equal(got.view(Cout, Cin, 3, 3), true.view(Cout, Cin, 3, 3).transpose(2, 3))
    assert not torch.equal(got, true)


def test_make_operands_contract():
    N, H, W, Cin, Cout, CinPad, CoutPad = 2, 5, 6, 12, 85, 16, 96
    xb, dyb, x, dy = R.make_operands(N, H, W, H, W, Cin, Cout, CinPad, CoutPad, seed=1, ldx=48, x_off=16, ldy=192, dy_off=96)
    assert xb.dtype == torch.bfloat16 and xb.shape == (N, H, W, 48) and dyb.shape == (N, H, W, 192)
    assert torch.equal(xb[..., 16:28].double(), x) and torch.equal(dyb[..., 96:181].double(), dy)      # exact in bf16
    assert torch.equal(x, x.round()) and float(x.abs().max()) == 3 and float(dy.abs().max()) == 2
    assert (xb[..., 28:32] == 0).all() and (dyb[..., 181:192] == 0).all()                               # pad channels
    assert xb[..., :16].isnan().all() and xb[..., 32:].isnan().all() and dyb[..., :96].isnan().all()    # outside the view
    # a second view into the same buffers takes the NaN slice and leaves the first alone
    R.make_operands(N, H, W, H, W, 16, 96, 16, 96, seed=2, ldx=48, x_off=0, ldy=192, dy_off=0, xbuf=xb, dybuf=dyb)
    assert torch.equal(xb[..., 16:28].double(), x) and not xb[..., :32].isnan().any() and xb[..., 32:].isnan().all()
    with pytest.raises(AssertionError):                      # 6 * pixels >= 2^24: the sums would not be exact
        R.make_operands(700, 64, 64, 64, 64, 1, 1, 16, 32, seed=0)
