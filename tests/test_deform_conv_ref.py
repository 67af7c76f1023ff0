"""CPU: the float64 restatement of the deformable convolution (tests/deform_conv_ref.py) is pinned by four identities -
detectron2 / torchvision are not installed, so no run of their kernels stands behind it."""
import pytest
import torch
import torch.nn.functional as F

import deform_conv_ref as R


def _case(N, C, Cout, H, W, stride, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, C, 3, 3, generator=g, dtype=torch.float64)
    Ho, Wo = R.out_size(H, W, stride)
    return x, w, Ho, Wo, g


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", [(7, 9), (8, 8)])
def test_zero_offsets_equal_conv2d(stride, hw):
    x, w, Ho, Wo, _ = _case(2, 5, 4, *hw, stride, 1)
    y = R.deform_conv(x, torch.zeros(2, 18, Ho, Wo, dtype=torch.float64), w, stride)
    ref = F.conv2d(x, w, None, stride, 1)
    assert y.shape == ref.shape and float((y - ref).abs().max()) < 1e-12


@pytest.mark.parametrize("stride", [1, 2])
def test_integer_offsets_equal_a_convolution_over_shifted_taps(stride):
    """one integer shift (a, b) per tap, the same at every pixel: tap t reads the zero-padded image moved by (a_t, b_t)"""
    N, C, Cout, H, W = 2, 3, 4, 7, 9
    x, w, Ho, Wo, g = _case(N, C, Cout, H, W, stride, 2)
    sh = torch.randint(-3, 4, (9, 2), generator=g)
    sh[0], sh[8] = torch.tensor([-9, 0]), torch.tensor([0, 11])           # (far outside: the whole tap reads zero)
    offset = sh.double().reshape(18).view(1, 18, 1, 1).expand(N, 18, Ho, Wo).contiguous()
    y = R.deform_conv(x, offset, w, stride)
    P = 16
    xp = F.pad(x, (P, P, P, P))
    ref = torch.zeros_like(y)
    for t in range(9):
        i, j = t // 3, t % 3
        a, b = int(sh[t, 0]), int(sh[t, 1])
        h0, w0 = P - 1 + i + a, P - 1 + j + b
        patch = xp[:, :, h0:h0 + (Ho - 1) * stride + 1:stride, w0:w0 + (Wo - 1) * stride + 1:stride]
        ref += torch.einsum("nchw,oc->nohw", patch, w[:, :, i, j])
    assert float((y - ref).abs().max()) < 1e-12


def test_samples_at_exactly_minus_one_and_exactly_H_are_zero():
    """h = -1 and h = H lie outside the open range: zero, although one row of their cell (0 resp. H - 1) is a real row"""
    N, C, H, W = 1, 2, 5, 6
    x = torch.ones(N, C, H, W, dtype=torch.float64)
    offset = torch.zeros(N, 18, H, W, dtype=torch.float64)
    col = R.deform_cols(x, offset, 1)                  # tap 0 of output row 0 sits at h = -1; tap 6 of the last row at h = H
    assert float(col[0, 0, :, 0].abs().max()) == 0 and float(col[0, H - 1, :, 6].abs().max()) == 0
    assert float(col[0, :, 0, 0].abs().max()) == 0 and float(col[0, :, W - 1, 2].abs().max()) == 0      # w = -1, w = W
    # just inside: the bands (-1, 0) and (H - 1, H) see the border row with the weight of their distance
    o2 = offset.clone()
    o2[:, 0] = 0.25                                    # tap 0 row offset: h = -0.75 at output row 0
    o2[:, 12] = -0.25                                  # tap 6 row offset: h = H - 0.25 at the last output row
    c2 = R.deform_cols(x, o2, 1)
    assert abs(float(c2[0, 0, 2, 0, 0]) - 0.25) < 1e-15 and abs(float(c2[0, H - 1, 2, 6, 0]) - 0.25) < 1e-15
    h, w = R.sample_points(o2, H, W, 1)
    assert float(h[0, 0, 2, 0]) == -0.75 and float(h[0, H - 1, 2, 6]) == H - 0.25


def test_gradcheck_with_non_integer_offsets():
    g = torch.Generator().manual_seed(5)
    N, C, Cout, H, W = 1, 2, 2, 4, 5
    for stride in (1, 2):
        Ho, Wo = R.out_size(H, W, stride)
        x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(Cout, C, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
        # non-integer sample points well away from the cell borders (the function has kinks there): k + 0.2 .. k + 0.8
        offset = (torch.randint(-2, 3, (N, 18, Ho, Wo), generator=g).double() +
                  0.2 + 0.6 * torch.rand(N, 18, Ho, Wo, generator=g, dtype=torch.float64)).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda a, b, c: R.deform_conv(a, b, c, stride), (x, offset, w), eps=1e-6, atol=1e-6)


def test_right_hand_difference_at_an_integer_coordinate():
    """at h = 2 exactly the cell is rows 2, 3: d/dh = x[3] - x[2] (not the left-hand or the central difference)"""
    x = torch.tensor([0.0, 1.0, 3.0, 7.0, 15.0], dtype=torch.float64).view(1, 1, 5, 1).expand(1, 1, 5, 3).contiguous()
    offset = torch.zeros(1, 18, 5, 3, dtype=torch.float64, requires_grad=True)
    col = R.deform_cols(x, offset, 1)
    col[0, 2, 1, 4, 0].backward()                      # centre tap of output pixel (2, 1): h = 2, w = 1
    assert float(offset.grad[0, 8, 2, 1]) == 4.0 and float(offset.grad[0, 9, 2, 1]) == 0.0
