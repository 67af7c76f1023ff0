"""CPU: the float64 restatement of the grouped 3x3 convolution (tests/gconv_ref.py) equals float64 F.conv2d(groups = G) and its
autograd gradients on random data, for every served group width and both strides; its packed-image layout is checked
against the header's index formula entry by entry."""
import pytest
import torch
import torch.nn.functional as F

import gconv_ref as R

CASES = [(Cg, G, stride, H, W) for Cg, G in ((8, 3), (16, 2), (24, 2), (32, 2), (16, 1)) for stride, H, W in ((1, 5, 7), (2, 5, 7), (2, 6, 4), (1, 1, 1))]


@pytest.mark.parametrize("Cg,G,stride,H,W", CASES)
def test_reference_equals_torch_autograd(Cg, G, stride, H, W):
    g = torch.Generator().manual_seed(Cg * 100 + G * 10 + stride + H)
    C, N = Cg * G, 2
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(C, Cg, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, b, stride=stride, padding=1, groups=G)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    xh, dyh = x.detach().permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
    assert tuple(y.shape[2:]) == R.out_size(H, W, stride)
    torch.testing.assert_close(R.forward(xh, w.detach(), G, stride, b.detach()), y.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.forward(xh, w.detach(), G, stride), (y.detach() - b.detach().view(1, C, 1, 1)).permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.dgrad(dyh, w.detach(), G, stride, H, W), x.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    gw, gb = R.wgrad(xh, dyh, G, stride)
    torch.testing.assert_close(gw, w.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gb, b.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("Cg", R.SERVED_CG)
def test_packed_image_layout(Cg):
    G = 2
    C = G * Cg
    w = torch.arange(C * Cg * 9, dtype=torch.float64).reshape(C, Cg, 3, 3) + 1.0        # every entry distinct and non-zero
    wf, wd = R.packed_images(w, Cg)
    assert tuple(wf.shape) == tuple(wd.shape) == R.image_shape(C, Cg)
    _, MT, NK, _, _ = R.image_shape(C, Cg)
    assert MT == -(-Cg // 16) and NK * 4 >= 9 * Cg // 8 > (NK - 1) * 4
    for g in range(G):
        for mt in range(MT):
            for m in range(NK):
                for lane in range(64):
                    row, q = mt * 16 + (lane & 15), 4 * m + (lane >> 4)
                    for j in range(8):
                        if row >= Cg or q >= 9 * Cg // 8:
                            assert wf[g, mt, m, lane, j] == 0 and wd[g, mt, m, lane, j] == 0
                            continue
                        t, k = q // (Cg // 8), (q % (Cg // 8)) * 8 + j
                        assert wf[g, mt, m, lane, j] == w[g * Cg + row, k, t // 3, t % 3]
                        assert wd[g, mt, m, lane, j] == w[g * Cg + k, row, 2 - t // 3, 2 - t % 3]
    # every weight appears exactly once in either image
    assert sorted(wf[wf != 0].tolist()) == sorted(w.reshape(-1).tolist()) == sorted(wd[wd != 0].tolist())
