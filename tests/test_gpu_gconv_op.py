"""GPU (-m gpu): torch.ops.mi355.conv2d_grouped with autograd, and ops.patch_grouped_convs, against float64
F.conv2d(groups = G) and its autograd gradients: exactly on integer-valued operands, within the relative-L2 bound that
tests/test_ops_boundary.py applies to mi355::conv2d (1e-2) on random normal operands rounded to bf16."""
import pytest
import torch
import torch.nn.functional as F

import yolov7_d2_amd  # noqa: F401
from yolov7_d2_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (Cg, G, H, W, stride)
SHAPES = [(8, 3, 9, 13, 1), (16, 4, 16, 16, 2), (24, 2, 9, 13, 2), (32, 2, 8, 12, 1)]


def _reference(x, w, b, dy, stride, G):
    """float64 F.conv2d(groups) and its autograd gradients of the given (already rounded) operands"""
    x64 = x.detach().double().cpu().requires_grad_(True)
    w64 = w.detach().double().cpu().requires_grad_(True)
    b64 = None if b is None else b.detach().double().cpu().requires_grad_(True)
    y = F.conv2d(x64, w64, b64, stride=stride, padding=1, groups=G)
    y.backward(dy.detach().double().cpu())
    return y.detach(), x64.grad, w64.grad, (None if b is None else b64.grad)


def _operands(Cg, G, H, W, stride, integer, bias=True, seed=0):
    g = torch.Generator().manual_seed(seed + Cg + 7 * G + H)
    C, N = Cg * G, 2
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if integer:
        x = torch.randint(-2, 3, (N, C, H, W), generator=g).float()
        w = torch.randint(-1, 2, (C, Cg, 3, 3), generator=g).float()
        b = torch.randint(-3, 4, (C,), generator=g).float()
        dy = torch.randint(-2, 3, (N, C, Ho, Wo), generator=g).float()
    else:
        x = torch.randn(N, C, H, W, generator=g)
        w = torch.randn(C, Cg, 3, 3, generator=g) / (3.0 * Cg ** 0.5)
        b = torch.randn(C, generator=g)
        dy = torch.randn(N, C, Ho, Wo, generator=g)
    x = x.to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = dy.to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return x, w.to(DEV), (b.to(DEV) if bias else None), dy


@pytest.mark.parametrize("Cg,G,H,W,stride", SHAPES)
def test_integer_operands_are_exact(Cg, G, H, W, stride):
    x, w, b, dy = _operands(Cg, G, H, W, stride, integer=True)
    x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    y = torch.ops.mi355.conv2d_grouped(x, w, b, stride, 1, G)
    y.backward(dy)
    ry, rdx, rgw, rgb = _reference(x, w, b, dy, stride, G)
    assert float(ry.abs().max()) <= 256 and float(rdx.abs().max()) <= 256      # the exact-integer premise (bf16 stores)
    assert y.dtype == torch.bfloat16 and y.shape == ry.shape and w.grad.shape == w.shape and w.grad.dtype == torch.float32
    assert torch.equal(y.detach().double().cpu(), ry)
    assert torch.equal(x.grad.double().cpu(), rdx)
    assert torch.equal(w.grad.double().cpu(), rgw)
    assert torch.equal(b.grad.double().cpu(), rgb)


@pytest.mark.parametrize("Cg,G,H,W,stride", SHAPES)
def test_random_operands_within_the_conv2d_bound(Cg, G, H, W, stride):
    x, w, b, dy = _operands(Cg, G, H, W, stride, integer=False)
    x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    y = torch.ops.mi355.conv2d_grouped(x, w, b, stride, 1, G)
    y.backward(dy)
    # the kernels multiply bf16 operands: the reference gets the same rounded weight
    ry, rdx, rgw, rgb = _reference(x, w.detach().to(torch.bfloat16), b, dy, stride, G)
    for name, got, ref in (("y", y.detach(), ry), ("dx", x.grad, rdx), ("gw", w.grad, rgw), ("gb", b.grad, rgb)):
        rel = float((got.double().cpu() - ref).norm() / ref.norm())
        print(name, rel)
        assert rel < 1e-2, (name, rel)


def test_needs_input_grad_combinations():
    Cg, G, H, W, stride = 16, 4, 9, 13, 1
    x, w, b, dy = _operands(Cg, G, H, W, stride, integer=True)
    ry, rdx, rgw, rgb = _reference(x, w, b, dy, stride, G)
    # frozen weight and bias: only the data gradient
    xa = x.clone().requires_grad_(True)
    torch.ops.mi355.conv2d_grouped(xa, w, b, stride, 1, G).backward(dy)
    assert torch.equal(xa.grad.double().cpu(), rdx) and w.grad is None and b.grad is None
    # input without gradient: weight and bias gradients only
    wa, ba = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    torch.ops.mi355.conv2d_grouped(x, wa, ba, stride, 1, G).backward(dy)
    assert x.grad is None and torch.equal(wa.grad.double().cpu(), rgw) and torch.equal(ba.grad.double().cpu(), rgb)
    # frozen weight, trained bias
    bb = b.clone().requires_grad_(True)
    torch.ops.mi355.conv2d_grouped(x, w, bb, stride, 1, G).backward(dy)
    assert torch.equal(bb.grad.double().cpu(), rgb) and w.grad is None
    # no bias at all
    wb = w.clone().requires_grad_(True)
    y = torch.ops.mi355.conv2d_grouped(x, wb, None, stride, 1, G)
    y.backward(dy)
    assert torch.equal(y.detach().double().cpu(), ry - b.double().cpu().view(1, -1, 1, 1)) and torch.equal(wb.grad.double().cpu(), rgw)


def test_unserved_geometry_is_refused_by_name():
    x = torch.zeros(1, 48, 4, 4, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="Cg 12"):
        torch.ops.mi355.conv2d_grouped(x, torch.zeros(48, 12, 3, 3, device=DEV), None, 1, 1, 4)
    x = torch.zeros(1, 32, 4, 4, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="padding"):
        torch.ops.mi355.conv2d_grouped(x, torch.zeros(32, 16, 3, 3, device=DEV), None, 1, 0, 2)
    with pytest.raises(RuntimeError, match="kernel"):
        torch.ops.mi355.conv2d_grouped(x, torch.zeros(32, 16, 1, 1, device=DEV), None, 1, 1, 2)


def test_cpu_tensor_fails_like_conv2d():
    with pytest.raises(NotImplementedError) as e1:
        torch.ops.mi355.conv2d(torch.zeros(1, 16, 4, 4), torch.zeros(16, 16, 3, 3), None, 1, 1)
    with pytest.raises(NotImplementedError) as e2:
        torch.ops.mi355.conv2d_grouped(torch.zeros(1, 16, 4, 4), torch.zeros(16, 8, 3, 3), None, 1, 1, 2)
    assert "CPU" in str(e1.value) and "CPU" in str(e2.value)


def _net():
    torch.manual_seed(3)
    net = torch.nn.Sequential(
        torch.nn.Conv2d(32, 32, 3, padding=1, bias=False),                       # dense 3x3
        torch.nn.Conv2d(32, 32, 3, stride=2, padding=1, groups=2, bias=True),    # the eligible grouped 3x3 (Cg 16)
        torch.nn.Conv2d(32, 32, 3, padding=1, groups=32, bias=False),            # depthwise 3x3
        torch.nn.Conv2d(32, 32, 3, padding=1, groups=8, bias=False),             # grouped, but Cg 4 is not served
        torch.nn.Conv2d(32, 32, 1, groups=2, bias=False),                        # grouped 1x1: not served
    ).to(DEV)
    return net


def test_patch_grouped_convs():
    net = _net()
    keys = list(net.state_dict().keys())
    before = {i: m.forward for i, m in enumerate(net)}
    assert ops.patch_grouped_convs(net) == 1
    assert list(net.state_dict().keys()) == keys
    for i, m in enumerate(net):
        assert ("forward" in m.__dict__) == (i == 1), i        # only the eligible module got an instance-level forward
        if i != 1:
            assert m.forward == before[i]
    m = net[1]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 32, 9, 13, generator=g).to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(2, 32, 5, 7, generator=g).to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    # one training step of the patched module; the same gradients as the op called directly on copies of the parameters
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    w0, b0 = m.weight.detach().clone().requires_grad_(True), m.bias.detach().clone().requires_grad_(True)
    xa = x.clone().requires_grad_(True)
    ya = m(xa)
    ya.backward(dy)
    xb = x.clone().requires_grad_(True)
    yb = torch.ops.mi355.conv2d_grouped(xb, w0, b0, 2, 1, 2)
    yb.backward(dy)
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    assert torch.equal(m.weight.grad, w0.grad) and torch.equal(m.bias.grad, b0.grad)
    opt.step()
    assert torch.equal(m.weight.detach(), torch.add(w0.detach(), w0.grad, alpha=-0.1)) and torch.equal(m.bias.detach(), torch.add(b0.detach(), b0.grad, alpha=-0.1))
