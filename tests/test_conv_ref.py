"""CPU: tests/conv_ref.py - the float64 reference of the forward / data-gradient convolution that
tests/test_gpu_conv_exact.py compares the kernels with - against float64 torch (conv2d and its autograd) for 1x1, 3x3
stride 1 and 3x3 stride 2 on odd and even maps, and the tap tables the plan builds (PlanBuilder.fwd_taps and the
data-gradient tables of PlanBuilder.dgrad_cmds, the four stride-2 parity classes among them) fed to the descriptor-level
reference against the layer gradient."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
from yolov7_d2_amd import _lib as L
from yolov7_d2_amd.plan import PlanBuilder

LAYERS = [(1, 1, 6, 7), (1, 1, 5, 5), (3, 1, 6, 8), (3, 1, 7, 5), (3, 2, 8, 6), (3, 2, 9, 7), (3, 2, 8, 7), (3, 2, 9, 6)]   # k, stride, H, W
IDS = ["k%ds%d_%dx%d" % c for c in LAYERS]


def _layer(k, stride, H, W, N=2, Cin=5, Cout=7, seed=0):
    g = torch.Generator().manual_seed(seed + 10 * k + stride + H)
    x = torch.randn(N, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, k, k, generator=g, dtype=torch.float64)
    oH, oW = R.conv_out(H, W, k, stride)
    dy = torch.randn(N, oH, oW, Cout, generator=g, dtype=torch.float64)
    return x, w, dy, oH, oW


def _torch_layer(x, w, dy, stride):
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(xn, w, None, stride, w.shape[2] // 2)
    y.backward(dy.permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), xn.grad.permute(0, 2, 3, 1)


def _plan_specs(k, stride, H, W, N=2, Cin=32, Cout=32):
    """the convolution records of a one-layer plan (host only: nothing is materialised)"""
    b = PlanBuilder("cpu", training=True)
    x = b.new_act(N, H, W, Cin, "x")
    w = torch.zeros(Cout, Cin, k, k)
    bn = dict(gamma=torch.ones(Cout), beta=torch.zeros(Cout), rm=torch.zeros(Cout), rv=torch.ones(Cout),
              nbt=torch.zeros((), dtype=torch.long), eps=1e-3, momentum=0.03, ggamma=torch.zeros(Cout), gbeta=torch.zeros(Cout))
    out = b.base_conv("c", x, w, bn, k, stride, torch.zeros_like(w))
    assert b.grad_mode(out) == 0
    b.finalize(materialize=False)
    return {s.tag: s for s in b.conv_records}


@pytest.mark.parametrize("case", LAYERS, ids=IDS)
def test_forward_and_scatter_gradient_equal_torch(case):
    k, stride, H, W = case
    x, w, dy, oH, oW = _layer(*case)
    y_t, dx_t = _torch_layer(x, w, dy, stride)
    torch.testing.assert_close(R.forward_layer(x, w, stride), y_t, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.dgrad_scatter(dy, w, stride, H, W), dx_t, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", LAYERS, ids=IDS)
def test_plan_tap_tables_through_the_descriptor_reference(case):
    """the tables of the plan's own convolution records (forward, data gradient - one launch, or the four parity classes)
    run through conv_reference give the layer's forward / gradient; the unvisited pixels of a class keep their NaN"""
    k, stride, H, W = case
    x, w, dy, oH, oW = _layer(*case)
    y_t, dx_t = _torch_layer(x, w, dy, stride)
    specs = _plan_specs(k, stride, H, W)
    f = specs["c.conv"]
    assert list(f.taps) == PlanBuilder.fwd_taps(k, k // 2) == R.square_taps(k)
    assert (f.outH, f.outW, f.gridH, f.gridW, f.in_stride, f.out_stride) == (oH, oW, oH, oW, stride, 1)
    nan = torch.full((x.shape[0], oH, oW, w.shape[0]), float("nan"), dtype=torch.float64)
    y, _ = R.conv_reference(x, R.fwd_slabs(w), list(f.taps), nan, f.gridH, f.gridW, in_stride=f.in_stride, flags=R.OUT_F32)
    torch.testing.assert_close(y, y_t.float().double(), rtol=1e-6, atol=1e-6)
    dgr = [s for t, s in sorted(specs.items()) if ".dgrad" in t]
    assert len(dgr) == (4 if stride == 2 else 1)
    dx = torch.full((x.shape[0], H, W, w.shape[1]), float("nan"), dtype=torch.float64)
    for i, s in enumerate(dgr):
        assert (s.outH, s.outW, s.in_stride) == (H, W, 1)
        before = dx.clone()
        dx, _ = R.conv_reference(dy, R.dgrad_slabs(w), list(s.taps), dx, s.gridH, s.gridW, out_stride=s.out_stride,
                                 out_oy=s.out_oy, out_ox=s.out_ox, flags=R.OUT_F32)
        written = ~dx.isnan() & before.isnan()
        assert int(written.sum()) == x.shape[0] * s.gridH * s.gridW * w.shape[1]      # disjoint classes, each writes its own grid
        if stride == 2:
            assert (list(s.taps), s.out_oy, s.out_ox, s.gridH, s.gridW) == R.dgrad_s2_classes(H, W)[i]
        else:
            assert list(s.taps) == R.dgrad_taps_s1(k)
    assert not dx.isnan().any()
    torch.testing.assert_close(dx, dx_t.float().double(), rtol=1e-6, atol=1e-6)


def test_epilogues_of_the_descriptor_reference():
    """bias, ReLU, accumulate, add + ReLU, ReLU mask and both kinds of statistics on integer data, against direct formulas"""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-2, 3, (2, 5, 6, 8), generator=g).double()
    w = torch.randint(-1, 2, (4, 8, 3, 3), generator=g).double()
    r = R.forward_layer(x, w, 1)
    old = torch.randint(-9, 10, r.shape, generator=g).double()
    aux = torch.randint(-3, 4, r.shape, generator=g).double()
    bias = torch.randint(-4, 5, (4,), generator=g).double()
    kw = dict(gridH=5, gridW=6)
    run = lambda **k: R.conv_reference(x, R.fwd_slabs(w), R.square_taps(3), old, **kw, **k)
    assert torch.equal(run(bias=bias)[0], r + bias)
    assert torch.equal(run(bias=bias, flags=R.RELU)[0], (r + bias).clamp(min=0))
    assert torch.equal(run(flags=R.ACCUM)[0], r + old)
    assert torch.equal(run(flags=R.ADDRELU, bias=bias, aux=aux)[0], (r + bias + aux).clamp(min=0))
    assert torch.equal(run(flags=R.RELUMASK, aux=aux)[0], r * (aux > 0))
    assert torch.equal(run(flags=R.ACCUM | R.RELUMASK, aux=aux)[0], (r + old) * (aux > 0))
    y, st = run(want_stats=True)
    assert torch.equal(st[:, 0], r.reshape(-1, 4).sum(0)) and torch.equal(st[:, 1], (r * r).reshape(-1, 4).sum(0))
    mean, inv = torch.tensor([1.0, -2.0, 0.0, 3.0], dtype=torch.float64), torch.tensor([0.5, 2.0, 1.0, 0.25], dtype=torch.float64)
    y, st = run(flags=R.BNBWD, bn_y=aux, bn_mean=mean, bn_invstd=inv, want_stats=True)
    assert torch.equal(st[:, 1], (r * (aux - mean) * inv).reshape(-1, 4).sum(0))
    # a sub-grid with an output stride: only the visited pixels change, a bf16 store rounds
    y, _ = R.conv_reference(x, R.fwd_slabs(w) * (1 + 2.0 ** -10), R.square_taps(3), old, 2, 3, out_stride=2, out_oy=1, out_ox=0)
    m = torch.zeros(5, 6, dtype=torch.bool)
    m[1:4:2, 0:5:2] = True
    assert torch.equal(y[:, ~m], old[:, ~m]) and torch.equal(y[:, m], R.bf16_round(r[:, :2, :3] * (1 + 2.0 ** -10)).reshape(2, 6, 4))
    with pytest.raises(AssertionError):
        R.assert_exact(torch.tensor([257.0]))
    with pytest.raises(AssertionError):
        R.assert_exact(torch.tensor([0.5]))
    R.assert_exact(torch.tensor([256.0, float("nan"), -3.0]))


def test_packed_image_layout():
    """wf[tap][ci / 8][co][ci % 8] and wd[tap][co / 8][ci][co % 8] with zero pads (include/mi355_det.h:245-246)"""
    w = torch.arange(3 * 10 * 9, dtype=torch.float64).reshape(3, 10, 3, 3) + 1
    wf = R.packed_image(R.fwd_slabs(w), 2, 32)
    wd = R.packed_image(R.dgrad_slabs(w), 1, 32)
    assert wf.shape == (9, 2, 32, 8) and wd.shape == (9, 1, 32, 8)
    for (co, ci, r, s) in ((0, 0, 0, 0), (2, 9, 2, 1), (1, 7, 1, 1)):
        assert wf[r * 3 + s, ci // 8, co, ci % 8] == w[co, ci, r, s] == wd[r * 3 + s, co // 8, ci, co % 8]
    assert wf[:, :, 3:].abs().sum() == 0 and wf[:, 1, :, 2:].abs().sum() == 0 and wd[:, :, 10:].abs().sum() == 0 and wd[..., 3:].abs().sum() == 0
    assert L.MI_MAX_TAPS >= 9
