"""GPU (-m gpu): the deformable 3x3 convolution - csrc/deform_conv.hip (mi_deform_im2col / _col2im / _absmax / _zero_f32 / _dx_finish),
the GEMMs it hands to the convolution kernels, modeling/resnet.py's DeformConv / DeformBottleneckBlock and the SparseInst
step on a DCN backbone - against the float64 restatement of tests/deform_conv_ref.py.

Exact cases (no tolerance, the method of tests/test_gpu_conv_exact.py): x, the weights and dy hold small integers and the
offsets are multiples of 0.25, so every interpolation weight is a multiple of 1/16, every sampled value, product and fp32
partial sum is an exact multiple of 1/16 (1/4 for the coordinate gradients) whatever the order - the float atomics of
mi_deform_col2im included - and every bf16 store holds a value bf16 represents.  Those conditions are asserted on the
reference of every case before anything is launched.  Every output sits between guard words that must survive, and is
pre-filled with NaN.

Random-offset cases, the block and the SparseInst steps use the bounds of test_gpu_resnet.py::test_bottleneck_block_fwd_bwd
(output < 1e-2, gradients < 3e-2, norm-relative) and of test_sparseinst_vd_captured_step_equals_eager_across_two_shapes."""
import copy
import ctypes as C
import functools
import os

import pytest
import torch

import deform_conv_ref as R
import yolov7_d2_amd as M
from yolov7_d2_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -1536.0          # sentinel (exact in bf16, fp32 and fp64)
GUARD = 64              # guard elements on either side of every output
N, COUT = 2, 32
F32_EXACT = float(1 << 24)


def _rel(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).norm() / (b.detach().double().cpu().norm() + 1e-12))


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


# ------------------------------------------------------------------------------------------------------- exact cases (CPU part)
def _sparse(g, shape, p, vals):
    v = torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), shape, generator=g)]
    return v * (torch.rand(shape, generator=g) < p)


@functools.lru_cache(maxsize=None)
def exact_case(Cc, H, W, stride):
    """operands and the float64 reference of one exact case, with the conditions of the method asserted (CPU only)"""
    g = torch.Generator().manual_seed(1000 + 7 * Cc + 13 * H + 17 * W + stride)
    Ho, Wo = R.out_size(H, W, stride)
    x = _sparse(g, (N, Cc, H, W), 0.25, (-2, -1, 1, 2))
    w = _sparse(g, (COUT, Cc, 3, 3), 0.06, (-1, 1))
    scale = torch.tensor([1.0, 2.0], dtype=torch.float64)[torch.arange(COUT) % 2]
    shift = torch.randint(-2, 3, (COUT,), generator=g).double()
    dy = _sparse(g, (N, COUT, Ho, Wo), 0.1, (-1, 1))
    off = torch.randint(-10, 11, (N, 18, Ho, Wo), generator=g).double() * 0.25
    hb, wb = (Ho - 1) * stride + 1, (Wo - 1) * stride + 1          # base coordinate of the last row's / column's third tap
    forced = [  # (n, ho, wo, tap, row offset, column offset)
        (0, 0, 1, 0, 0.0, 0.25),                  # h exactly -1
        (0, 0, 2, 0, 0.5, 0.0),                   # h in (-1, 0)
        (0, 0, 3, 1, -0.75, 0.5),                 # h = -1.75: just outside
        (0, Ho - 1, 1, 7, H - hb, 0.0),           # h exactly H
        (0, Ho - 1, 2, 7, H - hb - 0.5, 0.25),    # h in (H - 1, H)
        (1, 1, 0, 3, 0.5, 0.0),                   # w exactly -1
        (1, 2, 0, 3, 0.0, 0.75),                  # w in (-1, 0)
        (1, 1, Wo - 1, 5, 0.25, W - wb),          # w exactly W
        (1, 2, Wo - 1, 5, 0.0, W - wb - 0.25),    # w in (W - 1, W)
        (1, 0, 0, 4, -12.0, 0.0), (1, 0, 1, 4, 0.0, 20.0), (0, 1, 1, 8, 9.5, -11.25),      # far outside
        (0, 1, 2, 4, 0.0, 0.0),                   # an interior integer point: three corners with zero weight
        (0, 2, 1, 4, 0.75, -0.25), (1, 2, 2, 0, 1.25, 1.5),                              # interior, all four corners
    ]
    for n, ho, wo, t, a, b in forced:
        off[n, 2 * t, ho, wo], off[n, 2 * t + 1, ho, wo] = a, b
    assert torch.equal(_bf(off), off)
    h, ww = R.sample_points(off, H, W, stride)
    for v, S in ((h, H), (ww, W)):                # the classes the issue names, in both directions
        assert bool((v == -1).any()) and bool((v == S).any()) and bool(((v > -1) & (v < 0)).any()) and bool(((v > S - 1) & (v < S)).any())
        assert bool((v < -3).any()) and bool((v > S + 2).any()) and bool(((v > 0) & (v < S - 1) & (v != v.floor())).any())
    xr, offr, wr = x.clone().requires_grad_(True), off.clone().requires_grad_(True), w.clone().requires_grad_(True)
    col = R.deform_cols(xr, offr, stride)
    col.retain_grad()
    wf = R.tap_major(wr * scale.view(-1, 1, 1, 1))
    y = torch.einsum("nhwtc,otc->nohw", col, wf) + shift.view(1, -1, 1, 1)
    (y * dy).sum().backward()
    ref = dict(col=col.detach(), y=y.detach(), dcol=col.grad, dx=xr.grad, doff=offr.grad, gw=wr.grad)
    # the same with the ReLU in the epilogue and the input's ReLU mask on dx (the autograd node)
    xr2, offr2, wr2 = x.clone().requires_grad_(True), off.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y2 = torch.relu(torch.einsum("nhwtc,otc->nohw", R.deform_cols(xr2, offr2, stride), R.tap_major(wr2 * scale.view(-1, 1, 1, 1))) +
                    shift.view(1, -1, 1, 1))
    (y2 * dy).sum().backward()
    ref2 = dict(y=y2.detach(), dx=xr2.grad, dx_masked=xr2.grad * (x > 0), doff=offr2.grad, gw=wr2.grad)
    # ---- the conditions of the method
    for name, r in (("1", ref), ("2", ref2)):
        for k, v in r.items():
            if k == "gw":
                assert torch.equal(v.float().double(), v), (name, k)
            else:
                assert torch.equal(_bf(v), v), (name, k, float(v.abs().max()))       # what a bf16 store keeps is the value itself
            q = 4.0 if k == "doff" else 16.0
            assert torch.equal((v * q).round(), v * q), (name, k)
    K = 9 * Cc
    colmax, wmax, dymax = float(ref["col"].abs().max()), float((w * scale.view(-1, 1, 1, 1)).abs().max()), float(dy.abs().max())
    dcolmax, xmax = float(ref["dcol"].abs().max()), float(x.abs().max())
    assert 16 * (colmax * wmax * K + float(shift.abs().max())) < F32_EXACT               # y: any order of the k-chunks
    assert 16 * dymax * wmax * COUT < F32_EXACT                                            # dcol
    assert 16 * colmax * dymax * N * Ho * Wo * float(scale.max()) < F32_EXACT              # gW (and its scaling by a power of two)
    assert 16 * dcolmax * N * Ho * Wo * 9 * 4 < F32_EXACT                                  # dx: every atomic add into one element
    assert 4 * dcolmax * 4 * xmax * Cc < F32_EXACT                                         # d_offset: the sum over C
    return dict(x=x, w=w, scale=scale, shift=shift, dy=dy, off=off, ref=ref, ref2=ref2, Ho=Ho, Wo=Wo)


# ------------------------------------------------------------------------------------------------------- device helpers
class Guarded:
    """an output of `shape` (NaN) between GUARD sentinel elements; `lo` / `hi`: extra sentinel channels beside the last
    dimension's view that must survive too"""

    def __init__(self, shape, dtype, hi=0):
        self.shape, self.hi = tuple(shape), hi
        full = self.shape[:-1] + (self.shape[-1] + hi,)
        n = 1
        for s in full:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
        self.all = self.buf[GUARD:GUARD + n].view(full)
        self.view = self.all[..., :self.shape[-1]]
        self.view.fill_(float("nan"))
        self.ld = full[-1]

    def dense(self):
        assert self.hi == 0
        return self.all

    def intact(self):
        ok = bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[-GUARD:] == SENT).all())
        return ok and (self.hi == 0 or bool((self.all[..., self.shape[-1]:] == SENT).all()))


def _same(got, exp, what):
    """bit-for-bit (after the store's rounding, which the reference survives unchanged)"""
    exp = exp.to(got.dtype).to(got.device)
    if not torch.equal(got, exp):
        ne = ~((got == exp) | (got.isnan() & exp.isnan()))
        first = tuple(torch.nonzero(ne)[0].tolist())
        raise AssertionError("%s: %d of %d elements differ (%d NaN), first at %s: got %r, expected %r" % (
            what, int(ne.sum()), ne.numel(), int(got.isnan().sum()), first, float(got[first]), float(exp[first])))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _wgrad_into(g, xh, dyh, scale, gw):
    """ops._ConvGeom.wgrad with the gradient written into the caller's (guarded) buffer"""
    from yolov7_d2_amd.ops import _ld
    d = L.mi_wgrad_desc()
    d.x, d.dy, d.gw = xh.data_ptr(), dyh.data_ptr(), gw.data_ptr()
    d.row_scale = scale.data_ptr()
    d.ldx, d.ldy, d.N, d.H, d.W, d.outH, d.outW, d.stride = _ld(xh), _ld(dyh), g.N, g.H, g.W, g.Ho, g.Wo, g.s
    d.Cin, d.Cout, d.CinPad, d.CoutPad, d.ntaps = g.Cin, g.Cout, g.CinP, g.CoutP, 1
    need = L.lib().mi_conv2d_wgrad_plan(C.byref(d))
    L.check(need, "mi_conv2d_wgrad_plan")
    ws = torch.empty(max(int(need), 16), dtype=torch.uint8, device=DEV)
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
    L.check(L.lib().mi_conv2d_wgrad(C.byref(d), L.stream_ptr()), "mi_conv2d_wgrad")
    return ws


EXACT = [(Cc, H, W, s) for Cc in (32, 96) for (H, W) in ((7, 9), (8, 8)) for s in (1, 2)]


@pytest.mark.parametrize("Cc,H,W,stride", EXACT)
def test_exact_through_the_c_abi(Cc, H, W, stride):
    """columns, output, dcol, d_offset (padding channels zero), the fp32 dx sum, dx with and without the ReLU mask, and gW -
    each launch on its own guarded buffer.  x lies in a buffer 32 channels wider (NaN beside it), the offsets in rows of 32
    whose 14 padding channels are NaN: neither may be read."""
    from yolov7_d2_amd.modeling.resnet import _deform_geom, _tap_major
    c = exact_case(Cc, H, W, stride)
    ref, Ho, Wo = c["ref"], c["Ho"], c["Wo"]
    lib, sp = L.lib(), L.stream_ptr()
    xb = torch.full((N, H, W, Cc + 32), float("nan"), dtype=torch.bfloat16, device=DEV)
    xb[..., :Cc] = _nhwc(c["x"]).to(DEV, torch.bfloat16)
    offb = torch.full((N, Ho, Wo, 32), float("nan"), dtype=torch.bfloat16, device=DEV)
    offb[..., :18] = _nhwc(c["off"]).to(DEV, torch.bfloat16)
    # ---- forward: sampled im2col, then the 1x1 route
    col = Guarded((N, Ho, Wo, 9 * Cc), torch.bfloat16)
    L.check(lib.mi_deform_im2col(xb.data_ptr(), Cc + 32, offb.data_ptr(), 32, col.view.data_ptr(), N, H, W, Cc, stride, 1, 1, sp), "im2col")
    torch.cuda.synchronize()
    _same(col.dense(), ref["col"].reshape(N, Ho, Wo, 9 * Cc), "col")
    assert col.intact()
    g = _deform_geom((N, Cc, H, W), (COUT, Cc, 3, 3), stride)
    assert (g.Cin, g.k, g.Ho, g.Wo) == (9 * Cc, 1, Ho, Wo)
    wd32, scale, shift = c["w"].float().to(DEV), c["scale"].float().to(DEV), c["shift"].float().to(DEV)
    wf, wd = g.pack(_tap_major(wd32), dgrad=True, scale=scale)
    y = Guarded((N, Ho, Wo, COUT), torch.bfloat16)
    g.fwd(col.dense(), wf, y.dense(), bias=shift)
    torch.cuda.synchronize()
    _same(y.dense(), _nhwc(ref["y"]), "y")
    assert y.intact()
    # ---- backward: dcol, gW, col2im, the pass to bf16
    dyh = _nhwc(c["dy"]).to(DEV, torch.bfloat16)
    dcol = Guarded((N, Ho, Wo, 9 * Cc), torch.bfloat16)
    g.dgrad(dyh, wd, dcol.dense())
    torch.cuda.synchronize()
    _same(dcol.dense(), ref["dcol"].reshape(N, Ho, Wo, 9 * Cc), "dcol")
    assert dcol.intact()
    gw = Guarded((COUT, 9 * Cc), torch.float32)
    keep = _wgrad_into(g, col.dense(), dyh, scale, gw.view)
    torch.cuda.synchronize()
    _same(gw.dense().view(COUT, 3, 3, Cc).permute(0, 3, 1, 2), ref["gw"], "gW")
    assert gw.intact()
    del keep
    gmax = Guarded((4,), torch.float32)
    L.check(lib.mi_deform_zero_f32(gmax.view.data_ptr(), 4, sp), "zero")
    L.check(lib.mi_deform_absmax(dcol.view.data_ptr(), dcol.view.numel(), gmax.view.data_ptr(), sp), "absmax")
    torch.cuda.synchronize()
    assert gmax.intact() and gmax.dense().tolist() == [float(ref["dcol"].abs().max()), 0.0, 0.0, 0.0]
    exp_off = torch.zeros(N, Ho, Wo, 32, dtype=torch.float64)
    exp_off[..., :18] = _nhwc(ref["doff"])
    # plain adds, and adds on the grid of max |dcol| (2^(e - 16) <= 1/16 here: every addend of the case lies on it)
    assert float(ref["dcol"].abs().max()) <= 4096
    for grid in (None, gmax.view.data_ptr()):
        dx32 = Guarded((N, H, W, Cc), torch.float32)
        doff = Guarded((N, Ho, Wo, 32), torch.bfloat16)
        L.check(lib.mi_deform_zero_f32(dx32.view.data_ptr(), dx32.view.numel(), sp), "zero")
        torch.cuda.synchronize()
        assert dx32.intact() and float(dx32.dense().abs().max()) == 0
        L.check(lib.mi_deform_col2im(dcol.view.data_ptr(), xb.data_ptr(), Cc + 32, offb.data_ptr(), 32, dx32.view.data_ptr(),
                                     doff.view.data_ptr(), grid, N, H, W, Cc, stride, 1, 1, sp), "col2im")
        torch.cuda.synchronize()
        _same(dx32.dense(), _nhwc(ref["dx"]), "dx32")
        _same(doff.dense(), exp_off, "d_offset (18 live channels, 14 zero)")
        assert dx32.intact() and doff.intact() and gmax.intact()
    for mask in (False, True):
        dx = Guarded((N, H, W, Cc), torch.bfloat16, hi=8)
        L.check(lib.mi_deform_dx_finish(dx32.view.data_ptr(), xb.data_ptr() if mask else None, Cc + 32 if mask else 0,
                                        dx.view.data_ptr(), dx.ld, N * H * W, Cc, sp), "dx_finish")
        torch.cuda.synchronize()
        exp = _nhwc(ref["dx"] * (c["x"] > 0) if mask else ref["dx"])
        _same(dx.view, exp, "dx (mask %s)" % mask)
        assert dx.intact()


@pytest.mark.parametrize("keep_col", ["1", "0"])
@pytest.mark.parametrize("Cc,H,W,stride", EXACT[1::3])
def test_exact_through_the_autograd_node(Cc, H, W, stride, keep_col, monkeypatch):
    """DeformConv's node (ReLU in the epilogue, the input's ReLU mask on dx), columns kept and re-sampled; the offsets are read
    in place from rows of 32 (their gradient comes back into such rows), and once from a plain fp32 NCHW tensor"""
    from yolov7_d2_amd.modeling.resnet import _DeformConvFn, _offset_operand
    monkeypatch.setenv("MI_DEFORM_KEEP_COL", keep_col)
    c = exact_case(Cc, H, W, stride)
    ref, Ho, Wo = c["ref2"], c["Ho"], c["Wo"]
    scale, shift = c["scale"].float().to(DEV), c["shift"].float().to(DEV)
    dy = c["dy"].to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    for in_place in (True, False):
        x = c["x"].to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w = c["w"].float().to(DEV).requires_grad_(True)
        if in_place:
            rows = torch.full((N, Ho, Wo, 32), float("nan"), dtype=torch.bfloat16, device=DEV)
            rows[..., :18] = _nhwc(c["off"]).to(DEV, torch.bfloat16)
            rows.requires_grad_(True)
            offset = rows.permute(0, 3, 1, 2)[:, :18]
            assert _offset_operand(offset, N, Ho, Wo)[0] is offset
        else:
            rows = None
            offset = c["off"].float().to(DEV).requires_grad_(True)
        y = _DeformConvFn.apply(x, offset, w, scale, shift, stride, True, True)
        y.backward(dy)
        torch.cuda.synchronize()
        _same(y.detach(), ref["y"], "y")
        _same(x.grad, ref["dx_masked"], "dx")
        _same(w.grad, ref["gw"], "gW")
        if in_place:
            _same(rows.grad[..., :18], _nhwc(ref["doff"]), "d_offset")
            assert float(rows.grad[..., 18:].abs().max()) == 0
        else:
            _same(offset.grad, ref["doff"], "d_offset")


# ------------------------------------------------------------------------------------------------------- random offsets
def _norm_state(g, co):
    return {"weight": 0.5 + torch.rand(co, generator=g), "bias": torch.randn(co, generator=g) * 0.1,
            "running_mean": torch.randn(co, generator=g) * 0.1, "running_var": 0.5 + torch.rand(co, generator=g)}


def _affine(ns):
    scale = ns["weight"].double() * (ns["running_var"].double() + 1e-5).rsqrt()
    return scale, ns["bias"].double() - ns["running_mean"].double() * scale


@pytest.mark.parametrize("Cc,Cout,H,W,stride", [(96, 64, 15, 17, 1), (96, 64, 15, 17, 2), (256, 128, 8, 8, 1)])
def test_random_offsets_against_the_restatement(Cc, Cout, H, W, stride):
    """offsets ~ N(0, 1.5): output, dx, d_offset and gW against the float64 restatement with the device's bf16 stores"""
    from yolov7_d2_amd.modeling.resnet import DeformConv
    g = torch.Generator().manual_seed(11 + Cc + stride)
    Ho, Wo = R.out_size(H, W, stride)
    m = DeformConv(Cc, Cout, stride)
    ns = _norm_state(g, Cout)
    w = _bf(torch.randn(Cout, Cc, 3, 3, generator=g) * (2.0 / (9 * Cc)) ** 0.5)
    m.load_state_dict({"weight": w, **{"norm." + k: v for k, v in ns.items()}})
    m.to(DEV)
    x = _bf(torch.randn(N, Cc, H, W, generator=g))
    off = _bf(torch.randn(N, 18, Ho, Wo, generator=g) * 1.5)
    go = _bf(torch.randn(N, Cout, Ho, Wo, generator=g))
    xr, offr, wr = (t.double().requires_grad_(True) for t in (x, off, w))
    scale, shift = _affine(ns)
    ref = R.deform_conv(xr, offr, wr, stride, scale, shift, relu=True, device_rounding=True)
    ref.backward(go.double())
    xd = x.to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    od = off.to(DEV, torch.bfloat16).requires_grad_(True)
    out = m(xd, od, relu=True)
    out.backward(go.to(DEV, torch.bfloat16))
    errs = dict(out=_rel(out, ref), dx=_rel(xd.grad, xr.grad), d_offset=_rel(od.grad, offr.grad), gW=_rel(m.weight.grad, wr.grad))
    print("deform conv, random offsets", (Cc, Cout, H, W, stride), {k: round(v, 5) for k, v in errs.items()})
    assert errs["out"] < 1e-2, errs
    assert errs["dx"] < 3e-2 and errs["d_offset"] < 3e-2 and errs["gW"] < 3e-2, errs
    # the no-autograd path (evaluation, a frozen stage) computes the same output
    with torch.no_grad():
        assert torch.equal(m(xd, od, relu=True), out.detach())
    m.weight.requires_grad_(False)
    with torch.no_grad():
        assert torch.equal(m(xd.detach(), od.detach(), relu=True), out.detach())


def test_col2im_sums_on_the_grid_are_bit_reproducible_and_close():
    """random operands, small maps (many adds per element): with the grid of max |dcol| the fp32 dx sum has the same bits in
    every run - the float atomics arrive in whatever order - and differs from the float64 sum of the unrounded addends by at
    most (adds per element) * max |dcol| * 2^-16 (the grid's half step per addend) plus the fp32 rounding of the sum"""
    lib, sp = L.lib(), L.stream_ptr()
    g = torch.Generator().manual_seed(77)
    Cc, H, W, stride = 96, 5, 6, 1
    x = _bf(torch.randn(N, Cc, H, W, generator=g)).double()
    off = _bf(torch.randn(N, 18, H, W, generator=g) * 1.5).double()
    dcol = _bf(torch.randn(N, H, W, 9, Cc, generator=g) * torch.rand(N, H, W, 9, 1, generator=g) * 8).double()
    xr = x.clone().requires_grad_(True)
    (R.deform_cols(xr, off, stride) * dcol).sum().backward()
    xb = _nhwc(x).to(DEV, torch.bfloat16)
    offb = torch.zeros(N, H, W, 32, dtype=torch.bfloat16, device=DEV)
    offb[..., :18] = _nhwc(off).to(DEV, torch.bfloat16)
    dc = dcol.reshape(N, H, W, 9 * Cc).to(DEV, torch.bfloat16)
    buf = torch.empty(N * H * W * Cc + 4, device=DEV)
    doff = torch.empty(N, H, W, 32, dtype=torch.bfloat16, device=DEV)
    runs = []
    for _ in range(6):
        L.check(lib.mi_deform_zero_f32(buf.data_ptr(), buf.numel(), sp), "zero")
        L.check(lib.mi_deform_absmax(dc.data_ptr(), dc.numel(), buf[-4:].data_ptr(), sp), "absmax")
        L.check(lib.mi_deform_col2im(dc.data_ptr(), xb.data_ptr(), Cc, offb.data_ptr(), 32, buf.data_ptr(), doff.data_ptr(),
                                     buf[-4:].data_ptr(), N, H, W, Cc, stride, 1, 1, sp), "col2im")
        torch.cuda.synchronize()
        runs.append(buf[:-4].clone())
    assert all(torch.equal(r, runs[0]) for r in runs[1:])
    m = float(dcol.abs().max())
    assert float(buf[-4]) == m
    got = runs[0].view(N, H, W, Cc).permute(0, 3, 1, 2).double().cpu()
    nadds = 9 * 4 * H * W                                              # (every corner of every tap of every pixel of the image)
    err = float((got - xr.grad).abs().max())
    print("col2im on the grid: max |dx32 - float64 sum| %.3e, max |dx| %.3e, max |dcol| %.3e" % (err, float(xr.grad.abs().max()), m))
    assert err <= nadds * m * 2.0 ** -16 + float(xr.grad.abs().max()) * 2.0 ** -20


# ------------------------------------------------------------------------------------------------------- the block
def _block_state(g, blk, offset_std):
    sd = {}
    for n in ("shortcut", "conv1", "conv2", "conv3"):
        mod = getattr(blk, n)
        if mod is None:
            continue
        co, ci, k, _ = mod.weight.shape
        sd[n + ".weight"] = _bf(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
        sd.update({n + ".norm." + k_: v for k_, v in _norm_state(g, co).items()})
    bc = blk.conv2_offset.weight.shape[1]
    sd["conv2_offset.weight"] = _bf(torch.randn(18, bc, 3, 3, generator=g) * offset_std / (9 * bc) ** 0.5)
    sd["conv2_offset.bias"] = torch.randn(18, generator=g) * offset_std * 0.25
    return sd


def _ref_params(sd, has_sc):
    p = {k: v.double().requires_grad_(True) for k, v in sd.items() if ".norm." not in k}
    aff = {n: _affine({k: sd[n + ".norm." + k] for k in ("weight", "bias", "running_mean", "running_var")})
           for n in ("conv1", "conv2", "conv3") + (("shortcut",) if has_sc else ())}
    tree = {n: (p[n + ".weight"],) + aff[n] for n in aff}
    tree["conv2_offset"] = (p["conv2_offset.weight"], p["conv2_offset.bias"])
    if not has_sc:
        tree["shortcut"] = None
    return p, tree


@pytest.mark.parametrize("cin,cout,bc,stride,H,W", [(256, 512, 128, 2, 15, 17), (512, 512, 128, 1, 8, 8)])
def test_deform_bottleneck_block_fwd_bwd(cin, cout, bc, stride, H, W):
    """DeformBottleneckBlock with random conv2_offset weights (offsets of order 1) against the restated block: output, input
    gradient and every parameter gradient - conv2_offset's weight and bias included"""
    from yolov7_d2_amd.modeling.resnet import DeformBottleneckBlock
    g = torch.Generator().manual_seed(21 + stride)
    blk = DeformBottleneckBlock(cin, cout, bc, stride=stride)
    sd = _block_state(g, blk, offset_std=1.0)
    blk.load_state_dict(sd)
    blk.to(DEV)
    x = _bf(torch.randn(N, cin, H, W, generator=g)).relu()
    p, tree = _ref_params(sd, blk.shortcut is not None)
    xr = x.double().requires_grad_(True)
    ref = R.deform_block(xr, tree, stride)
    go = _bf(torch.randn(ref.shape, generator=g))
    ref.backward(go.double())
    xd = x.to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = blk(xd)
    out.backward(go.to(DEV, torch.bfloat16))
    errs = {"out": _rel(out, ref), "x": _rel(xd.grad, xr.grad)}
    errs.update({n: _rel(q.grad, p[n].grad) for n, q in blk.named_parameters()})
    print("deform block", (cin, cout, bc, stride, H, W), {k: round(v, 5) for k, v in errs.items()})
    assert errs.pop("out") < 1e-2, errs
    assert all(v < 3e-2 for v in errs.values()), errs


def test_zero_offsets_equal_the_plain_bottleneck_block():
    """conv2_offset at its zero initialisation: the block is a BottleneckBlock carrying the same weights - and conv2_offset
    still receives a gradient it can leave zero with"""
    from yolov7_d2_amd.modeling.resnet import BottleneckBlock, DeformBottleneckBlock
    g = torch.Generator().manual_seed(31)
    cin, cout, bc, stride, H, W = 256, 512, 128, 2, 15, 17
    dblk, blk = DeformBottleneckBlock(cin, cout, bc, stride=stride), BottleneckBlock(cin, cout, bc, stride=stride)
    sd = _block_state(g, dblk, offset_std=0.0)
    assert float(sd["conv2_offset.weight"].abs().max()) == 0 and float(sd["conv2_offset.bias"].abs().max()) == 0
    dblk.load_state_dict(sd)
    blk.load_state_dict({k: v for k, v in sd.items() if "conv2_offset" not in k})
    dblk.to(DEV), blk.to(DEV)
    x = _bf(torch.randn(N, cin, H, W, generator=g)).relu().to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    go = _bf(torch.randn(N, cout, 8, 9, generator=g)).to(DEV, torch.bfloat16)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    oa, ob = dblk(xa), blk(xb)
    oa.backward(go)
    ob.backward(go)
    errs = {"out": _rel(oa, ob), "x": _rel(xa.grad, xb.grad)}
    errs.update({n: _rel(dict(dblk.named_parameters())[n].grad, q.grad) for n, q in blk.named_parameters()})
    print("deform block, zero offsets vs BottleneckBlock", {k: round(v, 6) for k, v in errs.items()})
    assert errs.pop("out") < 1e-2, errs
    assert all(v < 3e-2 for v in errs.values()), errs
    for t in (dblk.conv2_offset.weight.grad, dblk.conv2_offset.bias.grad):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------- SparseInst on a DCN backbone
def _dcn_model():
    torch.manual_seed(0)
    cfg = M.sparse_inst_r50_giam_cfg(device=DEV)
    cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = [False, False, True, True]
    model = M.build_model(cfg)
    n = 0
    with torch.no_grad():          # random small conv2_offset weights, so that the offsets do something
        for blk in (b for st in model.backbone.stage_modules() for b in st):
            if hasattr(blk, "conv2_offset"):
                blk.conv2_offset.weight.normal_(0, 0.01)
                blk.conv2_offset.bias.normal_(0, 0.1)
                n += 1
    assert n == 9
    return model.train()


def test_sparseinst_dcn_eager_step_trains_every_backbone_parameter():
    from test_gpu_resnetvd import _si_inputs
    model = _dcn_model()
    losses = model(_si_inputs(1, ((192, 224), (160, 200))))
    assert losses and all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
    sum(losses.values()).backward()
    params = dict(model.backbone.named_parameters())
    assert len(params) == 1 + 16 * 3 + 4 + 9 * 2
    bad = [n for n, p in params.items() if p.grad is None or not bool(torch.isfinite(p.grad).all()) or float(p.grad.abs().max()) == 0]
    assert not bad, bad


def test_sparseinst_dcn_captured_step_equals_eager_across_two_shapes():
    """the sequence of test_sparseinst_vd_captured_step_equals_eager_across_two_shapes on the DCN backbone: capture at one
    padded shape, an eager forward, a capture at a second shape, then replays of both - every step's losses equal the eager
    model's"""
    from test_gpu_resnetvd import _si_inputs
    from yolov7_d2_amd.graph_step import GraphedTrainStep
    from yolov7_d2_amd.optim import MultiTensorAdamW
    eager = _dcn_model()
    graphed = copy.deepcopy(eager)
    mk = lambda m: MultiTensorAdamW([p for p in m.parameters() if p.requires_grad], lr=5e-5, weight_decay=0.05)
    oe, og = mk(eager), mk(graphed)
    a1, a2 = _si_inputs(1, ((192, 224), (160, 200))), _si_inputs(3, ((170, 224), (192, 200)))
    b1, b2 = _si_inputs(2, ((128, 160), (120, 150)), counts=(3, 1)), _si_inputs(4, ((100, 160), (128, 140)), counts=(2, 0))
    assert eager.batch_key(a1) == eager.batch_key(a2) != eager.batch_key(b1) == eager.batch_key(b2)
    step = GraphedTrainStep(graphed, og)
    try:
        for it, b in enumerate((a1, b1, a2, b2)):
            if it == 1:
                with torch.no_grad():
                    graphed(a2)                       # an eager forward between the two captures
            losses = eager(b)
            oe.zero_grad(set_to_none=True)
            sum(losses.values()).backward()
            oe.step()
            out = step(b)
            assert len(step.graphs) == min(it + 1, 2)
            for k, v in losses.items():
                print("captured vs eager, step", it, k, float(out[k]), float(v), "diff %.3e" % abs(float(out[k]) - float(v)))
            for k, v in losses.items():
                torch.testing.assert_close(out[k].float(), v.detach().float(), rtol=3e-3, atol=3e-3, msg=f"step {it} {k}")
        torch.cuda.synchronize()
    finally:
        step.close()
