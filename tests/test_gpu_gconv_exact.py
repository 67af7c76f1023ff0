"""GPU (-m gpu): the grouped 3x3 convolution kernels (csrc/conv_grouped.hip) - forward, data gradient, weight gradient and
mi_gconv_pack_weight - against the plain float64 reference of tests/gconv_ref.py with NO tolerance, through the C ABI.

The method (tests/gconv_ref.py): the bf16 operands hold small integers, so every product and every fp32 partial sum is an
exact integer whatever the order of taps, octets, tiles or splits, and any correct kernel equals the reference BIT FOR BIT.
The conditions are asserted on the float64 reference of every case when it is built (Case), before anything is launched;
test_premise_holds_for_every_case builds all of them on the CPU (no GPU needed): no case is ever skipped for failing them.

Hygiene of every launch: an input view sits in a NaN buffer (guards, the channels beyond C, the neighbouring slice) that must
not reach the result; an output view is pre-filled with NaN inside a buffer of sentinel words (guards, the channels beyond C,
the neighbouring channels of a slice) that must survive bit for bit."""
import ctypes as C
import functools

import pytest
import torch

import gconv_ref as R
from yolov7_d2_amd import _lib as L

DEV = "cuda"
SENT = -1536.0      # exact in bf16 and fp32
GUARD = 64
NAN = float("nan")

# (Cg, G, row stride): the table of the group widths; C = G * Cg
GROUPS = [(8, 3, 32), (16, 10, 160), (24, 3, 96), (32, 2, 64), (16, 1, 16)]
# (H, W, stride), N = 2: 1x1 - every tap but the centre is padding; 9x13 - odd, ragged against any tile; 16x16; stride 2
MAPS = [(1, 1, 1), (9, 13, 1), (16, 16, 1), (8, 12, 2), (9, 13, 2)]
N = 2
# "table": the view starts at channel 0 of rows of the table's stride; "slice": a channel slice at offset 8 of a map 16 wider
VARIANTS = ["table", "slice"]
SPLIT = (16, 10, 160, 40, 40, 1)        # the split-K weight gradient: Cg, G, row stride, H, W, stride


class Case:
    """integer operands and the float64 reference of one (group shape, map); the premise is asserted here"""

    def __init__(self, Cg, G, H, W, stride):
        self.Cg, self.G, self.C, self.H, self.W, self.stride = Cg, G, Cg * G, H, W, stride
        self.Ho, self.Wo = R.out_size(H, W, stride)
        g = torch.Generator().manual_seed(1000 * Cg + 100 * G + 10 * H + W + stride)
        Cc = self.C
        self.x = torch.randint(-2, 3, (N, H, W, Cc), generator=g).double()
        self.dy = torch.randint(-2, 3, (N, self.Ho, self.Wo, Cc), generator=g).double()
        self.w = torch.randint(-1, 2, (Cc, Cg, 3, 3), generator=g).double()
        self.bias = torch.randint(-3, 4, (Cc,), generator=g).double()
        for t in (self.x, self.dy, self.w):         # bf16 operands: integers of magnitude <= 256
            assert bool((t == t.round()).all()) and float(t.abs().max()) <= R.BF16_INT_MAX
        ax, ady, aw, ab = self.x.abs(), self.dy.abs(), self.w.abs(), self.bias.abs()
        self.y = R.forward(self.x, self.w, G, stride)
        self.yb = R.forward(self.x, self.w, G, stride, self.bias)
        R.assert_exact(self.y, R.forward(ax, aw, G, stride), bf16=True)
        R.assert_exact(self.yb, R.forward(ax, aw, G, stride, ab), bf16=True)
        self.dx = R.dgrad(self.dy, self.w, G, stride, H, W)
        R.assert_exact(self.dx, R.dgrad(ady, aw, G, stride, H, W), bf16=True)
        self.gw, self.gb = R.wgrad(self.x, self.dy, G, stride)
        agw, agb = R.wgrad(ax, ady, G, stride)
        R.assert_exact(self.gw, agw, bf16=False)
        R.assert_exact(self.gb, agb, bf16=False)
        self.wf, self.wd = R.packed_images(self.w, Cg)


@functools.lru_cache(maxsize=None)
def case(Cg, G, H, W, stride):
    return Case(Cg, G, H, W, stride)


def all_cases():
    return [(Cg, G, H, W, s) for (Cg, G, _) in GROUPS for (H, W, s) in MAPS] + [SPLIT[:2] + SPLIT[3:]]


def test_premise_holds_for_every_case():
    """CPU: 100 % of the cases satisfy the exact-integer conditions on the reference alone"""
    for k in all_cases():
        case(*k)


# ------------------------------------------------------------------------------------------------------------- buffers
def layout(variant, C_, ld):
    """(pixel stride of the buffer, channel offset of the view)"""
    return (ld, 0) if variant == "table" else (ld + 16, 8)


class Buf:
    """a guarded flat buffer holding an NHWC map of `ld` channels per pixel; the view is channels [off, off + C)"""

    def __init__(self, shape3, C_, ld, off, fill, dtype=torch.bfloat16):
        self.shape3, self.C, self.ld, self.off = shape3, C_, ld, off
        n = shape3[0] * shape3[1] * shape3[2] * ld
        self.flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.map = self.flat[GUARD:GUARD + n].view(*shape3, ld)

    @property
    def view(self):
        return self.map[..., self.off:self.off + self.C]

    @property
    def ptr(self):
        return self.flat.data_ptr() + (GUARD + self.off) * self.flat.element_size()


def in_buf(vals, ld, off):
    """NaN everywhere but the view"""
    b = Buf(tuple(vals.shape[:3]), vals.shape[3], ld, off, NAN)
    b.view.copy_(vals.to(torch.bfloat16))
    return b


def out_buf(shape3, C_, ld, off):
    """sentinels everywhere, NaN in the view: every element of the view must be written, nothing else touched"""
    b = Buf(shape3, C_, ld, off, SENT)
    b.view.fill_(NAN)
    return b


def check_out(b, ref, what):
    exp = torch.full_like(b.flat, SENT)
    n = exp.numel() - 2 * GUARD
    exp[GUARD:GUARD + n].view(*b.shape3, b.ld)[..., b.off:b.off + b.C] = ref.to(b.flat.dtype)
    torch.cuda.synchronize()
    assert torch.equal(b.flat, exp), (what, "result, channels beyond C, neighbouring channels or guards differ")


def flat_out(n, dtype):
    f = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
    f[GUARD:GUARD + n] = NAN
    return f


def check_flat(f, ref, what):
    exp = torch.full_like(f, SENT)
    exp[GUARD:GUARD + ref.numel()] = ref.reshape(-1).to(f.dtype)
    torch.cuda.synchronize()
    assert torch.equal(f, exp), (what, "result or guards differ")


def desc(c, **kw):
    d = L.mi_gconv_desc()
    d.N, d.H, d.W, d.Cin, d.Cout, d.G = N, c.H, c.W, c.C, c.C, c.G
    d.kh, d.kw, d.stride, d.padding, d.dilation = 3, 3, c.stride, 1, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def packed(c):
    """mi_gconv_pack_weight into guarded NaN buffers: both images must equal the reference image, zero entries included"""
    n = L.lib().mi_gconv_weight_image_bytes(c.C, c.Cg) // 2
    assert n == c.wf.numel()
    wm = c.w.float().to(DEV)
    wf, wd = flat_out(n, torch.bfloat16), flat_out(n, torch.bfloat16)
    e = wf.element_size()
    L.check(L.lib().mi_gconv_pack_weight(wm.data_ptr(), c.C, c.Cg, wf.data_ptr() + GUARD * e, wd.data_ptr() + GUARD * e, L.stream_ptr()),
            "mi_gconv_pack_weight")
    check_flat(wf, c.wf, "forward image")
    check_flat(wd, c.wd, "data-gradient image")
    return wf.data_ptr() + GUARD * e, wd.data_ptr() + GUARD * e, (wf, wd)


def run_wgrad(c, xb, dyb, with_bias):
    """-> (guarded gw buffer, guarded gbias buffer or None, number of split partials)"""
    d = desc(c, x=xb.ptr, ldx=xb.ld, y=dyb.ptr, ldy=dyb.ld)
    ns = C.c_int32(0)
    need = L.check(L.lib().mi_gconv_wgrad_plan(C.byref(d), C.byref(ns)), "mi_gconv_wgrad_plan")
    assert need == ns.value * (c.C * c.Cg * 9 + c.C) * 4
    ws = torch.full((need // 4 + 2 * GUARD,), NAN, dtype=torch.float32, device=DEV)
    gw = flat_out(c.C * c.Cg * 9, torch.float32)
    gb = flat_out(c.C, torch.float32) if with_bias else None
    d.gw, d.gbias = gw.data_ptr() + 4 * GUARD, (gb.data_ptr() + 4 * GUARD if with_bias else None)
    d.ws, d.ws_bytes = ws.data_ptr() + 4 * GUARD, need
    L.check(L.lib().mi_gconv_wgrad(C.byref(d), L.stream_ptr()), "mi_gconv_wgrad")
    torch.cuda.synchronize()
    assert bool(ws[:GUARD].isnan().all()) and bool(ws[GUARD + need // 4:].isnan().all()), "the workspace was overrun"
    return gw, gb, ns.value


# --------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("H,W,stride", MAPS)
@pytest.mark.parametrize("Cg,G,ld", GROUPS)
def test_forward_dgrad_wgrad_exact(Cg, G, ld, H, W, stride, variant):
    c = case(Cg, G, H, W, stride)
    ldb, off = layout(variant, c.C, ld)
    wf, wd, keep = packed(c)
    xb = in_buf(c.x, ldb, off)
    dyb = in_buf(c.dy, ldb, off)
    # forward, bias off / on
    for bias, ref in ((None, c.y), (c.bias.float().to(DEV), c.yb)):
        yb = out_buf((N, c.Ho, c.Wo), c.C, ldb, off)
        d = desc(c, x=xb.ptr, ldx=ldb, y=yb.ptr, ldy=ldb, w=wf, bias=L.ptr(bias))
        L.check(L.lib().mi_gconv_fwd(C.byref(d), L.stream_ptr()), "mi_gconv_fwd")
        check_out(yb, ref, ("forward", "bias" if bias is not None else "no bias"))
    # data gradient: every pixel of dx is written by the launch (NaN pre-fill), also where a stride-2 tap never reaches
    dxb = out_buf((N, H, W), c.C, ldb, off)
    d = desc(c, x=dxb.ptr, ldx=ldb, y=dyb.ptr, ldy=ldb, w=wd)
    L.check(L.lib().mi_gconv_dgrad(C.byref(d), L.stream_ptr()), "mi_gconv_dgrad")
    check_out(dxb, c.dx, "data gradient")
    # weight gradient, without / with the bias gradient
    for with_bias in (False, True):
        gw, gb, _ = run_wgrad(c, xb, dyb, with_bias)
        check_flat(gw, c.gw, "weight gradient")
        if with_bias:
            check_flat(gb, c.gb, "bias gradient")
    # the inputs were only read
    for b, v in ((xb, c.x), (dyb, c.dy)):
        assert torch.equal(b.view, v.to(torch.bfloat16).to(DEV)) and bool(b.flat[:GUARD].isnan().all())


@pytest.mark.gpu
def test_wgrad_split_partials_exact_and_reproducible():
    Cg, G, ld, H, W, stride = SPLIT
    c = case(Cg, G, H, W, stride)
    xb, dyb = in_buf(c.x, ld, 0), in_buf(c.dy, ld, 0)
    gw1, gb1, ns = run_wgrad(c, xb, dyb, True)
    assert ns >= 2, "the plan must split this shape: the case is here to cover the split reduction"
    check_flat(gw1, c.gw, "weight gradient (split)")
    check_flat(gb1, c.gb, "bias gradient (split)")
    gw2, gb2, ns2 = run_wgrad(c, xb, dyb, True)
    assert ns2 == ns and torch.equal(gw1, gw2) and torch.equal(gb1, gb2)
