"""GPU (-m gpu): the pooling and data-movement kernels of csrc/misc_ops.hip - the SPP pools, MaxPool2d(3, 2, 1) in both
backward forms, the nearest 2x upsample, mi_copy_bf16, mi_scale_rows_f32 - the arena SGD and the full-model gradient clip
against the plain float64 / integer references of tests/pool_ref.py with NO tolerance, through the C ABI by ctypes.

The method (tests/pool_ref.py): pooled values and the max-pool code bytes are selections, so they must equal the
first-maximum-in-row-major-order reference on tie-heavy input; the gradients are integer families on which every fp32
partial sum is exact in any order, so the device must equal float64, rounded once to bf16, bit for bit - and since the
gradient lands on the element the window chose, that pins the tie rule of the SPP index planes without looking at their
private layout.  The SGD operands are dyadic so that two steps are exact with or without FMA contraction.  The conditions
are asserted on the reference of every case before anything is launched.  Three cases run Gaussian gradients and are held
to the derived bound pool_ref.sum_bound; nothing else has a tolerance.

Hygiene of every launch: every output lives in a buffer of sentinel words that must survive, is pre-filled with NaN where
accumulate = 0 and must have been written entirely; inputs hold NaN outside their views; row strides are wider than C, in
two forms (a padded row, a slice of a wider concat buffer); the SPP index planes and the max-pool code bytes are guarded the
same way.  The branches a case reaches are computed on the host from its shape and counted; the table must be complete."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pool_ref as R
from yolov7_d2_amd import _lib as L
from yolov7_d2_amd import optim

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -1536.0
GUARD = 64
NAN = float("nan")
F64 = torch.float64
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
SEEN = collections.Counter()


def sp():
    return L.stream_ptr()


def T_(a):
    """numpy -> device tensor of the same dtype"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Buf:
    """rows x width elements at row stride ld inside a flat buffer with GUARD elements before and after: `fill` in the view,
    `other` everywhere else (SENT for outputs, NaN for inputs)"""

    def __init__(self, nrows, width, ld, dtype, fill=NAN, other=SENT):
        self.nrows, self.width, self.ld, self.other = nrows, width, ld, other
        self.flat = torch.full((nrows * ld + 2 * GUARD,), other, dtype=dtype, device=DEV)
        self.set(fill)

    def _v(self, flat=None):
        flat = self.flat if flat is None else flat
        return flat[GUARD:GUARD + self.nrows * self.ld].view(self.nrows, self.ld)[:, :self.width]

    def _t(self, value, cast=True):
        """numpy / host tensors: rounded to the buffer's type on the HOST where `cast` (a device cast may flush a subnormal)"""
        if isinstance(value, np.ndarray):
            value = torch.from_numpy(np.ascontiguousarray(value))
        if torch.is_tensor(value):
            value = value.reshape(self.nrows, self.width)
            if cast and not value.is_cuda:
                value = value.to(self.flat.dtype)
            value = value.to(DEV)
        return value

    def set(self, fill):
        fill = self._t(fill)
        self._v()[...] = fill.to(self.flat.dtype) if torch.is_tensor(fill) else fill

    @property
    def ptr(self):
        return self.ptr_at(0)

    def ptr_at(self, col):
        return self.flat.data_ptr() + (GUARD + col) * self.flat.element_size()

    def view(self):
        return self._v().to(F64)

    def complaint(self, name, value, bits=False):
        """None if the WHOLE buffer is `value` (NaN = NaN; bits: the same 16-bit words) in the view and untouched elsewhere"""
        value = self._t(value, cast=bits)
        if bits:
            exp = torch.full(self.flat.shape, self.other, dtype=self.flat.dtype, device=DEV)
            self._v(exp)[...] = value.to(self.flat.dtype)
            bad = self.flat.view(torch.int16) != exp.view(torch.int16)
        else:
            exp = torch.full(self.flat.shape, self.other, dtype=F64, device=DEV)
            self._v(exp)[...] = value.to(F64)
            got = self.flat.to(F64)
            bad = ~((got == exp) | (got.isnan() & exp.isnan()))
        if not bool(bad.any()):
            return None
        i = int(torch.nonzero(bad)[0])
        return "%s: %d elements differ, first at flat %d (row %d, column %d): got %r, expected %r" % (
            name, int(bad.sum()), i - GUARD, (i - GUARD) // self.ld, (i - GUARD) % self.ld, float(self.flat[i]), float(exp[i]))

    def guards(self, name, unwritten=NAN):
        """None if everything outside the view is untouched and the view holds no `unwritten` element"""
        v = self.view()
        left = int((v.isnan() if unwritten != unwritten else v == unwritten).sum())
        if left:
            return "%s: %d elements were not written" % (name, left)
        return self.complaint(name + " (outside the view)", v)


def some(*complaints):
    return [s for s in complaints if s]


class Slot:
    """C channels of npix pixels as a kernel sees them: a padded row (ld = C + 8) or, wide, the upper half of a 2C-channel
    concat buffer (ld = 2C + 8) whose lower half holds `rest` and must survive.  Outputs: value NaN or the prior, rest 7;
    inputs: rest NaN and NaN around."""

    def __init__(self, npix, Cc, wide, dtype=BF, value=NAN, out=True):
        self.C, self.wide = Cc, wide
        self.rest = 7.0 if out else NAN
        self.buf = Buf(npix, 2 * Cc if wide else Cc, (2 * Cc if wide else Cc) + 8, dtype, self._full(value, npix), SENT if out else NAN)
        self.ptr, self.ld = self.buf.ptr_at(Cc if wide else 0), self.buf.ld

    def _full(self, value, npix):
        """on the host, in the dtype of `value`"""
        if isinstance(value, np.ndarray):
            value = torch.from_numpy(np.ascontiguousarray(value)).reshape(npix, self.C)
        else:
            value = torch.full((npix, self.C), value, dtype=F64)
        return torch.cat([torch.full_like(value, self.rest), value], 1) if self.wide else value

    def complaint(self, name, value, bits=False):
        return self.buf.complaint(name, self._full(value, self.buf.nrows), bits)

    def values(self):
        return self.buf.view()[:, -self.C:].cpu().numpy()


def in_slot(a, wide=False, dtype=BF):
    a = np.asarray(a)
    return Slot(a.size // a.shape[-1], a.shape[-1], wide, dtype, a, out=False)


def out_slot(shape, wide=False, prior=None):
    return Slot(int(np.prod(shape[:-1])), shape[-1], wide, BF, NAN if prior is None else prior)


def px(a):
    """[N][H][W][C] -> [pixels][C]"""
    return np.asarray(a).reshape(-1, np.asarray(a).shape[-1])


def code_buf(n, fill=255):
    return Buf(1, n, n, U8, fill, 77)


# ----------------------------------------------------------------------------------------------------------------- SPP
class SppOut:
    """y5, y9, y13: slices [C, 4C) of one 4C-channel concat buffer (channels [0, C) hold 7 and must survive), as the YOLOX
    plan lays them out, or three padded buffers"""

    def __init__(self, npix, Cc, cat, values=None):
        self.cat, self.C, self.npix = cat, Cc, npix
        out = values is None
        vals = [torch.full((npix, Cc), NAN, dtype=F64, device=DEV)] * 3 if out else [T_(px(v)).to(F64) for v in values]
        if cat:
            self.head = torch.full((npix, Cc), 7.0 if out else NAN, dtype=F64, device=DEV)
            self.bufs = [Buf(npix, 4 * Cc, 4 * Cc + 16, BF, torch.cat([self.head] + vals, 1), SENT if out else NAN)]
            self.ptrs, self.ld = [self.bufs[0].ptr_at(Cc * (i + 1)) for i in range(3)], 4 * Cc + 16
        else:
            self.bufs = [Buf(npix, Cc, Cc + 24, BF, v, SENT if out else NAN) for v in vals]
            self.ptrs, self.ld = [b.ptr for b in self.bufs], Cc + 24

    def complaints(self, name, refs):
        refs = [T_(px(r)).to(F64) for r in refs]
        if self.cat:
            return some(self.bufs[0].complaint(name + " y5|y9|y13", torch.cat([self.head] + refs, 1)))
        return some(*[b.complaint("%s y%d" % (name, k), r) for b, k, r in zip(self.bufs, R.SPP_KS, refs)])


def spp_forward(shape, x, cat):
    N, H, W, Cc = shape
    npix = N * H * W
    xin = in_slot(px(x), wide=not cat)
    y = SppOut(npix, Cc, cat)
    idx = code_buf(6 * npix * Cc)
    L.check(L.lib().mi_spp_pool_fwd(xin.ptr, xin.ld, *y.ptrs, y.ld, idx.ptr, N, H, W, Cc, sp()), "spp_fwd")
    torch.cuda.synchronize()
    for k in R.spp_labels(N, H, W, Cc, False):
        SEEN[k] += 1
    return y, idx


def spp_backward(shape, idx, gs, prior, acc, cat):
    N, H, W, Cc = shape
    d = SppOut(N * H * W, Cc, cat, gs)
    dx = out_slot(shape, wide=cat, prior=px(prior) if acc else None)
    before = idx.flat.clone()
    L.check(L.lib().mi_spp_pool_bwd(*d.ptrs, d.ld, idx.ptr, dx.ptr, dx.ld, acc, N, H, W, Cc, sp()), "spp_bwd")
    torch.cuda.synchronize()
    for k in R.spp_labels(N, H, W, Cc, True) | {"spp_bwd:acc%d" % acc}:
        SEEN[k] += 1
    return dx, some(None if torch.equal(before, idx.flat) else "the backward wrote to the index planes")


def run_spp(shape, fam, seed, cat, bwd=True):
    """forward on a family, then the backward on the gradient family with accumulate 0 and 1"""
    N, H, W, Cc = shape
    name = "spp %r %s%s" % (shape, fam, " concat" if cat else "")
    x = R.family(fam, shape, seed)
    ref = R.spp_fwd(x)
    y, idx = spp_forward(shape, x, cat)
    bad = y.complaints(name, [v for v, _ in ref]) + some(idx.guards(name + " index planes", 255))
    if not bwd:
        return bad
    poss = [p for _, p in ref]
    gs, prior = [R.grads(shape, seed + 1 + i) for i in range(3)], R.grads(shape, seed + 4)
    assert R.grad_family_ok(R.spp_bwd(poss, gs, prior, np.abs), prior, *gs)
    ref0 = R.spp_bwd(poss, gs)
    for acc in (0, 1):
        dx, b = spp_backward(shape, idx, gs, prior, acc, cat)
        bad += b + some(dx.complaint("%s dx accumulate %d" % (name, acc), px(R.round_bf16(ref0 + prior * acc))))
    return bad


@pytest.mark.parametrize("plane", R.SPP_PLANES)
def test_spp_pools_and_their_gradient_exact(plane):
    """every plane of the table - 63 pixels, the degenerate 1 x 14 and 14 x 1, 3 x 40 (narrower than every radius one way),
    513 pixels (the smallest second round), 1024 (the backward's limit) - on grids of 8 (identity block remap), 16 (a real
    permutation), 9 and 1 (remap off), all six input families per plane: y5, y9, y13 equal the first-maximum reference, and
    the integer gradient, accumulate 0 and 1, equals the float64 scatter-add rounded once - so every window chose the
    first maximum in row-major order"""
    bad = []
    for j, (N, Cc, f0, f1) in enumerate(R.spp_cases(plane)):
        for t, fam in enumerate((f0, f1)):
            bad += run_spp((N,) + plane + (Cc,), fam, 1000 * plane[0] + 10 * plane[1] + j, cat=(j + t) % 2 == 0)
    assert bad == [], bad[:8]


def test_spp_forward_three_rounds():
    """33 x 32 = 1056 pixels: a thread of the forward walks three pixels; the backward refuses this plane"""
    assert run_spp((1, 33, 32, 64), "levels", 5, cat=True, bwd=False) == []


def test_spp_gaussian_gradient_within_the_derived_bound():
    """Gaussian dy and prior dx on SiLU input at 19 x 27, accumulate 1: n (per pixel, from the reference) terms added in fp32
    in some order and stored once as bf16"""
    shape = (2, 19, 27, 64)
    x = R.family("silu", shape, 11)
    poss = [p for _, p in R.spp_fwd(x)]
    rng = np.random.default_rng(12)
    gs, prior = [R.round_bf16(rng.standard_normal(shape)) for _ in range(3)], R.round_bf16(rng.standard_normal(shape))
    _, idx = spp_forward(shape, x, True)
    dx, bad = spp_backward(shape, idx, gs, prior, 1, False)
    ref = R.spp_bwd(poss, gs, prior)
    bound = R.sum_bound(ref, R.spp_bwd(poss, gs, prior, np.ones_like), R.spp_bwd(poss, gs, prior, np.abs))
    ratio = float((np.abs(dx.values() - px(ref)) / px(bound)).max())
    print("spp backward, Gaussian gradients: worst |device - float64| / bound %.3f" % ratio)
    assert bad + some(dx.buf.guards("dx")) == [] and ratio <= 1.0


def test_spp_rejections_return_errors_and_write_nothing():
    lib = L.lib()

    def untouched(bufs):
        torch.cuda.synchronize()
        return some(*[b.complaint("refused launch", torch.full((b.nrows, b.width), 255 if b.flat.dtype == U8 else NAN, dtype=F64)) for b in bufs])

    def fwd_args(H, W, Cc=8, ld=None, null=None):
        n = H * W
        ld = Cc + 8 if ld is None else ld
        x = Buf(n, Cc, ld, BF, 1.0, NAN)
        ys = [Buf(n, Cc, ld, BF) for _ in range(3)]
        idx = code_buf(6 * n * Cc)
        a = [x.ptr, ld, ys[0].ptr, ys[1].ptr, ys[2].ptr, ld, idx.ptr, 1, H, W, Cc, sp()]
        if null is not None:
            a[null] = None
        return a, ys + [idx]

    def bwd_args(H, W, Cc=8, ld=None, null=None):
        n = H * W
        ld = Cc + 8 if ld is None else ld
        ds = [Buf(n, Cc, ld, BF, 1.0, NAN) for _ in range(3)]
        idx = code_buf(6 * n * Cc, 6)
        dx = Buf(n, Cc, ld, BF)
        a = [ds[0].ptr, ds[1].ptr, ds[2].ptr, ld, idx.ptr, dx.ptr, ld, 0, 1, H, W, Cc, sp()]
        if null is not None:
            a[null] = None
        return a, [dx]

    assert 25 * 41 == 2 * R.SPP_T + 1 and 65 * 65 * 40 > 160 * 1024 >= 64 * 64 * 40
    a, outs = bwd_args(25, 41)
    assert lib.mi_spp_pool_bwd(*a) != 0 and b"spp_bwd" in lib.mi_last_error() and untouched(outs) == []
    a, outs = fwd_args(65, 65)
    assert lib.mi_spp_pool_fwd(*a) != 0 and b"spp_fwd" in lib.mi_last_error() and untouched(outs) == []
    for kw in (dict(Cc=12, ld=24), dict(ld=20), dict(null=0), dict(null=3), dict(null=6)):
        a, outs = fwd_args(7, 9, **kw)
        assert lib.mi_spp_pool_fwd(*a) == R.MI_EINVAL and b"spp_fwd" in lib.mi_last_error() and untouched(outs) == [], kw
    for kw in (dict(Cc=12, ld=24), dict(ld=20), dict(null=1), dict(null=4), dict(null=5)):
        a, outs = bwd_args(7, 9, **kw)
        assert lib.mi_spp_pool_bwd(*a) == R.MI_EINVAL and b"spp_bwd" in lib.mi_last_error() and (kw.get("null") == 5 or untouched(outs) == []), kw


# ------------------------------------------------------------------------------------------------- MaxPool2d(3, 2, 1)
def pooled(shape):
    N, H, W, Cc = shape
    return (N, (H + 1) // 2, (W + 1) // 2, Cc)


def run_maxpool_fwd(shape, x, vals, pos, wide, name):
    """mi_maxpool3x3s2_fwd and _fwd_idx: values (the sign of a zero is not compared) and the code bytes"""
    N, H, W, Cc = shape
    osh = pooled(shape)
    items = int(np.prod(osh)) // 8
    xin = in_slot(px(x), wide)
    y, y2 = out_slot(osh, not wide), out_slot(osh, wide)
    code = code_buf(int(np.prod(osh)))
    L.check(L.lib().mi_maxpool3x3s2_fwd(xin.ptr, xin.ld, y.ptr, y.ld, N, H, W, Cc, sp()), "maxpool_fwd")
    L.check(L.lib().mi_maxpool3x3s2_fwd_idx(xin.ptr, xin.ld, y2.ptr, y2.ld, code.ptr, N, H, W, Cc, sp()), "maxpool_fwd_idx")
    torch.cuda.synchronize()
    if R.trips(items) > 1:
        SEEN["maxpool_fwd:trip2"] += 1
        SEEN["maxpool_fwd_idx:trip2"] += 1
    return some(y.complaint(name + " fwd", px(vals)), y2.complaint(name + " fwd_idx", px(vals)),
                code.complaint(name + " code bytes", R.maxpool_code(pos).reshape(1, -1)))


def run_maxpool_bwd(shape, x, pos, g, prior, acc, wide, name):
    """mi_maxpool3x3s2_bwd_idx on the reference's code bytes and mi_maxpool3x3s2_bwd from x: both the float64 scatter-add"""
    N, H, W, Cc = shape
    ref = R.maxpool_bwd(pos, g, 3, 2, 1, H, W)
    assert R.grad_family_ok(R.maxpool_bwd(pos, np.abs(g), 3, 2, 1, H, W) + np.abs(prior), g, prior)
    ref = px(R.round_bf16(ref + prior * acc))
    xin, gin = in_slot(px(x), wide), in_slot(px(g), not wide)
    codes = R.maxpool_code(pos).reshape(1, -1)
    code = code_buf(codes.size, codes)
    dx_i, dx_x = out_slot(shape, wide, px(prior) if acc else None), out_slot(shape, not wide, px(prior) if acc else None)
    L.check(L.lib().mi_maxpool3x3s2_bwd_idx(code.ptr, gin.ptr, gin.ld, dx_i.ptr, dx_i.ld, acc, N, H, W, Cc, sp()), "maxpool_bwd_idx")
    L.check(L.lib().mi_maxpool3x3s2_bwd(xin.ptr, xin.ld, gin.ptr, gin.ld, dx_x.ptr, dx_x.ld, acc, N, H, W, Cc, sp()), "maxpool_bwd")
    torch.cuda.synchronize()
    for k in ("maxpool_bwd", "maxpool_bwd_idx"):
        SEEN["%s:acc%d" % (k, acc)] += 1
        if R.trips(N * H * W * Cc // 8) > 1:
            SEEN[k + ":trip2"] += 1
    return some(dx_i.complaint("%s bwd_idx accumulate %d" % (name, acc), ref), dx_x.complaint("%s bwd accumulate %d" % (name, acc), ref),
                code.complaint(name + " code bytes (an input)", codes))


@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES)
def test_maxpool3x3s2_exact(shape):
    """both forward forms on every family: the values and, byte for byte, the position dy * 3 + dx of the first maximum;
    both backward forms on the integer gradient with accumulate 0 and 1: equal to the reference and so to each other"""
    bad = []
    for i, fam in enumerate(R.FAMILIES):
        x = R.family(fam, shape, 30 + i)
        vals, pos = R.maxpool_first(x, 3, 2, 1)
        name = "maxpool %r %s" % (shape, fam)
        bad += run_maxpool_fwd(shape, x, vals, pos, i % 2 == 1, name)
        g, prior = R.grads(pos.shape, 40 + i), R.grads(shape, 50 + i)
        for acc in (0, 1):
            bad += run_maxpool_bwd(shape, x, pos, g, prior, acc, (i + acc) % 2 == 1, name)
    assert bad == [], bad[:8]


def test_maxpool_gaussian_gradient_within_the_derived_bound():
    shape = R.MAXPOOL_SHAPES[0]
    N, H, W, Cc = shape
    x = R.family("silu", shape, 61)
    _, pos = R.maxpool_first(x, 3, 2, 1)
    rng = np.random.default_rng(62)
    g, prior = R.round_bf16(rng.standard_normal(pos.shape)), R.round_bf16(rng.standard_normal(shape))
    ref = R.maxpool_bwd(pos, g, 3, 2, 1, H, W) + prior
    bound = R.sum_bound(ref, R.maxpool_bwd(pos, np.ones_like(g), 3, 2, 1, H, W) + 1, R.maxpool_bwd(pos, np.abs(g), 3, 2, 1, H, W) + np.abs(prior))
    xin, gin, code = in_slot(px(x)), in_slot(px(g)), code_buf(pos.size, R.maxpool_code(pos).reshape(1, -1))
    dx_i, dx_x = out_slot(shape, False, px(prior)), out_slot(shape, True, px(prior))
    L.check(L.lib().mi_maxpool3x3s2_bwd_idx(code.ptr, gin.ptr, gin.ld, dx_i.ptr, dx_i.ld, 1, N, H, W, Cc, sp()), "maxpool_bwd_idx")
    L.check(L.lib().mi_maxpool3x3s2_bwd(xin.ptr, xin.ld, gin.ptr, gin.ld, dx_x.ptr, dx_x.ld, 1, N, H, W, Cc, sp()), "maxpool_bwd")
    torch.cuda.synchronize()
    ratios = [float((np.abs(d.values() - px(ref)) / px(bound)).max()) for d in (dx_i, dx_x)]
    print("max-pool backward, Gaussian gradients: worst |device - float64| / bound: bwd_idx %.3f, bwd %.3f" % tuple(ratios))
    assert some(dx_i.buf.guards("bwd_idx dx"), dx_x.buf.guards("bwd dx")) == [] and max(ratios) <= 1.0


@functools.lru_cache(maxsize=None)
def big_maxpool(N):
    """364 x 364 x 64 on {-1, 0, 1} in float32 (exact for a selection) and its reference, computed once and left unchanged"""
    shape = (N, 364, 364, 64)
    x = R.levels_f32(shape, 70 + N)
    vals, pos = R.maxpool_first(x, 3, 2, 1)
    return shape, x, vals, pos


def test_maxpool_forward_second_grid_trip():
    """N = 4 at 364 x 364 x 64: 4 * 182 * 182 * 8 items, just above the 4096 blocks of 256: the second loop trip"""
    shape, x, vals, pos = big_maxpool(4)
    items = int(np.prod(pooled(shape))) // 8
    assert items > R.EW_CAP * 256 and R.trips(items) == 2
    assert run_maxpool_fwd(shape, x, vals, pos, False, "maxpool %r" % (shape,)) == []


def test_maxpool_backward_second_grid_trip():
    """the backward forms run one item per INPUT pixel group: 364 * 364 * 8 items at N = 1"""
    shape, x, _, pos = big_maxpool(1)
    assert np.prod(shape) // 8 > R.EW_CAP * 256 and R.trips(int(np.prod(shape)) // 8) == 2
    g, prior = R.grads(pos.shape, 72, np.float32), R.grads(shape, 73, np.float32)
    assert run_maxpool_bwd(shape, x, pos, g, prior, 1, False, "maxpool %r" % (shape,)) == []


# ----------------------------------------------------------------------------------------------------------- upsample
def run_upsample_fwd(shape, x, wide):
    N, H, W, Cc = shape
    xin, y = in_slot(px(x), wide), out_slot((N, 2 * H, 2 * W, Cc), not wide)
    L.check(L.lib().mi_upsample2x_fwd(xin.ptr, xin.ld, y.ptr, y.ld, N, H, W, Cc, sp()), "upsample_fwd")
    torch.cuda.synchronize()
    if R.trips(N * 4 * H * W * Cc // 8) > 1:
        SEEN["upsample_fwd:trip2"] += 1
    return some(y.complaint("upsample fwd %r" % (shape,), px(R.upsample2x(x)), bits=True))


def run_upsample_bwd(shape, g, prior, acc, wide, launch_only=False):
    N, H, W, Cc = shape
    gin = in_slot(px(g), wide)
    dx = out_slot(shape, not wide, px(prior) if acc else None)
    L.check(L.lib().mi_upsample2x_bwd(gin.ptr, gin.ld, dx.ptr, dx.ld, acc, N, H, W, Cc, sp()), "upsample_bwd")
    torch.cuda.synchronize()
    SEEN["upsample_bwd:acc%d" % acc] += 1
    if R.trips(N * H * W * Cc // 8) > 1:
        SEEN["upsample_bwd:trip2"] += 1
    if launch_only:
        return dx
    ab = R.upsample2x_bwd(np.abs(g)) + np.abs(prior)
    assert R.grad_family_ok(ab, g, prior) and ab.max() <= 5 * R.GRAD_MAX
    ref = R.round_bf16(R.upsample2x_bwd(g) + prior * acc)
    return some(dx.complaint("upsample bwd %r accumulate %d" % (shape, acc), px(ref)))


@pytest.mark.parametrize("shape", R.UPSAMPLE_SHAPES)
def test_upsample2x_exact(shape):
    """the forward is a bit copy (+-0, +-inf, the largest and smallest normal, a subnormal among the values): the 16-bit
    words are compared; the backward is the exact sum of the 2 x 2 block (+ prior) on the integer family"""
    N, H, W, Cc = shape
    bad = []
    for wide in (False, True):
        bad += run_upsample_fwd(shape, R.specials(N * H * W * Cc, 80 + wide).reshape(shape), wide)
        for acc in (0, 1):
            bad += run_upsample_bwd(shape, R.grads((N, 2 * H, 2 * W, Cc), 82 + acc), R.grads(shape, 84), acc, wide)
    assert bad == [], bad[:8]


def test_upsample_gaussian_gradient_within_the_derived_bound():
    shape = R.UPSAMPLE_SHAPES[0]
    N, H, W, Cc = shape
    rng = np.random.default_rng(86)
    g, prior = R.round_bf16(rng.standard_normal((N, 2 * H, 2 * W, Cc))), R.round_bf16(rng.standard_normal(shape))
    ref = R.upsample2x_bwd(g) + prior
    bound = R.sum_bound(ref, 5, R.upsample2x_bwd(np.abs(g)) + np.abs(prior))
    dx = run_upsample_bwd(shape, g, prior, 1, False, launch_only=True)
    ratio = float((np.abs(dx.values() - px(ref)) / px(bound)).max())
    print("upsample backward, Gaussian gradients: worst |device - float64| / bound %.3f" % ratio)
    assert dx.buf.guards("dx") is None and ratio <= 1.0


def test_upsample_second_grid_trip():
    """forward N = 1, backward N = 4 at 182 x 182 x 64 (its dy is 364 x 364): 4 * 182 * 182 * 8 items each"""
    shape = (1, 182, 182, 64)
    assert R.trips(4 * 182 * 182 * 8) == 2
    bad = run_upsample_fwd(shape, R.levels_f32(shape, 87), False)
    shape = (4, 182, 182, 64)
    bad += run_upsample_bwd(shape, R.grads((4, 364, 364, 64), 88, np.float32), R.grads(shape, 89, np.float32), 1, False)
    assert bad == [] and SEEN["upsample_fwd:trip2"] and SEEN["upsample_bwd:trip2"], bad


# ---------------------------------------------------------------------------------------------------------------- copy
def run_copy(npix, Cc, wide, acc, levels=False):
    name = "copy npix %d C %d %s accumulate %d" % (npix, Cc, "concat slice" if wide else "ld = C", acc)
    n = npix * Cc
    if levels:
        a, b = R.levels_f32((npix, Cc), 90), R.grads((npix, Cc), 91, np.float32)
    elif acc:
        a, b = (v.reshape(npix, Cc) for v in R.acc_pairs(n, 92 + Cc))
    else:
        a, b = R.specials(n, 93 + Cc).reshape(npix, Cc), None
    if wide:
        src, dst = in_slot(a, True), Slot(npix, Cc, True, BF, b if acc else NAN)
        args = (src.ptr, src.ld, dst.ptr, dst.ld)
    else:                                               # ld = C: dense rows between the guards
        src, dst = Buf(npix, Cc, Cc, BF, a, NAN), Buf(npix, Cc, Cc, BF, b if acc else NAN)
        args = (src.ptr, Cc, dst.ptr, Cc)
    L.check(L.lib().mi_copy_bf16(*args, acc, npix, Cc, sp()), "copy_bf16")
    torch.cuda.synchronize()
    SEEN["copy:acc%d" % acc] += 1
    if R.trips(npix * Cc // 8) > 1:
        SEEN["copy:trip2"] += 1
    return some(dst.complaint(name, R.copy_acc(a, b), False) if acc else dst.complaint(name, a, True))


@pytest.mark.parametrize("npix", R.COPY_NPIX)
def test_copy_bf16_exact(npix):
    """accumulate 0: a bit copy, special values included; accumulate 1: bf16(fl32(a + b)) on pairs up to 40 binades apart, ties
    on the bf16 grid, cancellation, infinities and overflow"""
    bad = []
    for Cc in R.COPY_CS:
        for wide in (False, True):
            for acc in (0, 1):
                bad += run_copy(npix, Cc, wide, acc)
    assert bad == [], bad[:8]


def test_copy_second_grid_trip():
    npix = 131200
    assert npix * 8 > R.EW_CAP * 256 and R.trips(npix * 8) == 2
    assert run_copy(npix, 64, True, 0, levels=True) + run_copy(npix, 64, False, 1, levels=True) == []


# ---------------------------------------------------------------------------------------------------------- scale_rows
def run_scale_rows(rows, rowlen, inplace):
    rng = np.random.default_rng(rows * 1000 + rowlen)
    n = rows * rowlen
    g = (rng.standard_normal((rows, rowlen)) * np.ldexp(1.0, rng.integers(-8, 9, (rows, rowlen)))).astype(np.float32)
    sc = rng.standard_normal(rows).astype(np.float32)
    ref = R.scale_rows(g, sc).reshape(1, n)
    gb, sb = Buf(1, n, n, F32, g.reshape(1, n), SENT if inplace else NAN), Buf(1, rows, rows, F32, sc.reshape(1, rows), NAN)
    ob = gb if inplace else Buf(1, n, n, F32)
    L.check(L.lib().mi_scale_rows_f32(gb.ptr, sb.ptr, ob.ptr, rows, rowlen, sp()), "scale_rows")
    torch.cuda.synchronize()
    SEEN["scale_rows:float4" if rowlen % 4 == 0 else "scale_rows:scalar"] += 1
    if rowlen % 4 == 0 and R.trips(n // 4, R.SCALE_ROWS_CAP) > 1:
        SEEN["scale_rows:trip2"] += 1
    name = "scale_rows %d x %d%s" % (rows, rowlen, " in place" if inplace else "")
    return some(ob.complaint(name, ref), sb.complaint(name + " (scale, an input)", sc.reshape(1, rows)),
                None if inplace else gb.complaint(name + " (g, an input)", g.reshape(1, n)))


@pytest.mark.parametrize("rows,rowlen", R.SCALE_ROWS_SHAPES)
def test_scale_rows_exact(rows, rowlen):
    """one fp32 multiply per element: bit for bit float32(float64(g) * float64(scale)), into another buffer and in place"""
    assert run_scale_rows(rows, rowlen, False) + run_scale_rows(rows, rowlen, True) == []


def test_scale_rows_second_grid_trip():
    assert 2100 * 1000 // 4 > R.SCALE_ROWS_CAP * 256
    assert run_scale_rows(2100, 1000, True) == [] and SEEN["scale_rows:trip2"]


# ----------------------------------------------------------------------------------------------------------------- SGD
def run_sgd():
    """two steps over the arena of pool_ref.SGD_SEGS, compared after each"""
    n = R.SGD_ARENA
    segs, own = R.sgd_segs(), R.sgd_owned()
    p, g, m = R.sgd_operands(7)
    for a in (p, g, m):
        a[~own] = SENT                                  # unowned gaps: sentinels in p, g and m
    arr = (L.mi_sgd_seg * len(segs))()
    for i, (o, c, wd, lr) in enumerate(segs):
        arr[i].offset, arr[i].count, arr[i].weight_decay, arr[i].lr = o, c, wd, lr
        for k in R.sgd_labels(o, c):
            SEEN[k] += 1
    sd = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    pb, gb = Buf(1, n, n, F32, p.reshape(1, n)), Buf(1, n, n, F32, g.reshape(1, n))
    mb = Buf(1, n, n, F32, np.where(own, NAN, SENT).reshape(1, n))       # the first step may not read it
    bad = []
    for step in (0, 1):
        assert R.sgd_family_ok(p, g, m, segs, R.SGD_MOMENTUM, R.SGD_GRAD_SCALE, step == 0)
        p, m = R.sgd_step(p, g, m, segs, R.SGD_MOMENTUM, R.SGD_GRAD_SCALE, step == 0)
        assert not np.isnan(m).any() and (m[~own] == SENT).all() and (p[~own] == SENT).all()
        L.check(L.lib().mi_sgd_momentum_step(pb.ptr, gb.ptr, mb.ptr, sd.data_ptr(), len(segs), R.SGD_MOMENTUM, R.SGD_GRAD_SCALE,
                                             int(step == 0), sp()), "sgd")
        torch.cuda.synchronize()
        SEEN["sgd:first_step" if step == 0 else "sgd:later_step"] += 1
        bad += some(pb.complaint("sgd step %d p" % step, p.reshape(1, n)), mb.complaint("sgd step %d momentum" % step, m.reshape(1, n)),
                    gb.complaint("sgd step %d g (an input)" % step, g.reshape(1, n)))
    return bad


def test_sgd_two_steps_exact():
    """first_step = 1 on a NaN-filled momentum buffer, then first_step = 0, grad_scale 2^-2, two (lr, wd) pairs: a segment of
    whole float4 pairs, one whose second vector stops mid-block plus a 3-element tail, a 3-element segment, one at an
    offset = 2 mod 4 (scalar only) and an empty one; p and the momentum buffer equal float64 bit for bit after each step, and
    the sentinels between the segments survive in p, g and m"""
    assert run_sgd() == []


# ---------------------------------------------------------------------------------------------------------------- clip
def clip_case(g0, max_norm):
    """optim.clip_grad_norm_flat_ on the device and torch.nn.utils.clip_grad_norm_ on the CPU -> device g, norm, torch g, norm"""
    n = g0.numel()
    gb = Buf(1, n, n, F32, g0.reshape(1, n).clone())
    ws = torch.empty(1024, dtype=F64, device=DEV)
    g = gb.flat[GUARD:GUARD + n]
    norm = optim.clip_grad_norm_flat_(g, max_norm, ws)
    torch.cuda.synchronize()
    w = torch.zeros(n, requires_grad=True)
    w.grad = g0.clone()
    tn = torch.nn.utils.clip_grad_norm_([w], max_norm)
    assert gb.complaint("guards", gb.view()) is None
    return g.cpu(), float(norm), w.grad, float(tn)


def same(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def test_full_model_clip_propagates_a_nan_norm():
    """one NaN among 70 001 gradients: torch.nn.utils.clip_grad_norm_ returns a NaN norm and poisons every gradient, so that
    the divergence shows in the next loss instead of a silent step on garbage; the device must do the same"""
    g0 = torch.randn(70001, generator=torch.Generator().manual_seed(3))
    g0[12345] = NAN
    g, norm, tg, tnorm = clip_case(g0, 1.0)
    assert bool(tg.isnan().all()) and tnorm != tnorm
    assert norm != norm and bool(g.isnan().all()), "%d of %d gradients are not NaN, norm %r" % (int((~g.isnan()).sum()), g.numel(), norm)


def test_full_model_clip_infinite_norm_and_small_norm():
    """one +inf: the coefficient is 0, finite entries become 0 and the infinite one NaN, as in torch; a norm below max_norm
    leaves the buffer bit-identical"""
    g0 = torch.randn(70001, generator=torch.Generator().manual_seed(4))
    g0[777] = float("inf")
    g, norm, tg, tnorm = clip_case(g0, 1.0)
    assert tnorm == float("inf") and int(tg.isnan().sum()) == 1 and float(tg[0]) == 0
    assert norm == tnorm and same(g, tg)
    g0 = torch.randn(70001, generator=torch.Generator().manual_seed(5))
    g, norm, tg, tnorm = clip_case(g0, 1000.0)
    exact = float(g0.double().norm())
    assert exact < 1000 and torch.equal(g.view(torch.int32), g0.view(torch.int32)) and torch.equal(tg, g0)
    # fp32 squares summed in pairs, then float64: each term within 2 * 2^-24 of its square, the root rounded once to fp32
    assert abs(norm - exact) <= exact * 2.0 ** -22


# ------------------------------------------------------------------------------------------------------------ coverage
def reach(label):
    """the smallest case that reaches a branch, for a run that selected this test alone"""
    kernel, what = label.split(":")
    if kernel in ("spp_fwd", "spp_bwd"):
        plane = {"round1": (7, 9), "round2": (19, 27), "round3": (33, 32)}.get(what, (7, 9))
        N, Cc = {"remap_identity": (1, 64), "remap_permuted": (2, 64)}.get(what, (3, 24))
        return run_spp((N,) + plane + (Cc,), "levels", 1, True, bwd=what != "round3")
    if what == "trip2":
        return {"copy": test_copy_second_grid_trip, "upsample_fwd": test_upsample_second_grid_trip, "upsample_bwd": test_upsample_second_grid_trip,
                "maxpool_fwd": test_maxpool_forward_second_grid_trip, "maxpool_fwd_idx": test_maxpool_forward_second_grid_trip,
                "maxpool_bwd": test_maxpool_backward_second_grid_trip, "maxpool_bwd_idx": test_maxpool_backward_second_grid_trip,
                "scale_rows": test_scale_rows_second_grid_trip}[kernel]() or []
    if kernel in ("maxpool_bwd", "maxpool_bwd_idx"):
        return test_maxpool3x3s2_exact(R.MAXPOOL_SHAPES[2]) or []
    if kernel == "upsample_bwd":
        return test_upsample2x_exact(R.UPSAMPLE_SHAPES[1]) or []
    if kernel == "copy":
        return run_copy(37, 24, True, int(what[-1]))
    if kernel == "scale_rows":
        return run_scale_rows(3, 4 if what == "float4" else 5, False)
    assert kernel == "sgd"
    return run_sgd()


def test_every_branch_was_reached():
    """the counted table: the SPP rounds and block remaps, accumulate 0 and 1 of every backward and of the copy, the second
    grid trip of every grid-stride kernel, both paths of scale_rows and every path of the SGD.  The tests above fill it; a
    label that is still empty (this test selected alone) is reached here first."""
    bad = []
    for k in R.REQUIRED:
        if SEEN.get(k, 0) == 0:
            bad += reach(k)
    assert bad == [], bad[:8]
    for k in R.REQUIRED:
        print("%-28s %d" % (k, SEEN.get(k, 0)))
    assert set(SEEN) <= set(R.REQUIRED), set(SEEN) - set(R.REQUIRED)
    missing = [k for k in R.REQUIRED if SEEN.get(k, 0) == 0]
    assert missing == [] and len(R.REQUIRED) == 38, missing
