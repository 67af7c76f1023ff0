"""Plain references of the pooling and data-movement kernels of csrc/misc_ops.hip - the SPP max-pools (k = 5, 9, 13),
MaxPool2d(3, 2, 1) in both backward forms, the nearest 2x upsample, mi_copy_bf16, mi_scale_rows_f32 - and of the arena SGD,
the operand families on which their fp32 arithmetic is EXACT, and the one derived bound where it is not.
tests/test_gpu_pool_exact.py compares the device with these bit for bit; tests/test_pool_ref.py pins them on the CPU.
Everything here is numpy float64 / integer arithmetic on the host, independent of torch; nothing is taken from the code
under test.  Activations are NHWC arrays [N][H][W][C].

The rule the pools are held to: an output takes the FIRST maximum of its window in row-major order, out-of-bounds cells
skipped (strict `>` while scanning).  maxpool_first states it as a scan, maxpool_first_windows as np.argmax over -inf-padded
windows (argmax returns the first occurrence); F.max_pool2d on the CPU follows the same rule (tests/test_pool_ref.py).
The input domain is finite: an all -inf window is outside the contract.

The exact families (asserted on every case - grad_family_ok, sgd_family_ok - before anything is launched):
  gradients: integer dy in [-64, 64] and an integer prior dx.  Every fp32 partial sum is then an integer below 2^24 in any
    order (the predicate bounds the sum of the magnitudes per input pixel), so the device must equal round_bf16(float64 sum).
    Sums above 256 land on half-way points of the bf16 grid: round-to-even is exercised.
  SGD: lr, wd, momentum, grad_scale powers of two, p, g, m multiples of 2^-6 in [-4, 4]: every product and every sum of two
    consecutive steps (first_step = 1, then 0) is its own fp32 rounding, so the kernel must equal float64 whether or not the
    compiler contracts to FMA.  A third step needs more than 24 bits (the predicate fails: tests/test_pool_ref.py).
The derived bound (sum_bound): n terms t added in fp32 in any order and stored as bf16 once lie within
  bf16_ulp(|ref| + E) / 2 + E of the float64 sum, E = n 2^-24 sum|t|.
"""
import numpy as np

F64 = np.float64
F32 = np.float32
MI_EINVAL = -1
EW_CAP = 4096                    # ew_blocks(): blocks of 256 threads, one 8-channel item per thread and trip
SCALE_ROWS_CAP = 2048
SPP_T = 512                      # threads of an SPP plane block = pixels per round
SPP_KS = (5, 9, 13)
BF16_MAX = float.fromhex("0x1.fep127")
BF16_MIN_NORMAL = 2.0 ** -126
BF16_SUBNORMAL = 3 * 2.0 ** -133
GRAD_MAX = 64


# ------------------------------------------------------------------------------------------------------------ bfloat16
def round_bf16(a):
    """float64 -> the nearest bf16 (8 significant bits, exponent range of fp32; one rounding, ties to even), as float64"""
    a = np.asarray(a, dtype=F64)
    with np.errstate(invalid="ignore", over="ignore"):
        m, e = np.frexp(a)                              # |m| in [0.5, 1)
        out = np.ldexp(np.rint(m * 256.0), e - 8)       # np.rint: ties to even
        sub = np.abs(a) < BF16_MIN_NORMAL
        out = np.where(sub, np.rint(a * 2.0 ** 133) * 2.0 ** -133, out)
        out = np.where(np.abs(out) > BF16_MAX, np.copysign(np.inf, a), out)
    return np.where(np.isfinite(a), out, a)


def bf16_ulp(a):
    """spacing of the bf16 grid in the binade of |a|"""
    a = np.abs(np.asarray(a, dtype=F64))
    _, e = np.frexp(np.maximum(a, BF16_MIN_NORMAL))
    return np.ldexp(1.0, e - 8)


def is_bf16(a):
    a = np.asarray(a, dtype=F64)
    return bool(np.array_equal(round_bf16(a), a, equal_nan=True))


def sum_bound(ref, nterms, abs_sum):
    """|device - ref| allowed for a bf16 store of an fp32 sum of `nterms` terms whose magnitudes add up to abs_sum"""
    E = np.asarray(nterms, dtype=F64) * 2.0 ** -24 * np.asarray(abs_sum, dtype=F64)
    return bf16_ulp(np.abs(ref) + E) / 2 + E


# ------------------------------------------------------------------------------------------------------------- pooling
def pool_out(H, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1


def _span(H, Ho, w, stride, pad):
    """outputs o in [0, Ho) whose window cell w is in bounds: 0 <= o * stride - pad + w < H"""
    lo = max(0, -((w - pad) // stride))
    hi = min(Ho - 1, (H - 1 + pad - w) // stride)
    return lo, hi


def maxpool_first(x, k, stride, pad):
    """-> values [N][Ho][Wo][C] and pos = wy * k + wx of the first maximum in row-major order (strict > while scanning the
    window, cells outside the plane skipped).  Vectorised over the outputs, the scan over the k * k cells is the loop."""
    x = np.asarray(x)
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H, k, stride, pad), pool_out(W, k, stride, pad)
    vals = np.full((N, Ho, Wo, C), -np.inf, dtype=x.dtype)
    pos = np.full((N, Ho, Wo, C), -1, dtype=np.int16)
    for wy in range(k):
        y0, y1 = _span(H, Ho, wy, stride, pad)
        if y1 < y0:
            continue
        for wx in range(k):
            x0, x1 = _span(W, Wo, wx, stride, pad)
            if x1 < x0:
                continue
            cand = x[:, y0 * stride - pad + wy:y1 * stride - pad + wy + 1:stride, x0 * stride - pad + wx:x1 * stride - pad + wx + 1:stride]
            v, p = vals[:, y0:y1 + 1, x0:x1 + 1], pos[:, y0:y1 + 1, x0:x1 + 1]
            m = cand > v
            np.copyto(v, cand, where=m)
            np.copyto(p, np.int16(wy * k + wx), where=m)
    assert int(pos.min()) >= 0, "a window without a finite cell is outside the contract"
    return vals, pos


def maxpool_first_windows(x, k, stride, pad):
    """the same rule, stated independently: np.argmax (first occurrence) over the -inf-padded windows"""
    x = np.asarray(x, dtype=F64)
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)), constant_values=-np.inf)
    win = np.lib.stride_tricks.sliding_window_view(xp, (k, k), axis=(1, 2))[:, ::stride, ::stride]
    win = win.reshape(win.shape[:4] + (k * k,))
    pos = np.argmax(win, axis=-1)
    return np.take_along_axis(win, pos[..., None], -1)[..., 0], pos.astype(np.int16)


def maxpool_bwd(pos, g, k, stride, pad, H, W):
    """scatter-add in float64: output (n, oy, ox, c) adds g to input (oy * stride - pad + pos // k, ox * stride - pad + pos % k)"""
    N, Ho, Wo, C = pos.shape
    p = pos.astype(np.int64)
    n = np.arange(N, dtype=np.int64).reshape(N, 1, 1, 1)
    iy = np.arange(Ho, dtype=np.int64).reshape(1, Ho, 1, 1) * stride - pad + p // k
    ix = np.arange(Wo, dtype=np.int64).reshape(1, 1, Wo, 1) * stride - pad + p % k
    assert int(iy.min()) >= 0 and int(iy.max()) < H and int(ix.min()) >= 0 and int(ix.max()) < W
    flat = ((n * H + iy) * W + ix) * C + np.arange(C, dtype=np.int64)
    dx = np.zeros(N * H * W * C, dtype=F64)
    np.add.at(dx, flat.reshape(-1), np.asarray(g, dtype=F64).reshape(-1))
    return dx.reshape(N, H, W, C)


def maxpool_code(pos):
    """what mi_maxpool3x3s2_fwd_idx stores per output element: the byte dy * 3 + dx (0 .. 8)"""
    assert int(pos.min()) >= 0 and int(pos.max()) <= 8
    return pos.astype(np.uint8)


def spp_fwd(x):
    """-> [(values, pos)] for k = 5, 9, 13 at stride 1, `same` padding.  The layout of the device's index planes is private
    to its forward / backward pair and is not modelled: the backward is what shows which element a window chose."""
    return [maxpool_first(x, k, 1, k // 2) for k in SPP_KS]


def spp_bwd(poss, gs, prior=None, weight=lambda g: g):
    """float64 sum of the three pools' scatter-adds (+ prior); `weight` maps each g first (np.abs, np.ones_like)"""
    N, H, W, C = poss[0].shape
    dx = np.zeros((N, H, W, C), dtype=F64) if prior is None else weight(np.asarray(prior, dtype=F64)).copy()
    for k, pos, g in zip(SPP_KS, poss, gs):
        dx += maxpool_bwd(pos, weight(np.asarray(g, dtype=F64)), k, 1, k // 2, H, W)
    return dx


def upsample2x(x):
    return np.repeat(np.repeat(np.asarray(x), 2, axis=1), 2, axis=2)


def upsample2x_bwd(g):
    g = np.asarray(g)
    N, H2, W2, C = g.shape
    return g.reshape(N, H2 // 2, 2, W2 // 2, 2, C).sum(axis=(2, 4), dtype=F64)


def scale_rows(g, sc):
    """one fp32 multiply is correctly rounded and the float64 product of two fp32 values is exact: fl32 of it, for any values"""
    g, sc = np.asarray(g, dtype=F32).astype(F64), np.asarray(sc, dtype=F32).astype(F64)
    return (g * sc.reshape(-1, 1)).astype(F32)


def copy_acc(a, b):
    """bf16(fl32(a + b)): two correctly rounded IEEE operations (a, b bf16 values)"""
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.asarray(a, dtype=F64).astype(F32) + np.asarray(b, dtype=F64).astype(F32)
    return round_bf16(s.astype(F64))


# ----------------------------------------------------------------------------------------------------------------- SGD
def sgd_step(p, g, m, segs, momentum, grad_scale, first_step, trace=None):
    """torch.optim.SGD (dampening 0, no nesterov) in float64 over a segment table [(offset, count, weight_decay, lr)]:
    d = g * grad_scale + wd * p; buf = d on the first step, else momentum * buf + d; p -= lr * buf.  Elements outside the
    segments keep their values.  -> p, m (copies); every intermediate is appended to `trace`."""
    p, m = np.array(p, dtype=F64), np.array(m, dtype=F64)
    g = np.asarray(g, dtype=F64)
    for off, cnt, wd, lr in segs:
        s = slice(off, off + cnt)
        gs, wp = g[s] * grad_scale, wd * p[s]
        d = gs + wp
        mb = None if first_step else momentum * m[s]
        buf = d if first_step else mb + d
        lb = lr * buf
        m[s] = buf
        p[s] = p[s] - lb
        if trace is not None:
            trace += [gs, wp, d, buf, lb, p[s].copy()] + ([] if mb is None else [mb])
    return p, m


def fits_f32(a):
    a = np.asarray(a, dtype=F64)
    return bool(np.array_equal(a.astype(F32).astype(F64), a))


def sgd_family_ok(p, g, m, segs, momentum, grad_scale, first_step):
    """every intermediate of this step (products, d, buf, p) is its own fp32 rounding"""
    trace = []
    sgd_step(p, g, m, segs, momentum, grad_scale, first_step, trace)
    return all(fits_f32(t) for t in trace)


SGD_MOMENTUM, SGD_GRAD_SCALE = 2.0 ** -1, 2.0 ** -2
SGD_LR_WD = ((2.0 ** -3, 2.0 ** -4), (2.0 ** -2, 2.0 ** -5))
# offset, count, index into SGD_LR_WD: a float4-only segment of 4096 vectors (`two` always on); 300 vectors + 3 tail elements
# (`two` on for lanes < 44, off above); 3 elements (tail only); an offset = 2 mod 4 (scalar-only); an empty segment
SGD_SEGS = ((0, 16384, 0), (16392, 1203, 1), (17600, 3, 0), (17610, 1030, 1), (18648, 0, 0))
SGD_ARENA = 18656


def sgd_segs():
    return [(o, c, SGD_LR_WD[k][1], SGD_LR_WD[k][0]) for o, c, k in SGD_SEGS]


def sgd_owned(n=SGD_ARENA):
    own = np.zeros(n, dtype=bool)
    for o, c, _ in SGD_SEGS:
        assert not own[o:o + c].any() and o + c <= n
        own[o:o + c] = True
    return own


def sgd_operands(seed, n=SGD_ARENA):
    """p, g, m: multiples of 2^-6 in [-4, 4]"""
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(-256, 257, n).astype(F64) / 64 for _ in range(3))


def sgd_labels(off, cnt):
    """the branches of sgd_kernel that a segment reaches, from its offset and count"""
    out = set()
    n4 = cnt // 4 if off % 4 == 0 else 0
    if n4 and cnt % 4 == 0:
        out.add("sgd:float4_only")
    if n4 * 4 < cnt:
        out.add("sgd:tail" if off % 4 == 0 else "sgd:scalar_only")
    for i0 in range(0, n4, 512):                        # trip of lane t handles vector i0 + t; `two` = i0 + t + 256 < n4
        lanes = np.arange(i0, min(i0 + 256, n4))
        out |= {"sgd:two_on"} if (lanes + 256 < n4).any() else set()
        out |= {"sgd:two_off"} if (lanes + 256 >= n4).any() else set()
    return out


# ------------------------------------------------------------------------------------------------------------- families
FAMILIES = ("silu", "levels", "const", "rows", "cols", "planes")


def family(name, shape, seed):
    """bf16-representable finite inputs [N][H][W][C]:
    silu    SiLU(randn) rounded to bf16: the real distribution, with its natural ties
    levels  {-1, 0, 1}: every window ties many times
    const   a constant plane (one value per image and channel): the first maximum is the first in-bounds cell
    rows    constant along each row, a random integer per row; cols: its transpose - the horizontal and the vertical rule apart
    planes  plane j = n * C + c holds {j, j + 1/2} - N * C / 2: the value ranges of two planes are disjoint, so a plane
            handled for the wrong (n, c) cannot pass"""
    N, H, W, C = shape
    rng = np.random.default_rng(seed)
    if name == "silu":
        z = rng.standard_normal(shape)
        x = round_bf16(z / (1 + np.exp(-z)))
    elif name == "levels":
        x = rng.integers(-1, 2, shape).astype(F64)
    elif name == "const":
        x = np.broadcast_to(rng.integers(-3, 4, (N, 1, 1, C)).astype(F64), shape).copy()
    elif name == "rows":
        x = np.broadcast_to(rng.integers(-2, 3, (N, H, 1, C)).astype(F64), shape).copy()
    elif name == "cols":
        x = np.broadcast_to(rng.integers(-2, 3, (N, 1, W, C)).astype(F64), shape).copy()
    else:
        assert name == "planes" and N * C <= 128
        j = (np.arange(N).reshape(N, 1, 1, 1) * C + np.arange(C)).astype(F64) - (N * C) // 2
        x = j + rng.integers(0, 2, shape) / 2
    assert is_bf16(x) and np.isfinite(x).all()
    return x


def levels_f32(shape, seed):
    """family `levels` as float32 without a float64 copy: the second-trip shapes are tens of megabytes"""
    return np.random.default_rng(seed).integers(-1, 2, shape, dtype=np.int8).astype(F32)


def grads(shape, seed, dtype=F64):
    """the gradient family: integers in [-GRAD_MAX, GRAD_MAX]"""
    return np.random.default_rng(seed).integers(-GRAD_MAX, GRAD_MAX + 1, shape, dtype=np.int8).astype(dtype)


def grad_family_ok(abs_sum, *operands):
    """operands (the dy's and the prior dx) are integers and bf16 values, and the magnitudes that meet in one input pixel
    (abs_sum: the reference backward of |dy| on |prior|) stay below 2^24: every fp32 partial sum is exact in any order"""
    for a in operands:
        a = np.asarray(a)
        if not (np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 256):      # every integer up to 256 is a bf16 value
            return False
    return bool(np.max(abs_sum) < 2.0 ** 24)


def specials(n, seed):
    """n bf16 values for a bit copy: random ones with +-0, +-inf, the largest and the smallest normal and a subnormal set in"""
    x = round_bf16(np.random.default_rng(seed).standard_normal(n) * 8)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, BF16_MAX, -BF16_MAX, BF16_MIN_NORMAL, -BF16_MIN_NORMAL, BF16_SUBNORMAL, -BF16_SUBNORMAL])
    k = np.arange(sp.size) * 7 % n if n >= sp.size else np.arange(n)
    x[k] = sp[:k.size]
    return x


def acc_pairs(n, seed):
    """(a, b) bf16 operands of an fp32 add: random binades up to 40 apart (a difference above 16 loses the small operand
    twice, above 24 even in fp32), sums that tie on the bf16 grid, cancellation, +-inf and the overflow of BF16_MAX twice"""
    rng = np.random.default_rng(seed)
    a = round_bf16(rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-20, 21, n)))
    b = round_bf16(rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-20, 21, n)))
    ed = [(256.0, 1.0), (258.0, 1.0), (1.0, 2.0 ** -9), (1.0 + 2.0 ** -7, 2.0 ** -8), (3.0, -3.0), (1.0, 2.0 ** -30), (2.0 ** 20, -2.0 ** -3),
          (np.inf, 1.0), (-np.inf, 5.0), (BF16_MAX, BF16_MAX), (-BF16_MAX, -BF16_MAX), (BF16_MAX, 2.0 ** 119), (0.0, -0.0)]
    for i, (u, v) in enumerate(ed[:n]):
        k = i * 5 % n
        a[k], b[k] = u, v
    assert is_bf16(a) and is_bf16(b)
    return a, b


# --------------------------------------------------------------------------------------------------------------- labels
def trips(items, cap=EW_CAP):
    """loop trips of the busiest thread of a grid-stride kernel launched on min(cap, ceil(items / 256)) blocks of 256"""
    blocks = max(1, min(cap, -(-items // 256)))
    return -(-items // (blocks * 256))


def spp_remap(G):
    """the block -> (image, channel group) map of the SPP kernels on a grid of G blocks -> label, map"""
    if G % 8:
        return "off", list(range(G))
    lb = [(b % 8) * (G // 8) + b // 8 for b in range(G)]
    assert sorted(lb) == list(range(G))
    return ("identity" if lb == list(range(G)) else "permuted"), lb


def spp_labels(N, H, W, C, bwd):
    k = "spp_bwd" if bwd else "spp_fwd"
    rounds = -(-H * W // SPP_T)
    assert bwd is False or rounds <= 2
    return {"%s:round%d" % (k, min(rounds, 3)), "%s:remap_%s" % (k, spp_remap(N * C // 8)[0])}


REQUIRED = (
    ["spp_fwd:round%d" % i for i in (1, 2, 3)] + ["spp_bwd:round%d" % i for i in (1, 2)]
    + ["%s:remap_%s" % (k, r) for k in ("spp_fwd", "spp_bwd") for r in ("identity", "permuted", "off")]
    + ["%s:acc%d" % (k, a) for k in ("spp_bwd", "maxpool_bwd", "maxpool_bwd_idx", "upsample_bwd", "copy") for a in (0, 1)]
    + ["%s:trip2" % k for k in ("copy", "upsample_fwd", "upsample_bwd", "maxpool_fwd", "maxpool_fwd_idx", "maxpool_bwd", "maxpool_bwd_idx", "scale_rows")]
    + ["scale_rows:float4", "scale_rows:scalar"]
    + ["sgd:float4_only", "sgd:tail", "sgd:scalar_only", "sgd:two_on", "sgd:two_off", "sgd:first_step", "sgd:later_step"])

# ---------------------------------------------------------------------------------------------------------------- cases
SPP_PLANES = ((7, 9), (1, 14), (14, 1), (3, 40), (19, 27), (32, 32))
SPP_NC = ((1, 64), (2, 64), (3, 24), (1, 8))           # grids of 8 (identity remap), 16 (permuted), 9 and 1 (off)


def spp_cases(plane):
    """(N, C, family, family) for a plane: the three remap classes on every plane, (1, 8) on every other one; the families
    rotate so that every plane meets all six and every remap class meets each of them on some plane"""
    i = SPP_PLANES.index(plane)
    ncs = SPP_NC[:3] + (SPP_NC[3:] if i % 2 == 0 else ())
    return [(N, C, FAMILIES[(i + 2 * j) % 6], FAMILIES[(i + 2 * j + 3) % 6]) for j, (N, C) in enumerate(ncs)]


MAXPOOL_SHAPES = ((2, 17, 22, 64), (1, 8, 8, 32), (1, 1, 1, 8), (1, 2, 3, 8), (3, 1, 9, 16))
UPSAMPLE_SHAPES = ((2, 6, 5, 32), (1, 1, 1, 8), (3, 7, 1, 24))
COPY_NPIX, COPY_CS = (1, 37, 4096), (8, 24, 64)
SCALE_ROWS_SHAPES = ((1, 4), (3, 5), (7, 36), (64, 27), (1, 1))
