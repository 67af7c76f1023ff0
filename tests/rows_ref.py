"""Plain references of the row-wise kernels of csrc/transformer_ops.hip (LayerNorm forward / backward with their fused
dropout forms, mi_dropout_bf16 / mi_dropout_add_bf16, mi_ew_bf16, mi_sigmoid_f32) and of the column sums of csrc/misc_ops.hip,
the operand families on which their fp32 arithmetic is EXACT, the derived bounds where it is not, and mutants.
tests/test_gpu_rows_exact.py compares the device with these bit for bit; tests/test_rows_ref.py pins them on the CPU.
Everything here is numpy float64 / integer arithmetic on the host; nothing is taken from the code under test.

The dropout RNG (csrc/common.h), as an integer model:
  rng_key(seed)      one splitmix64 round: z = seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019 (mod 2^64), two xor-shift-multiply
                     steps (30 / 0xBF58476D1CE4E5B9, 27 / 0x94D049BB133111EB), z ^ (z >> 31)
  rng32k(key, idx)   x = lo(idx) ^ lo(key) ^ hi(idx) ^ rot16(hi(idx)); the lowbias32 mixer (x ^= x >> 16, * 0x7feb352d,
                     x ^= x >> 15, * 0x846ca68b, x ^= x >> 16); the word is x ^ hi(key)
  drop_threshold(p)  (unsigned)((double)(float)p * 2^32), raised to 1 where p > 0 gave 0; an element is KEPT iff word >= thr
  the seed offset    (mi_dropout_seed_offset) is added to the seed, mod 2^64, BEFORE the key is formed
The high index word (idx >= 2^32) is pinned on the host only: no GPU test allocates 2^32 elements, so hi(idx) != 0 stays
untested on the device.  Both stages are bijections, so seed_with_word() can craft a seed for which a chosen element draws
exactly the threshold - the only place where `>=` and `>` differ - or the word 0, the only word that the `thr = 1` floor
drops at p = 2^-33 and that a threshold of 0 would keep.

The exact families (asserted on the reference of every case - assert_*_conditions - before anything is launched):
  LayerNorm forward: a row is m + a * s_c with s_c in {-3, -1, 1, 3} (family 0, equal counts: mean of s^2 = 5) or {-1, 1}
    (family 1), m = a * k with |k| <= 252, a a power of two, eps = 11 a^2 or 3 a^2 (one eps per launch: a is per case): the
    row sum E m, the deviations a s_c, their squares, var = 5 a^2 or a^2 and var + eps = 16 a^2 or 4 a^2 are exact in fp32
    in any order, the quotients by E are exact results of a correctly rounded division, rstd = 1 / (4 a) or 1 / (2 a) is a
    power of two that rsqrtf must hit within RSTD_ULPS, and y = s_c / 4 * gamma + beta (gamma in +-{0.5, 1, 2}, beta a small
    integer) has at most 7 significant bits, so that moving rstd by RSTD_ULPS ulps cannot change bf16(y) (asserted).
  fused forward: d = dropout(x) from the host model, res = t - d with t a family row (a = 2^-7, |t| < 1/2) and |d| in [1, 1.4):
    res is a bf16 value and fp32(res) + fp32(d) = t exactly, so sum_out = t whatever the mask.
  LayerNorm backward: mean a multiple of 1/2, x - mean a multiple of 1/2 within +-2, rstd in {1, 2}, dy an integer within +-2,
    gamma in +-{0.5, 1, 2}, E a power of two: every intermediate is a multiple of 1 / UNIT (UNIT = 16 E) below 2^24 / UNIT.
  column sums: small integers, different per pixel and channel; sums and sums of squares below 2^24.
"""
import types

import numpy as np
import torch

import bn_ref as BN

F64 = np.float64
F32 = np.float32
U32 = 2.0 ** -24                # fp32 unit roundoff
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
MI_EINVAL = -1

# ---- measured constants (tests/test_gpu_rows_exact.py prints each figure before it asserts; profiles/rows_exact_pytest_gpu.txt)
# rsqrtf on the exact forward families (arguments 4^k): worst distance from the float64 rstd measured on an MI355X: 0 ulps.
# The cap is measured + 1 ulp, because another ROCm release may expand rsqrtf differently; it may never exceed 4.
RSTD_ULPS = 1
# mi_sigmoid_f32 forward, 1 / (1 + expf(-x)) with the accurate expf: worst distance of the device's fp32 value from the
# float64 sigmoid over sigmoid_f32_args(), in fp32 ulps of the reference's binade, measured on an MI355X: 2.282 (in the
# negative tail near x = -16.7, where e = 2^24: half an ulp at the bottom of e's binade is a whole ulp at the top of the
# quotient's, so even three correctly rounded operations reach 2.22 there - tests/test_rows_ref.py).  The cap is the
# measured figure + 1 ulp, for the same reason as RSTD_ULPS; it is a distance, so it need not be a whole number.
SIGMOID_F32_MEASURED = 2.282
SIGMOID_F32_ULPS = SIGMOID_F32_MEASURED + 1
# mi_ew_bf16 ops 3 .. 6 (__expf): the bf16 store hides the fp32 error (half a bf16 ulp is 2^15 fp32 ulps), so what can be
# measured is |device - float64| / bound with bound = half a bf16 ulp + the DERIVED fp32 error of tests/bn_ref.py (sig_rel:
# v_exp_f32 within 1 ulp, the argument scaling 2 |x| u, one rounding of 1 + e, the quotient within 1 ulp).  Measured worst
# ratio over every finite bf16 argument (ops 3, 5) and over the grids (ops 4, 6): 1.000 each - reached where the
# reference lies next to a bf16 tie and never exceeded, which is what a correct kernel shows; the fp32 term matters only
# there.  No margin is added to a derived bound.
assert RSTD_ULPS <= 4


def bf16_rne(x):
    """float64 array -> nearest bf16 (one rounding, ties to even), as float64"""
    return BN.bf16_rne(torch.from_numpy(np.ascontiguousarray(x, dtype=F64))).numpy()


def bf16_half_ulp(x):
    return BN.bf16_half_ulp(torch.from_numpy(np.ascontiguousarray(x, dtype=F64))).numpy()


def f32(x):
    return np.asarray(x, dtype=F64).astype(F32).astype(F64)


def ulps32(got, ref):
    """distance in fp32 ulps (of the float64 reference's binade) between fp32 values `got` and float64 `ref` (> 0)"""
    ref = np.asarray(ref, dtype=F64)
    _, e = np.frexp(ref)
    return np.abs(np.asarray(got, dtype=F64) - ref) / np.ldexp(1.0, np.maximum(e, -125) - 24)


# ------------------------------------------------------------------------------------------------------------ the RNG
def rng_key(seed):
    z = (seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def rng32k(key, idx):
    """idx: array of uint64 element indices -> uint32 words"""
    idx = np.asarray(idx, dtype=np.uint64)
    hi = (idx >> np.uint64(32)).astype(np.uint32)
    x = idx.astype(np.uint32) ^ np.uint32(key & M32) ^ hi ^ ((hi << np.uint32(16)) | (hi >> np.uint32(16)))
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    x = x ^ (x >> np.uint32(16))
    return x ^ np.uint32(key >> 32)


def drop_threshold(p, floor=True):
    p = float(F32(p))
    thr = int(p * 4294967296.0) if p > 0 else 0
    return 1 if floor and p > 0 and thr == 0 else thr


def drop_scale(p):
    """1.f / (1.f - p): fp32"""
    return F32(1.0) / (F32(1.0) - F32(p))


def keep_mask(seed, offset, idx, p, mutant=None):
    """True where element idx is kept: word(seed + offset mod 2^64, idx) >= thr"""
    if mutant == "offset_after_key":
        key = (rng_key(seed & M64) + (offset or 0)) & M64
    else:
        key = rng_key((seed + (offset or 0)) & M64)
    w = rng32k(key, idx).astype(np.uint64)
    thr = np.uint64(drop_threshold(p, floor=mutant != "thr_floor_missing"))
    return w > thr if mutant == "keep_gt" else w >= thr


def _unxorshift(z, s):
    r = z
    for _ in range(64 // s + 1):
        r = z ^ (r >> s)
    return r


def seed_with_word(idx, word, key_hi=0x5bd1e995):
    """a seed whose key gives element idx (< 2^32) exactly `word`: both hash stages inverted"""
    x = (word ^ key_hi) & M32
    x ^= x >> 16
    x = (x * pow(0x846ca68b, -1, 1 << 32)) & M32
    x ^= (x >> 15) ^ (x >> 30)
    x = (x * pow(0x7feb352d, -1, 1 << 32)) & M32
    x ^= x >> 16
    key = (key_hi << 32) | (x ^ idx)
    z = _unxorshift(key, 31)
    z = (z * pow(0x94D049BB133111EB, -1, 1 << 64)) & M64
    z = _unxorshift(z, 27)
    z = (z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & M64
    z = _unxorshift(z, 30)
    return ((z - 0x632BE59BD9B4E019) * pow(0x9E3779B97F4A7C15, -1, 1 << 64)) & M64


def dropped(x, keep, p):
    """bf16(fp32(x) * fp32(1 / (1 - p))) where kept, +0 elsewhere: x float64 holding bf16 values"""
    prod = (np.asarray(x, dtype=F64).astype(F32) * drop_scale(p)).astype(F64)       # one IEEE fp32 multiply
    return np.where(keep, bf16_rne(prod), 0.0)


def dropout_ref(x, res, p, seed, offset=None, mutant=None):
    """mi_dropout_bf16 (res None) / mi_dropout_add_bf16 over a flat array: element i draws index i"""
    n = x.size
    d = dropped(x, keep_mask(seed, offset, np.arange(n, dtype=np.uint64), p, mutant), p)
    return d if res is None else bf16_rne(f32(res) + d)                            # the second rounding


FLOOR_P = 2.0 ** -33            # (unsigned)(p 2^32) = 0: the `thr = 1` floor; fp32(1 / (1 - p)) = 1
DROP_PS = (0.5, 0.1, FLOOR_P, 0.0)
DROP_NS = (8, 8 * 255, 8 * 257, 8 * 256 * 4096 + 8 * 300)      # the last: the grid-stride loop of dropout_kernel runs
SEED = 0x1234_5678_9ABC_DEF1
OFFSETS = (0, 7, M64)


def bf16_pool(n, seed, lo=-8, hi=8):
    """n bf16 values (float64) with full 8-bit significands over the binades 2^lo .. 2^hi, both signs"""
    g = np.random.default_rng(seed)
    return bf16_rne(g.choice([-1.0, 1.0], n) * (1 + g.integers(0, 128, n) / 128.0) * np.ldexp(1.0, g.integers(lo, hi, n)))


# ------------------------------------------------------------------------------------------------------ LayerNorm
def ln_fwd(x, gamma, beta, eps):
    """textbook LayerNorm, biased variance, float64: -> y, mean, rstd"""
    x = np.asarray(x, dtype=F64)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + float(F32(eps)))
    return (x - mean[:, None]) * rstd[:, None] * gamma[None, :] + beta[None, :], mean, rstd


def ln_bwd(x, dy, gamma, mean, rstd, parts=False):
    """-> dx, dgamma, dbeta (float64, unrounded) from given mean / rstd"""
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma[None, :]
    s1, s2 = g.mean(1), (g * xh).mean(1)
    dx = rstd[:, None] * (g - s1[:, None] - xh * s2[:, None])
    out = (dx, (dy * xh).sum(0), dy.sum(0))
    return out + (types.SimpleNamespace(xh=xh, g=g, s1=s1, s2=s2),) if parts else out


FWD_ES = tuple(range(64, 1025, 64))
FWD_TS = (1, 3, 4, 5, 37)
BWD_ES = (64, 128, 256, 512, 1024)
# T -> (blocks, rows in the last block) at 16 rows per block; 8193 rows at E = 64 make rows_per_block 20
BWD_TS = {1: (1, 1), 128: (8, 16), 143: (9, 15), 385: (25, 1), 512: (32, 16), 527: (33, 15), 625: (40, 1)}
BWD_T_LONG = 8193


def bwd_rows_per_block(T):
    rpb = -(-(-(-T // 512)) // 4) * 4
    return max(rpb, 16)


def bwd_cases():
    out = [(E, T) for E in BWD_ES for T in BWD_TS]
    return out + [(64, BWD_T_LONG)]


def ln_params(E, seed):
    g = np.random.default_rng(seed)
    gamma = g.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], E)
    beta = 2.0 * g.integers(-2, 3, E)           # even: y = +-gamma / 2 + beta of family 1 never cancels to 0
    return gamma, beta


def fwd_exact_case(T, E, family, seed, a_exp=None, kmax=252):
    """rows m + a s_c: -> namespace(x, gamma, beta, eps, y, mean, rstd)"""
    g = np.random.default_rng(seed)
    vals = np.array([-3.0, -1.0, 1.0, 3.0] if family == 0 else [-1.0, 1.0])
    a = 2.0 ** (int(g.integers(-6, 5)) if a_exp is None else a_exp)
    s = np.stack([g.permutation(np.tile(vals, E // len(vals))) for _ in range(T)])
    m = a * g.integers(-kmax, kmax + 1, T).astype(F64)
    gamma, beta = ln_params(E, seed + 1)
    x = m[:, None] + a * s
    eps = (11.0 if family == 0 else 3.0) * a * a
    y, mean, rstd = ln_fwd(x, gamma, beta, eps)
    return types.SimpleNamespace(T=T, E=E, a=a, x=x, gamma=gamma, beta=beta, eps=eps, y=y, mean=mean, rstd=rstd, family=family)


def assert_fwd_conditions(o):
    """what makes the forward exact (module docstring), on the float64 reference of one case"""
    assert np.array_equal(bf16_rne(o.x), o.x), "x is not on the bf16 grid"
    assert float(F32(o.eps)) == o.eps
    assert np.array_equal(f32(o.x.sum(1)), o.x.sum(1)) and np.all(np.abs(o.x).sum(1) / o.a < 2 ** 24)
    assert np.array_equal(o.mean * o.E, o.x.sum(1)) and np.array_equal(f32(o.mean), o.mean)
    d = o.x - o.mean[:, None]
    q = (d * d).sum(1)
    assert np.all(q / (o.a * o.a) < 2 ** 24) and np.array_equal(f32(q / o.E + o.eps), q / o.E + o.eps)
    v = q / o.E + o.eps
    mant, _ = np.frexp(v / 4 ** np.round(np.log2(v) / 2))
    assert np.all(mant == 0.5), "var + eps is not a power of four"
    assert np.array_equal(np.frexp(o.rstd)[0], np.full(o.T, 0.5)), "rstd is not a power of two"
    yb = bf16_rne(o.y)
    assert np.array_equal(yb, o.y), "y needs no rounding in this family"
    for sgn in (-1, 1):                                    # rstd off by RSTD_ULPS ulps, then every fp32 rounding against us
        r = o.rstd * (1 + sgn * RSTD_ULPS * 2.0 ** -23)
        y2 = d * r[:, None] * o.gamma[None, :] + o.beta[None, :]
        y2 = y2 + sgn * 4 * U32 * (np.abs(y2) + np.abs(o.beta[None, :]))
        assert np.array_equal(bf16_rne(y2), yb), "bf16(y) depends on the last bits of rstd"


def fused_fwd_case(T, E, family, p, seed, offset=None, mutant=None):
    """x, res with res + dropout(x) = t, t a family row (a = 2^-7, |t| < 1/2): -> forward case with x, res, t"""
    o = fwd_exact_case(T, E, family, seed, a_exp=-7, kmax=60)
    g = np.random.default_rng(seed + 2)
    xs = {0.5: 0.5, 0.1: 1.0, FLOOR_P: 1.0}[p]            # |x| in [xs, 1.25 xs): |d| in [1, 1.4) on the 2^-7 grid
    xin = g.choice([-1.0, 1.0], (T, E)) * (1 + g.integers(0, 32, (T, E)) / 128.0) * xs
    keep = keep_mask(seed, offset, np.arange(T * E, dtype=np.uint64), p, mutant).reshape(T, E)
    d = dropped(xin, keep, p)
    o.t, o.res, o.xin, o.d, o.keep, o.p, o.seed = o.x, o.x - d, xin, d, keep, p, seed
    return o


def assert_fused_conditions(o):
    assert_fwd_conditions(o)
    assert np.array_equal(bf16_rne(o.res), o.res), "res = t - d is not a bf16 value"
    assert np.array_equal(bf16_rne(o.xin), o.xin)
    assert np.array_equal(f32(f32(o.res) + o.d), o.t) and np.array_equal(bf16_rne(o.t), o.t)
    assert 0 < o.keep.mean() < 1 or o.T * o.E < 256


def bwd_exact_case(T, E, seed):
    g = np.random.default_rng(seed)
    mean = g.integers(-2, 3, T) / 2.0
    rstd = g.choice([1.0, 2.0], T)
    x = mean[:, None] + g.integers(-4, 5, (T, E)) / 2.0
    dy = g.integers(-2, 3, (T, E)).astype(F64)
    gamma = g.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], E)
    dx, dgamma, dbeta, parts = ln_bwd(x, dy, gamma, mean, rstd, parts=True)
    return types.SimpleNamespace(T=T, E=E, x=x, dy=dy, gamma=gamma, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta,
                                 parts=parts, seed=seed)


def assert_bwd_conditions(o):
    unit = 16.0 * o.E
    assert o.E & (o.E - 1) == 0
    p = o.parts
    for name, v in (("x", o.x), ("dy", o.dy), ("xh", p.xh), ("g", p.g), ("g xh", p.g * p.xh), ("s1", p.s1), ("s2", p.s2),
                    ("xh s2", p.xh * p.s2[:, None]), ("g - s1", p.g - p.s1[:, None]), ("dx", o.dx), ("dy xh", o.dy * p.xh)):
        assert np.array_equal(np.round(v * unit), v * unit) and np.all(np.abs(v) * unit < 2 ** 24), name
    # every partial sum, in any order: below 2^24 units of the terms' own grid
    assert np.all(np.abs(p.g * p.xh).sum(1) * 4 < 2 ** 24) and np.all(np.abs(p.g).sum(1) * 2 < 2 ** 24)
    assert np.abs(o.dy * p.xh).sum(0).max() * 2 < 2 ** 24 and np.abs(o.dy).sum(0).max() < 2 ** 24
    assert np.array_equal(bf16_rne(o.x), o.x)
    assert not np.array_equal(bf16_rne(o.dx), o.dx) or o.T * o.E <= 64 * 16, "dx should need its rounding"


def emulate_ln_bwd(o, p=0.0, offset=None, mutant=None):
    """the launch structure of mi_layernorm_bwd_dropout on the host (float64 on an exact family: the values of fp32):
    blocks of rows_per_block rows, a lane owning PER = E / 64 consecutive channels, block partials, the two loops of the
    parameter kernel.  -> dx (bf16), dx_drop (bf16), dgamma, dbeta, nblk"""
    T, E = o.T, o.E
    rpb = bwd_rows_per_block(T)
    nblk = -(-T // rpb)
    mean = np.roll(o.mean, -1) if mutant == "mean_wrong_row" else o.mean
    xh = (o.x - mean[:, None]) * o.rstd[:, None]
    g = o.dy * o.gamma[None, :]
    s1 = g.sum(1) / E
    s2 = (g * xh).sum(1) / (1 if mutant == "s2_no_1_over_E" else E)
    dx = bf16_rne(o.rstd[:, None] * (g - s1[:, None] - xh * s2[:, None]))
    PER = E // 64
    c = np.arange(E)
    col = (c // PER) + 64 * (c % PER) if mutant == "fwd_lane_map" else c      # lane = c / PER, j = c % PER -> lane + 64 j
    idx = (np.arange(T, dtype=np.uint64)[:, None] * np.uint64(E) + col[None, :].astype(np.uint64))
    dx_drop = dropped(dx, keep_mask(o.seed, offset, idx, p, mutant), p)
    part = np.zeros((nblk, E, 2))
    for b in range(nblk):
        r1 = min(T, (b + 1) * rpb) - (1 if mutant == "dgamma_last_row" else 0)
        rows = slice(b * rpb, r1)
        part[b, :, 0] = (o.dy[rows] * xh[rows]).sum(0)
        part[b, :, 1] = o.dy[rows].sum(0)
    acc = np.zeros((E, 2))
    for grp in range(8):
        k = grp
        while k + 24 < nblk:
            acc += part[k] + part[k + 8] + part[k + 16] + part[k + 24]
            k += 32
        if mutant == "skip_unroll_boundary" and k < nblk:
            k += 8
        while k < nblk:
            acc += part[k]
            k += 8
    return types.SimpleNamespace(dx=dx, dx_drop=dx_drop, dgamma=acc[:, 0], dbeta=acc[:, 1], nblk=nblk)


# ---- real statistics: Gaussian rows, elementwise bounds (first order, u = 2^-24; a sum of n fp32 terms in any order is
# within (n - 1) u sum |terms|; HI covers the higher orders for n u <= 2^-10)
HI = 1 + 2.0 ** -9


def real_case(T, E, seed):
    g = np.random.default_rng(seed)
    x = bf16_rne(g.standard_normal((T, E)) * 2 + 0.5)
    dy = bf16_rne(g.standard_normal((T, E)))
    gamma = f32(1 + 0.1 * g.standard_normal(E))
    beta = f32(0.1 * g.standard_normal(E))
    return types.SimpleNamespace(T=T, E=E, x=x, dy=dy, gamma=gamma, beta=beta, eps=1e-5)


def real_fwd_bounds(o):
    """-> reference (y, mean, rstd) and bounds (y, mean, rstd) on |device - reference|"""
    E, u = o.E, U32
    y, mean, rstd = ln_fwd(o.x, o.gamma, o.beta, o.eps)
    b_mean = E * u * np.abs(o.x).mean(1) + u * np.abs(mean)                   # the sum, the division
    d = o.x - mean[:, None]
    e_d = b_mean[:, None] + u * np.abs(d)                                     # d computed from the device's mean, rounded
    var = (d * d).mean(1)
    # d^2: 2 |d| e_d, rounded; the sum of E terms; the division and + eps round
    b_var = (2 * np.abs(d) * e_d + u * d * d).mean(1) + E * u * var + 2 * u * (var + o.eps)
    b_rstd = 0.5 * rstd * b_var / (var + o.eps) + RSTD_ULPS * 2 * u * rstd    # d rstd / d var, rsqrtf within RSTD_ULPS ulps
    ga = np.abs(o.gamma)[None, :]
    pre = ga * (rstd[:, None] * e_d + np.abs(d) * b_rstd[:, None]) + 3 * u * np.abs(d * rstd[:, None]) * ga + u * np.abs(y)
    pre = pre * HI
    b_y = pre + bf16_half_ulp(np.abs(y) + pre)
    return (y, mean, rstd), (b_y, b_mean * HI, b_rstd * HI)


def real_bwd_bounds(o, mean32, rstd32):
    """mean32 / rstd32: the fp32 statistics handed to the backward (float64 arrays of fp32 values): they are INPUTS, so
    the reference is taken at them and carries no statistics error"""
    E, T, u = o.E, o.T, U32
    dx, dgamma, dbeta, p = ln_bwd(o.x, o.dy, o.gamma, mean32, rstd32, parts=True)
    e_xh = 2 * u * np.abs(p.xh)
    b_s1 = (E + 1) * u * np.abs(p.g).mean(1)
    b_s2 = (E + 5) * u * np.abs(p.g * p.xh).mean(1)
    s1, s2 = np.abs(p.s1)[:, None], np.abs(p.s2)[:, None]
    inner = (u * np.abs(p.g) + b_s1[:, None] + np.abs(p.xh) * b_s2[:, None] + e_xh * s2 + u * np.abs(p.xh) * s2
             + 2 * u * (np.abs(p.g) + s1 + np.abs(p.xh) * s2))
    pre = (rstd32[:, None] * inner + u * np.abs(dx)) * HI
    b_dx = pre + bf16_half_ulp(np.abs(dx) + pre)
    b_dg = (T + 3) * u * np.abs(o.dy * p.xh).sum(0) * HI
    b_db = T * u * np.abs(o.dy).sum(0) * HI + 2.0 ** -149
    return (dx, dgamma, dbeta), (b_dx, b_dg, b_db)


def emulate_real_fp32(o, order, mean32, rstd32):
    """the forward and backward in fp32 on the host, sums in index order (order 0) or pairwise (order 1)"""
    def rsum(a, axis):
        a = a.astype(F32)
        if order == 0:
            return np.add.accumulate(a, axis=axis, dtype=F32).take(-1, axis=axis)
        a = np.moveaxis(a, axis, -1)
        while a.shape[-1] > 1:
            if a.shape[-1] % 2:
                a = np.concatenate([a, np.zeros(a.shape[:-1] + (1,), F32)], -1)
            a = a[..., 0::2] + a[..., 1::2]
        return a[..., 0]
    x, dy, gm, bt = (v.astype(F32) for v in (o.x, o.dy, o.gamma, o.beta))
    E = F32(o.E)
    mu = rsum(x, 1) / E
    d = x - mu[:, None]
    rs = (F32(1) / np.sqrt((rsum(d * d, 1) / E + F32(o.eps)).astype(F64))).astype(F32)
    y = bf16_rne((d * rs[:, None] * gm[None, :] + bt[None, :]).astype(F64))
    mb, rb = mean32.astype(F32), rstd32.astype(F32)          # the backward's statistics are its inputs
    xh = (x - mb[:, None]) * rb[:, None]
    g = dy * gm[None, :]
    s1, s2 = rsum(g, 1) / E, rsum(g * xh, 1) / E
    dx = bf16_rne((rb[:, None] * (g - s1[:, None] - xh * s2[:, None])).astype(F64))
    return types.SimpleNamespace(y=y, mean=mu.astype(F64), rstd=rs.astype(F64), dx=dx, dgamma=rsum(dy * xh, 0).astype(F64),
                                 dbeta=rsum(dy, 0).astype(F64))


def ratio(got, ref, bound):
    """worst |got - ref| / bound (NaN counts as infinite)"""
    r = np.abs(np.asarray(got, dtype=F64) - ref) / bound
    return float(np.where(np.isnan(r), np.inf, r).max())


# the criteria of tests/test_gpu_detr.py::test_layernorm_fwd_bwd_against_torch and of its column-sum tests
def old_ln_close(got, ref):
    return bool(np.all(np.abs(got - ref) <= 2e-2 + 2e-2 * np.abs(ref)))


def old_param_close(got, ref, T):
    return bool(np.all(np.abs(got - ref) <= 1e-3 * T ** 0.5 + 1e-3 * np.abs(ref)))


def old_keep_rate_ok(keep, p):
    """the dropout tests' criterion: the keep rate within 1 % (determinism and `the same mask in the backward` hold for
    any mask that is a function of (seed, index))"""
    return abs(float(np.asarray(keep).mean()) - (1 - p)) < 0.01


# ---------------------------------------------------------------------------------------------------- mi_ew_bf16
EW_NS = (8, 8 * 255, 8 * 257, 8 * 256 * 2048 + 8 * 300)       # the last: the grid-stride loop of ew_kernel runs
EW_UNARY = (1, 3, 5)
BF16_MAX = BN.BF16_MAX


def ew_edge_operands(n, seed):
    """n operand pairs (a, b) as float64 holding bf16 values: +-0, subnormals, the largest finite value, sums that overflow,
    sums that cancel to a tiny negative, and a random pool"""
    edge = np.array([0.0, -0.0, 2.0 ** -133, -2.0 ** -133, 2.0 ** -127, -2.0 ** -126, BF16_MAX, -BF16_MAX, 1.0, -1.0,
                     1 + 2.0 ** -7, -(1 + 2.0 ** -7), 255.0, 0.5 + 2.0 ** -8, 2.0 ** 127, -2.0 ** 127])
    g = np.random.default_rng(seed)
    a, b = np.meshgrid(edge, edge)
    a, b = a.ravel(), b.ravel()
    k = n - a.size
    if k < 0:
        sel = g.choice(a.size, n, replace=False)
        return a[sel], b[sel]
    return (np.concatenate([a, bf16_pool(k, seed, -10, 10)]), np.concatenate([b, bf16_pool(k, seed + 1, -10, 10)]))


def ew_exact(op, a, b, mutant=None):
    """ops 0, 1, 2, 7: one fp32 operation on bf16 values, rounded once (op 7: the sum is rounded, then relu)"""
    with np.errstate(over="ignore", invalid="ignore"):
        if op == 0:
            return bf16_rne(f32(a + b))                     # the IEEE fp32 sum (its own rounding), then the bf16 store
        if op == 1:
            return np.where(a > 0, a, 0.0)                  # fmaxf(x, 0): -0 and +0 compare equal; see relu_zero_ok
        if op == 2:
            return np.where(b > 0, a, 0.0)                  # NaN > 0 and -0 > 0 are false
        if op == 7:
            if mutant == "relu_add_rounded_once":
                return bf16_rne(np.where(f32(a + b) > 0, f32(a + b), 0.0))
            if mutant == "relu_before_add":
                return bf16_rne(np.where(a > 0, a, 0.0) + b)
            s = bf16_rne(f32(a + b))
            return np.where(s > 0, s, 0.0)
    raise ValueError(op)


def ew_bound(op, a, b=None):
    """ops 3 .. 6 -> (float64 reference, bound on |device - reference|): the fp32 value within the derived bound of
    tests/bn_ref.py (sig_rel: __expf = v_exp_f32 of a scaled argument, one rounding of 1 + e, a division within 1 ulp), its
    products rounded (u each), then the bf16 store: half a bf16 ulp at the perturbed value"""
    ta = torch.from_numpy(np.ascontiguousarray(a, dtype=F64))
    if op in (3, 5):
        s = torch.sigmoid(ta)
        if op == 3:
            ref, pre = s, s * BN.sig_rel(ta, s) + BN.FLOOR
        else:
            ref, pre = ta * s, BN.silu_bound(ta)
    else:
        tb = torch.from_numpy(np.ascontiguousarray(b, dtype=F64))
        if op == 4:                                         # dy * y * (1 - y): 1 - y exact or rounded, two products
            ref = ta * tb * (1 - tb)
            pre = ref.abs() * 3 * U32 + BN.FLOOR
        else:                                               # dy * silu'(x), a = dy, b = the forward INPUT
            s = torch.sigmoid(tb)
            gr = s * (1 + tb * (1 - s))
            ref = ta * gr
            pre = ta.abs() * BN.silu_grad_bound(tb) + ref.abs() * 2 * U32 + BN.FLOOR
    ref, pre = ref.numpy(), pre.numpy() * HI
    return ref, pre + bf16_half_ulp(np.abs(ref) + pre)


def all_finite_bf16():
    v = BN.all_finite_bf16().to(torch.float64).numpy()
    return v[: 65536 - 65536 % 8]


def ew_grid(op):
    """ops 4 / 6: a grid of dy times every finite bf16 second operand in a sensible range (op 4: y in [0, 1], a sigmoid
    output; op 6: |x| <= 128, beyond which silu' is 0 or 1 to the last bit)"""
    v = np.unique(all_finite_bf16())
    v = v[(v >= 0) & (v <= 1)] if op == 4 else v[np.abs(v) <= 128]
    dy = np.array([1.0, -1.0, 0.75, -2.5, 2.0 ** -20, 1 + 2.0 ** -7, 100.0, 0.0])
    a, b = np.meshgrid(dy, v)
    a, b = a.ravel(), b.ravel()
    k = -a.size % 8
    return np.concatenate([a, np.zeros(k)]), np.concatenate([b, np.zeros(k)])


SIG_NS = (1, 255, 257, 256 * 1024 + 300)


def sigmoid_f32_args():
    """fp32 arguments (as float64): a dense sweep of [-30, 30], +-0 and the ends of the range in which neither expf(-x) nor
    the quotient leaves the normal fp32 range (-87 .. 88)"""
    g = np.random.default_rng(11)
    return f32(np.concatenate([np.linspace(-30, 30, 200001), g.standard_normal(50000) * 4, [-0.0, 0.0, -87.0, 88.0]]))


def sigmoid_ref(x):
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(x, dtype=F64))).numpy()


def sigmoid_bwd_case(n, seed):
    """dyadic y in (0, 1) and dy: dy * y * (1 - y) exact in fp32 in any association"""
    g = np.random.default_rng(seed)
    y = g.integers(1, 64, n) / 64.0
    dy = g.integers(-32, 33, n) / 4.0
    return y, dy, dy * y * (1 - y)


# ---------------------------------------------------------------------------------------------------- column sums
COL_CS = (8, 60, 64, 72, 92, 2048, 4096, 4104)
COL_NPIX = (1, 255, 256, 257, 128 * 256 + 1)
COLSUM_MAX_CHUNKS = 64


def col_cp(C):
    return (C + 7) // 8 * 8


def col_blocks(npix, C, narrow):
    per = (256 // (col_cp(C) // 8)) * 8 if narrow else 256
    return max(1, min(128, -(-npix // per)))


def col_path(C, narrow):
    if narrow:
        return "colsum_stage1+2"
    return "colsum_wide_fused" if -(-col_cp(C) // 64) <= COLSUM_MAX_CHUNKS else "colsum_wide_stage1+2"


def col_values(npix, C, seed=0, device=None):
    """integers in [-5, 5], different per pixel and channel (a dropped, doubled or misplaced row changes a sum); float64
    numpy, or a float64 torch tensor made on `device`"""
    if device is None:
        p, c = np.arange(npix, dtype=np.int64)[:, None], np.arange(C, dtype=np.int64)[None, :]
        return (((p * 7 + c * 3 + (p // 11) * (c % 5) + seed) % 11) - 5).astype(F64)
    p, c = torch.arange(npix, device=device)[:, None], torch.arange(C, device=device)[None, :]
    return (((p * 7 + c * 3 + (p // 11) * (c % 5) + seed) % 11) - 5).to(torch.float64)


def col_ref(x, sq, out0=None):
    s = (x * x if sq else x).sum(0)
    return s if out0 is None else out0 + s


def assert_col_conditions(x, sq, out0=None):
    """x: numpy or torch float64 [npix][C]"""
    t = float((x * x if sq else abs(x)).sum(0).max()) + (0 if out0 is None else float(abs(out0).max()))
    assert t < 2 ** 24 and bool((x == x.round()).all())
    head = x[:8, :128]
    head = head.cpu().numpy() if torch.is_tensor(head) else head
    assert x.shape[1] < 8 or len({tuple(r) for r in head}) == len(head), "rows are not distinct"
    assert x.shape[1] < 128 or not np.array_equal(head[:, :64], head[:, 64:128]), "chunks are not distinct"


def emulate_colsum(x, C, sq, narrow, mutant=None):
    """the block structure of the column sums on the host (numpy [npix][C]): block b of nblk takes the pixels b PL + pl,
    stride nblk PL, and the final stage adds the partials [nblk][CP] of each 64-channel chunk at c0 = 64 * chunk"""
    npix = x.shape[0]
    nblk = col_blocks(npix, C, narrow)
    v = x * x if sq else x
    PL = 256 // (col_cp(C) // 8) if narrow else 32               # (the wide kernels: 32 pixel lanes for a full chunk)
    blk = (np.arange(npix) // PL) % nblk
    part = np.stack([v[blk == b].sum(0) for b in range(nblk)])
    out = np.zeros(C)
    for c0 in range(0, C, 64):
        w = min(64, C - c0)
        src = 0 if mutant == "wrong_c0" else c0
        out[c0:c0 + w] = part[:, src:src + w].sum(0)
    return out


MUTANTS = ("fwd_lane_map", "keep_gt", "offset_after_key", "dgamma_last_row", "s2_no_1_over_E", "mean_wrong_row",
           "skip_unroll_boundary", "wrong_c0", "relu_add_rounded_once",
           "thr_floor_missing")      # not in the issue's list: drop_threshold without its `thr = 1` floor (p = 2^-33 gives 0)

# ------------------------------------------------------------------------------------------------- coverage table
REQUIRED = (["layernorm_fwd_kernel<plain>", "layernorm_fwd_kernel<fused>"]
            + ["layernorm_bwd_kernel<%d>%s" % (p, d) for p in (1, 2, 4, 8, 16) for d in ("", "+dx_drop")]
            + ["layernorm_bwd_params_kernel", "dropout_kernel", "dropout_kernel+res", "mha_mask_kernel", "sigmoid_f32_kernel<fwd>",
               "sigmoid_f32_kernel<bwd>"]
            + ["ew_kernel<op%d>" % k for k in range(8)]
            + ["%s%s" % (path, s) for path in ("colsum_wide_fused", "colsum_wide_stage1+2") for s in ("", "<sq>")]
            + ["colsum_stage1+2"])
