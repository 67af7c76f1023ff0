"""Plain float64 reference of the BatchNorm(train) + SiLU (+ residual) ABI of csrc/bn_act.hip, as include/mi355_det.h states
it, and the operand families on which the kernels' fp32 arithmetic is EXACT (tests/test_gpu_bn_exact.py compares the device
with these bit for bit; tests/test_bn_ref.py pins them to torch's float64 batch_norm + silu autograd on the CPU).

The reference (torch float64, on whatever device the operands live on):
  slot_sums / fwd_prologue   the accumulator slots summed IN SLOT ORDER, mean, biased variance clamped at 0, invstd, scale,
                             shift; running mean / variance (momentum, unbiased factor count / (count - 1)); nbt + 1
  fwd_apply                  a = act(y * scale + shift) (+ res)
  bwd_sums                   (sum dz, sum dz * xhat), dz = da * act'(z), z = y * scale + shift, xhat = (y - mean) * invstd
  bwd_apply                  dy = gamma * invstd * (dz - c1 - xhat * c2), dgamma = sum dz * xhat, dbeta = sum dz, dres (+)= da
  eval_affine                scale = gamma / sqrt(rv + eps), shift = beta - rm * scale
  bf16_rne                   round-to-nearest-even of a float64 tensor to the bf16 grid (ONE rounding, from float64)

The exact families (every fp32 / fp64 operation of the kernels is exact, so the result does not depend on fma contraction,
summation order, block count, slot count or atomic arrival order; the conditions are ASSERTED on the float64 reference of
every case - assert_fwd_conditions / assert_bwd_conditions - before anything is launched):

  forward, train mode: count = 2^k; per-channel mean a multiple of 1/4; var = V - (double)(float)eps with V in {1, 1/4, 1/16},
    so var + (double)(float)eps is exactly V and invstd is exactly 1, 2 or 4; the accumulators s1 = mean * count and
    s2 = (var + mean^2) * count (exact in float64: 2^k times a 37-bit number) are split over the slots into dyadic parts of at
    most 45 significant bits on one grid, whose sum in any order is exact; gamma, beta small dyadics; y and res integers;
    momentum 2^-5, running statistics start as dyadics.  scale, shift, mean, invstd, the running mean of three successive
    launches and z = y * scale + shift are then exact; a is the RNE bf16 rounding of an exactly known value (the builder
    requires values that need rounding and ties in both directions).  The running variance multiplies by count / (count - 1),
    which is not exact: its first update is reproduced rounding for rounding (running_var_fp32: IEEE double and float
    operations whose order leaves no choice), later updates are held to rvar_tolerance (two fp32 roundings per launch).
  backward, ACT = 0: da integer in [-4, 4], y integer in [-8, 8], mean a multiple of 1/4, invstd = 2, gamma a signed power of
    two, count = 2^k (given separately from npix).  With q = 2^-(k+2): xhat, dz * xhat, the channel sums, c1, c2, xhat * c2,
    dz - c1 - xhat * c2 and dres + da are multiples of q below 2^24 q, and every partial sum of a channel is a multiple of 1/2
    below 2^23 (sum |dz * xhat| < 2^23): exact in fp32 in any order.
  saturated SiLU, ACT = 1 (forward and backward): scale and shift put every z at >= 32 or <= -100.  sigmoidf_ (csrc/common.h:
    rcp(1 + __expf(-z))) is then exactly 1 (1 + e == 1 in fp32 for e < 2^-24, rcp(1) = 1) or exactly 0 (__expf overflows to
    +inf for -z > 88.8, rcp(inf) = 0): the forward gives z or -0, act' = s * (1 + z * (1 - s)) is 1 or 0.  The reference uses
    these limits (sat_sigmoid) - the premise is checked on the device first (test_premise_*) - so the ACT = 1 instantiations,
    the one-launch backward (dz kept in registers) included, are bit-exact too.
"""
import collections
import math
import types

import torch

F64 = torch.float64
SLOTS = 16                      # MI_BN_SLOTS
MAXC = 2048                     # BN_MAXC
BAR_G = 16                      # MI_BN_BAR_GROUPS
BAR_WORDS = 64 * (1 + 2 * BAR_G)
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127
U32 = 2.0 ** -24                # fp32 unit roundoff (half an ulp, relative)
MOMENTUM = 2.0 ** -5
EPS = 1e-3


def rvar_tolerance(prev_tol, rvar_new):
    """bound on |device - float64| of the running variance after one more launch that starts from a running variance which
    is itself within prev_tol: the old error shrinks by 1 - m; x = (float)(var * unbias) <= 2 carries u |x| and enters times m;
    (1 - m) * rvar rounds (u |rvar|, or not at all under fma contraction) and the sum rounds (u |rvar_new|): in all
    (1 - m) prev_tol + u (2 |rvar_new| + 2 m), first order with |(1 - m) rvar| <= |rvar_new| + m |x|"""
    return (1 - MOMENTUM) * prev_tol + U32 * (2 * rvar_new.abs() + 4 * MOMENTUM)


def acc_c(C):
    """channels of one accumulator slot: C rounded up to 32 (the CoutPad of the conv epilogue)"""
    return (C + 31) // 32 * 32


def f32(x):
    """float64 tensor -> nearest fp32 -> float64"""
    return x.to(torch.float32).to(F64)


def eps_double(eps):
    """(double)(float)eps"""
    return float(torch.tensor(eps, dtype=torch.float32).to(F64))


def pow2(e):
    """2^e as float64, built from its bits (exact on every device; e an integer tensor within the normal range)"""
    return ((e.to(torch.int64) + 1023) << 52).view(F64)


def bf16_rne(x):
    """round a float64 tensor to the nearest bf16 (8 significant bits, exponent range of fp32, subnormals, ties to even,
    overflow to inf) - one rounding from float64; returned as float64"""
    x = x.to(F64)
    _, e = torch.frexp(x)                                  # |x| = m * 2^e, 0.5 <= m < 1
    e = torch.clamp(e, min=-125)                           # below 2^-126 the grid is that of the subnormals: 2^-133
    q = pow2(e - 8)
    r = torch.round(x / q) * q                             # torch.round: half to even; the scaling by 2^n is exact
    r = torch.where(r.abs() > BF16_MAX, torch.sign(x) * math.inf, r)
    return torch.where(torch.isfinite(x) & (x != 0), r, x)


def bf16_half_ulp(x):
    """half the spacing of the bf16 grid at |x| (float64)"""
    _, e = torch.frexp(x.to(F64))
    e = torch.clamp(e, min=-125)
    return pow2(e - 9)


# ---------------------------------------------------------------------------------------------------------- the reference
def sat_sigmoid(z):
    """the saturated limits of sigmoidf_ (module docstring): 1 for z >= 32, 0 for z <= -100; NaN in between (not used there)"""
    return torch.where(z >= 32, torch.ones_like(z), torch.where(z <= -100, torch.zeros_like(z), torch.full_like(z, math.nan)))


def sigmoid_of(z, act):
    return sat_sigmoid(z) if act == "sat" else torch.sigmoid(z)


def act_fn(z, act):
    """act: 0 identity, 1 SiLU, "sat" SiLU with the saturated sigmoid"""
    return z if act == 0 else z * sigmoid_of(z, act)


def act_grad(z, act):
    if act == 0:
        return torch.ones_like(z)
    s = sigmoid_of(z, act)
    return s * (1 + z * (1 - s))


def slot_sums(acc, nslots):
    """acc [SLOTS][CA][2] -> [CA][2]: slots 0 .. nslots - 1, added in slot order"""
    s = torch.zeros_like(acc[0])
    for k in range(nslots):
        s = s + acc[k]
    return s


def norm_slots(nslots):
    """the ABI's reading of nslots: outside 1 .. 16 means 16"""
    return nslots if 1 <= nslots <= SLOTS else SLOTS


def fwd_prologue(acc, nslots, count, gamma, beta, eps, momentum=None, rmean=None, rvar=None, nbt=None):
    """train-mode statistics from the accumulators: all float64.  acc [SLOTS][CA][2]; gamma, beta [C]"""
    C = gamma.numel()
    s = slot_sums(acc.to(F64), norm_slots(nslots))[:C]
    mean = s[:, 0] / count
    var = torch.clamp(s[:, 1] / count - mean * mean, min=0.0)
    invstd = 1.0 / torch.sqrt(var + eps_double(eps))
    scale = gamma.to(F64) * invstd
    shift = beta.to(F64) - mean * gamma.to(F64) * invstd
    out = types.SimpleNamespace(s1=s[:, 0], s2=s[:, 1], mean=mean, var=var, invstd=invstd, scale=scale, shift=shift,
                                rmean=None, rvar=None, nbt=None)
    if rmean is not None:
        unbias = count / (count - 1) if count > 1 else 1.0
        out.rmean = (1 - momentum) * rmean.to(F64) + momentum * mean
        out.rvar = (1 - momentum) * rvar.to(F64) + momentum * var * unbias
    if nbt is not None:
        out.nbt = nbt + 1
    return out


def running_var_fp32(rvar, var, count, momentum):
    """the running-variance update rounding for rounding: (float)(var * unbias) with the IEEE double product (unbias = the
    double quotient count / (count - 1)), then (1 - m) * rvar + m * that in fp32.  m = 2^-5: m * x is exact, and where
    (1 - m) * rvar is exact too (rvar a short dyadic: asserted) the sum rounds once however it is contracted."""
    unbias = torch.tensor(float(count) / float(count - 1) if count > 1 else 1.0, dtype=F64, device=var.device)
    x = f32(var * unbias)
    keep = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(momentum, dtype=torch.float32))
    p = keep * rvar.to(F64)
    assert torch.equal(f32(p), p), "(1 - momentum) * running_var is not exact in fp32"
    return f32(p + momentum * x)


def fwd_apply(y, scale, shift, act, res=None):
    a = act_fn(y.to(F64) * scale.to(F64) + shift.to(F64), act)
    return a if res is None else a + res.to(F64)


def bwd_parts(da, y, scale, shift, mean, invstd, act):
    y = y.to(F64)
    z = y * scale.to(F64) + shift.to(F64)
    dz = da.to(F64) * act_grad(z, act)
    xh = (y - mean.to(F64)) * invstd.to(F64)
    return dz, xh


def bwd_sums(da, y, scale, shift, mean, invstd, act):
    """(sum dz, sum dz * xhat) per channel"""
    dz, xh = bwd_parts(da, y, scale, shift, mean, invstd, act)
    return dz.sum(0), (dz * xh).sum(0)


def bwd_apply(da, y, scale, shift, mean, invstd, gamma, s1, s2, count, act, dres0=None, dres_mode=0):
    """-> dy, dgamma, dbeta, dres (None if dres_mode == 0; 1 overwrite, 2 accumulate onto dres0), float64, unrounded"""
    dz, xh = bwd_parts(da, y, scale, shift, mean, invstd, act)
    c1, c2 = s1 / count, s2 / count
    dy = gamma.to(F64) * invstd.to(F64) * (dz - c1 - xh * c2)
    dres = None
    if dres_mode == 1:
        dres = da.to(F64).clone()
    elif dres_mode == 2:
        dres = dres0.to(F64) + da.to(F64)
    return dy, s2, s1, dres


def eval_affine(gamma, beta, rm, rv, eps):
    invstd = 1.0 / torch.sqrt(rv.to(F64) + eps_double(eps))
    scale = gamma.to(F64) * invstd
    return scale, beta.to(F64) - rm.to(F64) * scale


# ------------------------------------------------------------------------------------------------- conditions and helpers
def on_grid(t, q, bits=24):
    """every element a multiple of q with magnitude below 2^bits q: representable with `bits` significant bits on that grid"""
    u = t / q
    return bool((u == torch.round(u)).all()) and bool((u.abs() < 2.0 ** bits).all())


def rounding_census(v):
    """how many elements of the exactly known float64 v are not bf16 numbers, and how many of those are ties that round
    up / down in magnitude"""
    r = bf16_rne(v)
    h = bf16_half_ulp(v)
    tie = (v != r) & ((v - r).abs() == h)
    return types.SimpleNamespace(inexact=int((v != r).sum()), ties_up=int((tie & (r.abs() > v.abs())).sum()),
                                 ties_down=int((tie & (r.abs() < v.abs())).sum()))


def tpb(C):
    """(C8, pixel lanes PL, working threads TPB) of a 256-thread block"""
    C8 = C // 8
    return C8, 256 // C8, (256 // C8) * C8


def ew_blocks(total):
    """grid of the streaming kernels (ew_blocks of csrc/bn_act.hip: BN_EW_ITEMS = 512 items per block, at most 1024 blocks)"""
    return max(1, min(1024, -(-total // 512)))


def fused_blocks(npix, C, cap):
    """grid of the one-launch backward (bn_fused_blocks: BN_FUSED_ITEMS = 4 items per thread, at most cap blocks)"""
    C8, _, T = tpb(C)
    return max(1, min(cap, -(-npix * C8 // (T * 4))))


def nmine_set(npix, C, nb):
    """the item counts the threads of a fused launch of nb blocks hold"""
    _, PL, _ = tpb(C)
    pstep = nb * PL
    lanes = torch.arange(nb * PL)
    n = torch.clamp((npix - lanes + pstep - 1) // pstep, min=0)
    return set(int(v) for v in n.unique())


def barrier_expected(nb_per_launch):
    """the barrier record after launches of the given block counts on zeroed words: flag [2], top arrivals [0] and every
    group's arrival counter 0; generation of group g = number of launches that used it (g < min(nb, 16))"""
    w = torch.zeros(BAR_WORDS, dtype=torch.int32)
    for nb in nb_per_launch:
        for g in range(min(nb, BAR_G)):
            w[64 * (1 + g)] += 1
    return w


# --------------------------------------------------------------------------------------------------------- forward family
# act: 0, "sat" (ACT = 1 on saturated operands);  lds = (ldy, ldres, lda) or None for C everywhere
FwdCase = collections.namedtuple("FwdCase", "name C npix nslots k act res train lds running seed")


def fwd_lds(c):
    if c.lds is not None:
        return c.lds
    return (c.C, c.C, c.C)


def fwd_cases():
    """C in {8, 24, 40, 96, 264, 1280, 2048} (C8 = 1, 3, 5, 12, 33, 160, 256: TPB 256, 255, 252, 231, 160 and the c += 256
    prologue loops), npix in {1, 5, 777, 4096}, nslots in {1, 3, 16} and 0 / 17 (= 16), train / eval, act 0 / saturated SiLU,
    with / without res, the running-statistics pointers present, absent, or without nbt; count = 2^8, 2^12, 2^17;
    pairwise different leading dimensions"""
    F = FwdCase
    return [
        F("f-c8-n1", 8, 1, 1, 8, 0, False, True, None, "both", 1),
        F("f-c8-n4096", 8, 4096, 16, 12, "sat", True, True, (16, 24, 8), "both", 2),
        F("f-c24-n777", 24, 777, 3, 12, 0, True, True, (40, 24, 32), "none", 3),
        F("f-c24-n5-eval", 24, 5, 16, 8, "sat", False, False, (24, 24, 48), "none", 4),
        F("f-c40-n4096", 40, 4096, 0, 17, 0, False, True, (48, 40, 56), "nonbt", 5),
        F("f-c40-n777-eval", 40, 777, 16, 8, 0, True, False, (40, 64, 48), "none", 6),
        F("f-c96-n5", 96, 5, 17, 8, "sat", True, True, (96, 104, 128), "both", 7),
        F("f-c96-n777", 96, 777, 3, 12, "sat", False, True, (128, 96, 96), "both", 8),
        F("f-c264-n777", 264, 777, 1, 17, 0, True, True, (264, 288, 272), "both", 9),
        F("f-c264-n5-eval", 264, 5, 16, 8, "sat", True, False, (272, 264, 288), "none", 10),
        F("f-c1280-n5", 1280, 5, 16, 12, 0, False, True, (1288, 1280, 1296), "both", 11),
        F("f-c1280-n777", 1280, 777, 3, 8, "sat", True, True, (1280, 1312, 1288), "nonbt", 12),
        F("f-c2048-n1", 2048, 1, 16, 8, "sat", False, True, None, "both", 13),
        F("f-c2048-n777", 2048, 777, 16, 17, 0, True, True, (2056, 2064, 2048), "both", 14),
    ]


def fwd_cap_case():
    """just beyond the 1024-block cap: 4100 x 256 = 1 049 600 items > 1024 x 256 x 4, the 4-deep loop makes a second, partial
    trip"""
    return FwdCase("f-c2048-n4100-cap", 2048, 4100, 16, 12, 0, True, True, (2048, 2056, 2064), "both", 15)


def _gen(seed):
    return torch.Generator().manual_seed(0xB17 + seed)


def _ri(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def make_fwd_operands(c):
    """CPU float64 operands of a forward case (module docstring).  acc holds NaN in the slots >= nslots and in the pad
    channels [C, CA) of every slot"""
    g = _gen(c.seed)
    C, CA, n = c.C, acc_c(c.C), norm_slots(c.nslots)
    count = 2 ** c.k
    o = types.SimpleNamespace(count=count)
    mean = _ri(g, -8, 8, (C,)) / 4
    invstd = 2.0 ** _ri(g, 0, 2, (C,))
    if c.act == "sat":
        gamma = 2.0 ** _ri(g, 0, 2, (C,))                    # scale = gamma * invstd in [1, 16]
        beta = _ri(g, -16, 16, (C,)) / 8
    else:
        gamma = _ri(g, 1, 12, (C,)) / 4 * (1 - 2 * _ri(g, 0, 1, (C,)))
        beta = _ri(g, -16, 16, (C,)) / 8
    if c.train:
        var = 1.0 / (invstd * invstd) - eps_double(EPS)
        s1, s2 = mean * count, (var + mean * mean) * count
        # the parts: random multiples of count / 8 in the first n - 1 slots, the remainder in the last
        acc = torch.full((SLOTS, CA, 2), math.nan, dtype=F64)
        parts = _ri(g, -64, 64, (max(n - 1, 0), C, 2)) * (count / 8.0)
        acc[:n - 1, :C] = parts
        acc[n - 1, :C, 0] = s1 - parts[:, :, 0].sum(0)
        acc[n - 1, :C, 1] = s2 - parts[:, :, 1].sum(0)
        o.acc, o.gamma, o.beta = acc, gamma, beta
        o.rmean0 = _ri(g, -32, 32, (C,)) / 16
        o.rvar0 = _ri(g, 1, 48, (C,)) / 16
        o.nbt0 = 40 + c.seed
        o.scale = o.shift = None
    else:
        o.acc = None
        o.scale = gamma * invstd
        o.shift = beta - mean * gamma * invstd
    scale = gamma * invstd
    shift = beta - mean * gamma * invstd
    if c.act == "sat":
        # y below floor((-100 - shift) / scale) or above ceil((32 - shift) / scale): |y| <= 148, an exact bf16 integer
        lo = torch.floor((-100 - shift) / scale) - _ri(g, 0, 40, (c.npix, C))
        hi = torch.ceil((32 - shift) / scale) + _ri(g, 0, 40, (c.npix, C))
        o.y = torch.where(_ri(g, 0, 1, (c.npix, C)) > 0, hi, lo)
    else:
        o.y = _ri(g, -64, 64, (c.npix, C))
    o.res = _ri(g, -32, 32, (c.npix, C)) if c.res else None
    return o


def fwd_reference(c, o, launches=1):
    """what `launches` successive forward launches of the case must leave: scale .. invstd (train mode), a, the running
    statistics and nbt after every launch.  Computed on o's device"""
    r = types.SimpleNamespace(rmean=[], rvar=[], rvar_tol=[], nbt=[])
    if c.train:
        rm, rv, nbt = (o.rmean0, o.rvar0, o.nbt0) if c.running != "none" else (None, None, None)
        p = None
        for i in range(launches):
            p = fwd_prologue(o.acc, c.nslots, o.count, o.gamma, o.beta, EPS, MOMENTUM, rm, rv, nbt)
            if rm is not None:
                # launch 1 from the dyadic start is reproduced rounding for rounding; later launches start from the float64
                # value of the fp32 number the previous one must have left (mean) / the float64 chain (variance)
                rv_new = running_var_fp32(rv, p.var, o.count, MOMENTUM) if i == 0 else p.rvar
                r.rvar_tol.append(torch.zeros_like(rv_new) if i == 0 else rvar_tolerance(r.rvar_tol[-1], rv_new))
                rm, rv, nbt = p.rmean, rv_new, p.nbt
                r.rmean.append(rm)
                r.rvar.append(rv)
                r.nbt.append(nbt if c.running == "both" else None)
        r.p = p
        r.scale, r.shift, r.mean, r.invstd = p.scale, p.shift, p.mean, p.invstd
    else:
        r.p = None
        r.scale, r.shift = o.scale, o.shift
        r.mean = r.invstd = None
    r.a_exact = fwd_apply(o.y, r.scale, r.shift, c.act, o.res)
    r.a = bf16_rne(r.a_exact)
    return r


def assert_fwd_conditions(c, o, r):
    """the conditions of the forward family, on the float64 reference (module docstring)"""
    assert on_grid(o.y, 1.0, 8) and (o.res is None or on_grid(o.res, 1.0, 8)), "y / res are not bf16 integers"
    if c.train:
        n = norm_slots(c.nslots)
        count = float(o.count)
        assert o.count == 2 ** c.k and c.k >= 4
        live = o.acc[:n, :c.C]
        assert bool(torch.isfinite(live).all()) and bool(o.acc[n:].isnan().all()) and bool(o.acc[:, c.C:].isnan().all())
        # one grid for the parts and every partial sum: 2^-34 count, 45 bits (53 available)
        assert on_grid(live, count * 2.0 ** -34, 45) and on_grid(live.abs().sum(0), count * 2.0 ** -34, 50)
        p = r.p
        vd = p.var + eps_double(EPS)
        assert bool(((vd == 1.0) | (vd == 0.25) | (vd == 0.0625)).all()), "var + eps is not 1, 1/4 or 1/16"
        assert bool(((p.invstd == 1.0) | (p.invstd == 2.0) | (p.invstd == 4.0)).all())
        assert on_grid(p.mean, 0.25, 8) and torch.equal(p.s1, p.mean * count)
        assert torch.equal(p.s2, (p.var + p.mean * p.mean) * count) and on_grid(p.var + p.mean * p.mean, 2.0 ** -34, 40)
        assert on_grid(o.gamma, 0.25, 8) and on_grid(o.beta, 0.125, 8)
        if c.running != "none":
            assert on_grid(o.rmean0, 2.0 ** -4, 10) and on_grid(o.rvar0, 2.0 ** -4, 10)
            for i, rm in enumerate(r.rmean):         # (31/32)^i rmean0 + ... stays on the 2^-(4 + 5 (i + 1)) grid, 24 bits
                assert on_grid(rm, 2.0 ** -(4 + 5 * (i + 1)), 24)
    assert on_grid(r.scale, 2.0 ** -4, 12) and on_grid(r.shift, 2.0 ** -5, 16)
    z = o.y * r.scale + r.shift
    assert on_grid(o.y * r.scale, 2.0 ** -5, 24) and on_grid(z, 2.0 ** -5, 24) and on_grid(r.a_exact, 2.0 ** -5, 24)
    if c.act == "sat":
        assert bool(((z >= 32) | (z <= -100)).all()) and bool((r.scale >= 1).all())
    if o.y.numel() >= 2000:
        cen = rounding_census(r.a_exact)
        assert cen.inexact > 0 and cen.ties_up > 0 and cen.ties_down > 0, vars(cen)


# -------------------------------------------------------------------------------------------------------- backward family
# dres: 0 absent, 1 overwritten, 2 accumulated;  lds = (ldda, ldy, lddy, lddres) or None;  nblk: blocks of the reduce launch;
# cap: resident-block budget for the fused launch (0 = the device's);  nodg: dgamma / dbeta NULL
BwdCase = collections.namedtuple("BwdCase", "name C npix nslots k act dres lds nblk cap nodg seed")


def bwd_lds(c):
    return c.lds if c.lds is not None else (c.C,) * 4


def bwd_cases():
    """the forward's C and npix; nblk in {1, 3, more blocks than pixel lanes of work, 1024}; dres absent / overwritten /
    accumulated; dgamma, dbeta NULL; count = 2^k is given separately from npix (the ABI takes both), small enough that the
    channel sums stay below 2^24 q = 2^(22 - k) as well"""
    B = BwdCase
    return [
        B("b-c8-n1", 8, 1, 1, 4, 0, 2, None, 3, 0, False, 1),                      # 3 blocks for one pixel
        B("b-c8-n4096", 8, 4096, 16, 8, "sat", 1, (16, 24, 8, 32), 1024, 0, False, 2),
        B("b-c24-n777", 24, 777, 3, 8, 0, 2, (40, 24, 32, 48), 3, 0, False, 3),
        B("b-c24-n5", 24, 5, 16, 4, "sat", 0, (24, 32, 48, 0), 1, 0, True, 4),
        B("b-c40-n4096", 40, 4096, 0, 8, 0, 0, (48, 40, 56, 0), 40, 0, False, 5),
        B("b-c40-n777", 40, 777, 3, 8, "sat", 2, (40, 64, 48, 56), 1024, 0, False, 6),
        B("b-c96-n5", 96, 5, 17, 4, 0, 1, (96, 104, 128, 112), 3, 0, True, 7),        # 21 lanes x 3 blocks > 5 pixels
        B("b-c96-n777", 96, 777, 16, 8, "sat", 1, (128, 96, 104, 112), 7, 0, False, 8),
        B("b-c264-n777", 264, 777, 1, 8, 0, 2, (264, 288, 272, 280), 1, 0, False, 9),
        B("b-c264-n5", 264, 5, 16, 4, "sat", 0, (272, 264, 288, 0), 3, 0, False, 10),
        B("b-c1280-n5", 1280, 5, 16, 4, 0, 2, (1288, 1280, 1296, 1304), 1024, 0, False, 11),  # 1024 blocks, 5 with work
        B("b-c1280-n777", 1280, 777, 3, 8, "sat", 0, (1280, 1312, 1288, 0), 40, 0, False, 12),
        B("b-c2048-n1", 2048, 1, 16, 4, "sat", 1, None, 1, 0, False, 13),
        B("b-c2048-n777", 2048, 777, 16, 8, 0, 1, (2056, 2064, 2048, 2072), 3, 0, True, 14),
    ]


def bwd_cap_cases():
    """just beyond the 1024-block cap of the streaming kernels: 2100 x 256 = 537 600 items > 1024 x 256 x 2, a thread of the
    2-deep apply loop takes a third item (a second trip); identity with accumulated dres, and its saturated-SiLU twin with
    dres overwritten"""
    lds = (2056, 2064, 2048, 2072)
    return [BwdCase("b-c2048-n2100-cap", 2048, 2100, 16, 8, 0, 2, lds, 1024, 0, False, 15),
            BwdCase("b-c2048-n2100-cap-sat", 2048, 2100, 16, 8, "sat", 1, lds, 1024, 0, False, 16)]


def fused_capacity_cases():
    """mi_bn_fused_set_capacity(cap) pins the grid of the one-launch backward at nb = cap in {1, 2, 15, 16, 17, 33} (one block;
    fewer blocks than barrier groups; the two-level barrier with even and uneven groups) and npix = nb * PL * m + r gives its
    threads m or m + 1 items, either side of the on-chip capacity R = 14 (and of 16), with odd tails for the
    4-deep and 2-deep streaming loops: {13, 14}, {15, 16}, {16, 17}, {19, 20}, {13, 14}, {17, 18}, {14, 15}; b-c8-n5-cap1 has
    threads without any item"""
    B = BwdCase
    return [
        B("u-c8-nb1", 8, 1 * 256 * 13 + 100, 16, 8, "sat", 2, (16, 24, 8, 32), 1, 1, False, 21),
        B("u-c8-n5-nb1", 8, 5, 3, 4, 0, 1, (8, 16, 24, 32), 1, 1, False, 22),
        B("u-c24-nb2", 24, 2 * 85 * 15 + 50, 3, 8, 0, 1, (40, 24, 32, 48), 1, 2, False, 23),
        B("u-c40-nb15", 40, 15 * 51 * 16 + 300, 16, 6, "sat", 0, (48, 40, 56, 0), 1, 15, False, 24),
        B("u-c96-nb16", 96, 16 * 21 * 19 + 100, 1, 6, 0, 2, (96, 104, 128, 112), 1, 16, True, 25),
        B("u-c264-nb17", 264, 17 * 7 * 13 + 50, 16, 8, "sat", 2, (264, 288, 272, 280), 1, 17, False, 26),
        B("u-c2048-nb17", 2048, 17 * 17 + 5, 5, 8, 0, 0, (2056, 2064, 2048, 0), 1, 17, False, 27),
        B("u-c1280-nb33", 1280, 33 * 14 + 7, 16, 8, "sat", 1, (1288, 1280, 1296, 1304), 1, 33, False, 28),
    ]


SAT_SCALE = 64.0


def make_bwd_operands(c):
    """CPU float64 operands of a backward case.  scale / shift / mean / invstd are independent inputs of the backward ABI:
    ACT = 0 ignores z, the saturated family puts z = 64 y + shift (shift in {0, 8, 16, 28}, y never -1 or 0) at >= 64 or
    <= -100"""
    g = _gen(100 + c.seed)
    C = c.C
    o = types.SimpleNamespace(count=2 ** c.k)
    o.da = _ri(g, -4, 4, (c.npix, C))
    o.y = _ri(g, -8, 8, (c.npix, C))
    o.mean = _ri(g, -8, 8, (C,)) / 4
    o.invstd = torch.full((C,), 2.0, dtype=F64)
    o.gamma = 2.0 ** _ri(g, -2, 2, (C,)) * (1 - 2 * _ri(g, 0, 1, (C,)))
    if c.act == "sat":
        o.y = torch.where((o.y == 0) | (o.y == -1), o.y + 3, o.y)
        o.scale = torch.full((C,), SAT_SCALE, dtype=F64)
        o.shift = torch.tensor([0.0, 8.0, 16.0, 28.0], dtype=F64)[torch.randint(0, 4, (C,), generator=g)]
    else:
        o.scale = o.gamma * o.invstd
        o.shift = -o.mean * o.scale
    o.dres0 = _ri(g, -100, 100, (c.npix, C)) if c.dres == 2 else None
    return o


def bwd_reference(c, o):
    """sums, dy (rounded), dgamma, dbeta, dres of a backward case"""
    s1, s2 = bwd_sums(o.da, o.y, o.scale, o.shift, o.mean, o.invstd, c.act)
    dy, dg, db, dres = bwd_apply(o.da, o.y, o.scale, o.shift, o.mean, o.invstd, o.gamma, s1, s2, float(o.count), c.act,
                                 o.dres0, c.dres)
    return types.SimpleNamespace(s1=s1, s2=s2, dy_exact=dy, dy=bf16_rne(dy), dgamma=dg, dbeta=db,
                                 dres=None if dres is None else bf16_rne(dres), dres_exact=dres)


def assert_bwd_conditions(c, o, r):
    """the conditions of the backward families, on the float64 reference (module docstring)"""
    count = float(o.count)
    q = 2.0 ** -(c.k + 2)
    assert on_grid(o.da, 1.0, 3) and on_grid(o.y, 1.0, 4) and bool((o.da.abs() <= 4).all()) and bool((o.y.abs() <= 8).all())
    assert on_grid(o.mean, 0.25, 6) and bool((o.invstd == 2.0).all())
    lg = torch.log2(o.gamma.abs())
    assert bool((lg == torch.round(lg)).all()) and bool((lg.abs() <= 2).all()), "gamma is not a signed power of two"
    z = o.y * o.scale + o.shift
    assert on_grid(o.scale, 2.0 ** -3, 12) and on_grid(o.shift, 2.0 ** -5, 16) and on_grid(z, 2.0 ** -5, 24)
    if c.act == "sat":
        assert bool(((z >= 32) | (z <= -100)).all())
    dz, xh = bwd_parts(o.da, o.y, o.scale, o.shift, o.mean, o.invstd, c.act)
    assert bool(((dz == o.da) | (dz == 0)).all())
    c1, c2 = r.s1 / count, r.s2 / count
    for t in (xh, dz * xh, r.s1, r.s2, c1, c2, xh * c2, dz - c1, dz - c1 - xh * c2):
        assert on_grid(t, q, 24), "an intermediate leaves the grid 2^-(k+2) x 2^24"
    # every partial sum of a channel, in any order: multiples of 1/2 below 2^23
    assert on_grid(dz * xh, 0.5, 24) and bool((dz.abs().sum(0) < 2.0 ** 23).all()) and bool(((dz * xh).abs().sum(0) < 2.0 ** 23).all())
    assert torch.equal(f32(r.dgamma), r.dgamma) and torch.equal(f32(r.dbeta), r.dbeta) and torch.equal(f32(c1), c1) and torch.equal(f32(c2), c2)
    if c.dres == 2:
        assert on_grid(o.dres0, 1.0, 8) and on_grid(r.dres_exact, 1.0, 8) and torch.equal(r.dres, r.dres_exact)


# -------------------------------------------------------------------------------------------------------- grouped launches
def group_cases():
    """kinds 0 - 3 with n in {1, 3, 8} jobs of different C, npix, ld and nslots, all of one activation (a launch parameter)"""
    def fwd(n, act, s):
        shapes = [(24, 777), (8, 5), (264, 300), (96, 1), (40, 1000), (1280, 33), (2048, 5), (8, 4096)][:n]
        return [FwdCase("gf%d-%s-%d" % (n, act, i), C, npix, (1, 3, 16, 0, 5, 16, 2, 17)[i], (12, 8, 17, 8, 12, 8, 8, 12)[i], act,
                        i % 2 == 0, i != 3, (C + 8 * ((i + 1) % 3), C + 8 * ((i + 2) % 3), C + 8 * (i % 3)),
                        ("both", "none", "nonbt")[i % 3], s + i) for i, (C, npix) in enumerate(shapes)]

    def bwd(n, act, s, fused):
        shapes = [(24, 777), (8, 5), (264, 300), (96, 1), (40, 1000), (1280, 33), (2048, 5), (8, 4096)][:n]
        return [BwdCase("g%s%d-%s-%d" % ("u" if fused else "b", n, act, i), C, npix, (1, 3, 16, 0, 5, 16, 2, 17)[i],
                        (8, 4, 8, 4, 8, 6, 4, 8)[i], act, i % 3,
                        (C + 8 * (i % 4), C + 8 * ((i + 1) % 4), C + 8 * ((i + 2) % 4), (C + 8 * ((i + 3) % 4)) if i % 3 else 0),
                        (1, 3, 7, 2, 40, 5, 1, 1024)[i], 0, i == 2, s + i) for i, (C, npix) in enumerate(shapes)]
    out = []
    for n, act in ((1, "sat"), (3, 0), (8, "sat"), (8, 0)):
        out.append(types.SimpleNamespace(kind=0, n=n, act=act, jobs=fwd(n, act, 200 + 10 * n)))
        out.append(types.SimpleNamespace(kind=12, n=n, act=act, jobs=bwd(n, act, 300 + 10 * n, False)))   # reduce, then apply
        out.append(types.SimpleNamespace(kind=3, n=n, act=act, jobs=bwd(n, act, 400 + 10 * n, True)))
    return out


# ------------------------------------------------------------------------------------------------ instantiations (coverage)
def instantiations():
    """every kernel instantiation of csrc/bn_act.hip: the three streaming kernels and the one-launch backward, each with the
    activation off / on, single and grouped - 16"""
    return ["%s%s_kernel<%d>" % (k, g, a) for k in ("bn_act_fwd", "bn_bwd_reduce", "bn_bwd_apply", "bn_bwd_fused")
            for g in ("", "_group") for a in (0, 1)]


def kernel_name(stem, act, group=False):
    """the instantiation a launch runs, by the dispatch of the entry points (act != 0 -> <1>)"""
    return "%s%s_kernel<%d>" % (stem, "_group" if group else "", 1 if act else 0)


# ------------------------------------------------------------------------------------------------------- derived bounds
# fp32 evaluation of sigmoidf_(z) = rcp(1 + __expf(-z)), __expf(x) = exp2(x * log2(e)) by v_exp_f32.  With u = 2^-24 (half an
# ulp) and the instruction accuracies of the CDNA ISA manuals (v_exp_f32 and v_rcp_f32: 1 ulp = 2 u; both flush subnormals):
#   t = fl(-z * log2e): the constant carries u, the product u                 -> e = 2^t is off by |t| ln2 2u = 2 |z| u (relative)
#   v_exp_f32: 2 u                                                            -> e (1 + (2 |z| + 2) u)
#   1 + e rounds: u; e's error enters 1 + e scaled by e / (1 + e) = 1 - s     -> (1 + e)(1 + ((2 |z| + 2)(1 - s) + 1) u)
#   v_rcp_f32: 2 u                                                            -> s (1 + ((2 |z| + 2)(1 - s) + 3) u)
# so |s_fp32 - s| <= s * SIG_REL(z, s) with SIG_REL = ((2 |z| + 2)(1 - s) + 3) u, to first order; beyond z < -87 (1 + e above
# 2^126, rcp flushes) and for subnormal z the absolute floor FLOOR = 2^-100 takes over (|z s| < 2^-119 there).
FLOOR = 2.0 ** -100


def sig_rel(z, s):
    return ((2 * z.abs() + 2) * (1 - s) + 3) * U32


def silu_bound(z, dz_abs=None):
    """|fp32 z * sigmoidf_(z) - silu(z)| for an fp32 z that is within dz_abs of the float64 z (first order): the derivative
    times dz_abs, the sigmoid term, one rounding of the product"""
    z = z.to(F64)
    s = torch.sigmoid(z)
    b = (z * s).abs() * (sig_rel(z, s) + U32) + FLOOR
    if dz_abs is not None:
        b = b + (s * (1 + z * (1 - s))).abs() * dz_abs
    return b


def silu_grad_bound(z, dz_abs=None):
    """|fp32 s * (1 + z * (1 - s)) - silu'(z)| (act_grad of csrc/bn_act.hip), first order: 1 - s carries s SIG_REL + u (1 - s);
    z * that and 1 + that round; the outer product carries s's error and rounds"""
    z = z.to(F64)
    s = torch.sigmoid(z)
    e1 = s * sig_rel(z, s) + U32 * (1 - s)                   # 1 - s
    t = z * (1 - s)
    e2 = z.abs() * e1 + U32 * t.abs()                        # z * (1 - s)
    e3 = e2 + U32 * (1 + t).abs()                            # 1 + z * (1 - s)
    b = s * e3 + (s * (1 + t)).abs() * (sig_rel(z, s) + U32) + FLOOR
    if dz_abs is not None:
        d2 = s * (1 - s) * (2 + z * (1 - 2 * s))             # silu''
        b = b + d2.abs() * dz_abs
    return b


def emulate_sigmoid_fp32(z32):
    """the expression of sigmoidf_ in fp32 on the host (correctly rounded operations, torch's exp)"""
    return torch.reciprocal(1.0 + torch.exp(-z32))


def all_finite_bf16():
    """every finite bf16 value, as a bf16 tensor (65 536 patterns minus inf / NaN, padded to 65 536 with zeros)"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v = bits.view(torch.bfloat16)
    return torch.where(torch.isfinite(v.float()), v, torch.zeros_like(v))


def norm_rel(a, b):
    """the criterion of tests/test_gpu_kernels.py: ||a - b|| / ||b||"""
    return float((a.to(F64) - b.to(F64)).norm() / b.to(F64).norm().clamp_min(1e-30))


def fused_old_criterion(dy_ref, dy):
    """the criterion of test_bn_backward_fused_matches_two_pass for dy: at most one bf16 ulp of the largest magnitude, and
    fewer than 2 % of the elements different"""
    diff = (dy_ref - dy).abs()
    return float(diff.max()) <= float(dy_ref.abs().max()) * 2 ** -7 and float((diff > 0).to(F64).mean()) < 0.02


# ------------------------------------------------------------------------------------------------------------- mutants
# Standing mutation evidence, on the reference side: each mutant is the reference with one defect a kernel could have.  It
# comes in two views: `exact` - what the defective kernel would leave under the hygiene of tests/test_gpu_bn_exact.py (outputs
# pre-filled with NaN before every launch, NaN in the unused accumulator slots, pairwise different leading dimensions) - and
# `old` - what it would leave under the hygiene of the older tests (one ld for every tensor, all 16 slots zeroed, outputs not
# refilled between the repeated launches).  The exact comparison must reject `exact`; the older criteria accept `old`.
def fwd_mutation_case():
    return FwdCase("mut-fwd", 264, 777, 3, 12, 0, True, True, (264, 288, 272), "both", 31)


def bwd_mutation_case():
    """2 blocks x 21 lanes, 17 or 18 items per thread: item R exists for R = 14 (and for 16)"""
    return BwdCase("mut-bwd", 96, 2 * 21 * 17 + 20, 3, 8, 0, 2, (104, 96, 112, 128), 3, 2, False, 32)


def fwd_outputs(r):
    """the outputs of one forward launch as a dict of float64 tensors"""
    d = dict(a=r.a, scale=r.scale, shift=r.shift, mean=r.mean, invstd=r.invstd)
    if r.rmean:
        d.update(rmean=r.rmean[0], rvar=r.rvar[0])
    return d


def fwd_mutants(c, o, r):
    """name -> (exact view, old view) of the forward outputs (one launch)"""
    ref = fwd_outputs(r)
    out = {}
    # the last channel group of pixel PL - 1 (block 0's last thread group) computed with the neighbouring group's scale / shift
    C8, PL, _ = tpb(c.C)
    m = dict(ref)
    cs, cn = slice((C8 - 1) * 8, C8 * 8), slice((C8 - 2) * 8, (C8 - 1) * 8)
    a = r.a_exact.clone()
    a[PL - 1, cs] = fwd_apply(o.y[PL - 1, cs], r.scale[cn], r.shift[cn], c.act, None if o.res is None else o.res[PL - 1, cs])
    m["a"] = bf16_rne(a)
    out["neighbouring channel group's scale / shift for the last thread group"] = (m, m)
    # slot `nslots` read as well: NaN under the exact hygiene, zero under the old one
    n = norm_slots(c.nslots)
    if n < SLOTS:
        out["slot nslots read"] = ({k: torch.full_like(v, math.nan) for k, v in ref.items()}, ref)
    # the running variance updated with the biased variance
    if r.rmean:
        m = dict(ref)
        m["rvar"] = f32((1 - MOMENTUM) * o.rvar0 + MOMENTUM * f32(r.p.var))
        out["biased variance in the running update"] = (m, m)
    return out


def bwd_outputs(r):
    d = dict(dy=r.dy, dgamma=r.dgamma, dbeta=r.dbeta)
    if r.dres is not None:
        d["dres"] = r.dres
    return d


def restride(flat, ld, npix, C):
    """rows of C elements read at row stride ld from the flat buffer (NaN beyond its end)"""
    idx = torch.arange(npix, device=flat.device)[:, None] * ld + torch.arange(C, device=flat.device)[None, :]
    ok = idx < flat.numel()
    return torch.where(ok, flat[idx.clamp(max=flat.numel() - 1)].to(F64), torch.full_like(idx, math.nan, dtype=F64))


def bwd_mutants(c, o, r, nb, R, da_flat):
    """name -> (exact view, old view) of the backward outputs.  nb, R: grid and register capacity of the fused launch; da_flat:
    the da buffer from the view's first element on, as the kernel sees it (row stride ldda, NaN between the rows)"""
    ref = bwd_outputs(r)
    count = float(o.count)
    out = {}

    def outputs(da, s1, s2):
        dy, dg, db, dres = bwd_apply(da, o.y, o.scale, o.shift, o.mean, o.invstd, o.gamma, s1, s2, count, c.act, o.dres0, c.dres)
        d = dict(dy=bf16_rne(dy), dgamma=dg, dbeta=db)
        if dres is not None:
            d["dres"] = bf16_rne(dres)
        return d
    # one pixel left out of one channel's sums
    dz, xh = bwd_parts(o.da, o.y, o.scale, o.shift, o.mean, o.invstd, c.act)
    pix = int(torch.nonzero(dz[:, 5] * xh[:, 5])[-1])
    s1, s2 = r.s1.clone(), r.s2.clone()
    s1[5] -= dz[pix, 5]
    s2[5] -= dz[pix, 5] * xh[pix, 5]
    m = outputs(o.da, s1, s2)
    out["one pixel left out of a channel's sums"] = (m, m)
    # item R of thread 0 of block 0 skipped in phase 2: dy keeps what was there - NaN, or the previous identical launch's value
    _, PL, _ = tpb(c.C)
    m = dict(ref)
    m["dy"] = ref["dy"].clone()
    m["dy"][R * nb * PL, 0:8] = math.nan
    out["item R of a thread skipped in phase 2"] = (m, ref)
    # da indexed with ldy
    ldda, ldy = bwd_lds(c)[0], bwd_lds(c)[1]
    assert ldda != ldy
    da2 = restride(da_flat, ldy, c.npix, c.C)
    s1b, s2b = bwd_sums(da2, o.y, o.scale, o.shift, o.mean, o.invstd, c.act)
    out["ldy used for da"] = (outputs(da2, s1b, s2b), ref)
    # dres overwritten where it should accumulate, at one item
    if c.dres == 2:
        m = dict(ref)
        m["dres"] = ref["dres"].clone()
        p = int(torch.nonzero(o.dres0[:, 8])[0])
        m["dres"][p, 8:16] = o.da[p, 8:16].to(ref["dres"].device)
        out["dres overwritten where it should accumulate"] = (m, m)
    return out


def same(a, b):
    """bitwise agreement of two float64 tensors holding fp32 / bf16 values (NaN equals NaN; -0 equals +0)"""
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def old_criteria_accept(ref, got):
    """the criteria the older tests hold these outputs to: 2e-2 norm-relative for every tensor (test_base_conv_fwd_bwd), the
    one-ulp / 2 % criterion for dy (test_bn_backward_fused_matches_two_pass), 2e-3 for the running statistics"""
    for k, v in ref.items():
        g = got[k]
        if k in ("rmean", "rvar"):
            if not bool(((g - v).abs() <= 2e-3 + 2e-3 * v.abs()).all()):
                return False
        elif not norm_rel(g, v) < 2e-2:         # (NaN fails)
            return False
    if "dy" in ref and not fused_old_criterion(ref["dy"], got["dy"]):
        return False
    return True


# ------------------------------------------------------------------------------------------- random-data numerics: bounds
# Elementwise first-order worst-case bounds for Gaussian data with real statistics and SiLU, from: the rounding points (half a
# bf16 ulp at every store: store_bound), the fp32 operations of the expressions as written in csrc/bn_act.hip (u = 2^-24 per
# operation; a contracted fma only removes a term), an fp32 summation chain of known length for the per-thread and per-block
# sums (any order of N additions: (N - 1) u sum |terms|), and the sigmoid term SIG_REL above.  Second-order terms are covered
# by the factor SECOND = 1 + 2^-10 on every fp32 bound.  The float64 reference is fed the same bf16 inputs and the device's
# own fp32 scale / shift / mean / invstd, so the statistics' rounding does not enter twice.
SECOND = 1 + 2.0 ** -10
NumCase = collections.namedtuple("NumCase", "name C npix nslots res dres nblk seed")


def numerics_cases():
    return [NumCase("n-c80", 80, 1500, 16, True, 2, 16, 1), NumCase("n-c264", 264, 700, 3, False, 1, 5, 2),
            NumCase("n-c24", 24, 3000, 5, True, 0, 8, 3)]


def make_numerics_operands(nc):
    g = _gen(500 + nc.seed)
    bf = lambda t: t.to(torch.bfloat16).to(F64)
    o = types.SimpleNamespace(count=nc.npix)
    o.y = bf(torch.randn(nc.npix, nc.C, generator=g) * 1.5 + 0.3)
    o.da = bf(torch.randn(nc.npix, nc.C, generator=g))
    o.res = bf(torch.randn(nc.npix, nc.C, generator=g)) if nc.res else None
    o.dres0 = bf(torch.randn(nc.npix, nc.C, generator=g)) if nc.dres == 2 else None
    o.gamma = (torch.rand(nc.C, generator=g) + 0.5).to(F64)
    o.beta = (torch.randn(nc.C, generator=g) * 0.1).to(F64)
    o.rmean0 = torch.randn(nc.C, generator=g).to(F64)
    o.rvar0 = (torch.rand(nc.C, generator=g) + 0.5).to(F64)
    CA = acc_c(nc.C)
    o.acc = torch.full((SLOTS, CA, 2), math.nan, dtype=F64)
    for k, ch in enumerate(torch.tensor_split(o.y, nc.nslots, dim=0)):
        o.acc[k, :nc.C, 0], o.acc[k, :nc.C, 1] = ch.sum(0), (ch * ch).sum(0)
    return o


def store_bound(v, e):
    """|bf16 store of a value within e of v, minus v|"""
    return e + bf16_half_ulp(v.abs() + e)


def stats_bounds(p, gamma, beta, momentum, rmean0, rvar0):
    """bounds for the fp32 numbers the train-mode prologue writes, against fwd_prologue in float64: the fp64 chain (16 adds,
    a product, a difference with cancellation, sqrt, divide, products: below 2^-45 relative to the largest operand) and one
    rounding to fp32; the running statistics add two fp32 products and a sum (3 u on the operands' magnitudes)"""
    d = 2.0 ** -45
    b = types.SimpleNamespace()
    b.mean = U32 * p.mean.abs() * SECOND + d * (p.s1.abs() / p.s1.abs().clamp_min(1e-300)) * p.mean.abs()
    relv = d * (p.var + p.mean * p.mean) / (p.var + eps_double(EPS))
    b.invstd = (U32 * SECOND + relv) * p.invstd
    b.scale = (U32 * SECOND + relv) * p.scale.abs()
    b.shift = U32 * p.shift.abs() * SECOND + (relv + d) * (beta.abs() + (p.mean * p.scale).abs())
    b.rmean = SECOND * U32 * (2 * ((1 - momentum) * rmean0).abs() + 2 * momentum * p.mean.abs() + p.rmean.abs())
    b.rvar = SECOND * U32 * (2 * ((1 - momentum) * rvar0).abs() + 2 * momentum * p.var.abs() * 1.01 + p.rvar.abs()) + relv * p.var
    return b


def numerics_fwd(o, scale, shift):
    """(a in float64, elementwise bound on the device's bf16 a) for ACT = 1, given the device's fp32 scale / shift"""
    z = o.y * scale + shift
    dzb = U32 * ((o.y * scale).abs() + z.abs())
    a = z * torch.sigmoid(z)
    e = silu_bound(z, dzb)
    if o.res is not None:
        a = a + o.res
        e = e + U32 * a.abs()
    return a, store_bound(a, e * SECOND)


def numerics_bwd(o, scale, shift, mean, invstd, gamma, chain, dres_mode):
    """reference and elementwise bounds of dgamma, dbeta, dy, dres for ACT = 1.  chain: the longest sequence of fp32
    additions a channel sum passes through (a thread's items + the pixel lanes of a block)"""
    y, da, count = o.y, o.da, float(o.count)
    z = y * scale + shift
    dzb = U32 * ((y * scale).abs() + z.abs())
    dz = da * act_grad(z, 1)
    e_dz = da.abs() * silu_grad_bound(z, dzb) + U32 * dz.abs()
    xh = (y - mean) * invstd
    e_xh = 2 * U32 * xh.abs()
    t = dz * xh
    e_t = xh.abs() * e_dz + dz.abs() * e_xh + U32 * t.abs()
    S1, S2 = dz.sum(0), t.sum(0)
    e_S1 = e_dz.sum(0) + chain * U32 * dz.abs().sum(0)
    e_S2 = e_t.sum(0) + chain * U32 * t.abs().sum(0)
    k1, k2 = S1 / count, S2 / count
    e_k1, e_k2 = e_S1 / count + U32 * k1.abs(), e_S2 / count + U32 * k2.abs()
    gi = gamma * invstd
    inner = dz - k1 - xh * k2
    e_in = e_dz + e_k1 + xh.abs() * e_k2 + k2.abs() * e_xh + U32 * (xh * k2).abs() + U32 * (dz - k1).abs() + U32 * inner.abs()
    dy = gi * inner
    e_dy = gi.abs() * e_in + inner.abs() * U32 * gi.abs() + U32 * dy.abs()
    ref = dict(dy=dy, dgamma=S2, dbeta=S1)
    bound = dict(dy=store_bound(dy, e_dy * SECOND), dgamma=(e_S2 + U32 * S2.abs()) * SECOND, dbeta=(e_S1 + U32 * S1.abs()) * SECOND)
    if dres_mode == 1:
        ref["dres"], bound["dres"] = da, torch.zeros_like(da)
    elif dres_mode == 2:
        ref["dres"] = o.dres0 + da
        bound["dres"] = store_bound(ref["dres"], U32 * ref["dres"].abs())
    return ref, bound


def emulate_numerics_fp32(o, scale, shift, mean, invstd, gamma, dres_mode):
    """the expressions of the kernels in fp32 on the host (sigmoidf_ by emulate_sigmoid_fp32, sums by torch's fp32 sum), stores
    rounded to bf16: a, dy, dgamma, dbeta, dres as float64"""
    f = lambda t: t.float()
    y, da, sc, sh, mu, is_ = f(o.y), f(o.da), f(scale), f(shift), f(mean), f(invstd)
    z = y * sc + sh
    s = emulate_sigmoid_fp32(z)
    a = z * s
    if o.res is not None:
        a = a + f(o.res)
    dz = da * (s * (1.0 + z * (1.0 - s)))
    xh = (y - mu) * is_
    S1, S2 = dz.sum(0), (dz * xh).sum(0)
    k1, k2 = (S1.to(F64) / o.count).float(), (S2.to(F64) / o.count).float()
    dy = (f(gamma) * is_) * (dz - k1 - xh * k2)
    bf = lambda t: t.to(torch.bfloat16).to(F64)
    out = dict(a=bf(a), dy=bf(dy), dgamma=S2.to(F64), dbeta=S1.to(F64))
    if dres_mode == 1:
        out["dres"] = o.da.clone()
    elif dres_mode == 2:
        out["dres"] = bf(f(o.dres0) + da)
    return out


def chain_length(npix, C, nb):
    """additions a channel sum passes through in a launch of nb blocks: a thread's items, then the block's pixel lanes"""
    _, PL, _ = tpb(C)
    return -(-npix // (nb * PL)) + PL


def eval_affine_bounds(gamma, beta, rm, rv, eps):
    """mi_bn_eval_affine computes invstd = 1.0f / sqrtf(rv + eps), scale = gamma * invstd, shift = beta - rm * gamma * invstd
    in fp32.  hipcc's default for this file rounds fp32 sqrt and divide correctly (-fhip-fp32-correctly-rounded-divide-sqrt),
    so with u = 2^-24: the sum rv + eps carries u, which enters invstd halved; sqrt u; divide u -> invstd (1 + 2.5 u);
    scale one more product -> 3.5 u |scale|; shift: rm * gamma (u), times invstd (2.5 u + u), the difference rounds (u |shift|)
    -> 4.5 u |rm scale| + u |shift| (an fma for the last two operations only removes a term).  Against the float64 reference
    that adds (double)(float)eps.  Returns (scale bound, shift bound)"""
    sc, sh = eval_affine(gamma, beta, rm, rv, eps)
    return 3.5 * U32 * sc.abs() * SECOND, (4.5 * U32 * (rm * sc).abs() + U32 * sh.abs()) * SECOND
