"""Plain float64 restatement of the BatchNorm + ReLU ABI of csrc/bn_relu.hip as include/mi355_det.h states it (mi_bn_stats,
mi_bn_relu_fwd, mi_bn_relu_bwd_reduce / _apply), and the cases tests/test_gpu_bn_relu_exact.py runs bit for bit.
tests/test_bn_relu_ref.py pins it to torch's float64 autograd of relu(batch_norm(y1) + batch_norm(y2)) and of the residual form.

  stats        per-channel (sum x, sum x^2)
  fwd          a = act(y1 * scale1 + shift1 [+ y2 * scale2 + shift2 | + res]), act = max(., 0) when relu; unrounded
  dz_of        dz = da where the saved output a > 0, else 0 (relu == 0: dz = da)
  bwd_norm     one norm operand: (sum dz, sum dz * xhat) and dy = gamma * invstd * (dz - c1 - xhat * c2), c = sums / count
  bwd_res      dres = dz (written by reduce already, read back by apply), or dres0 + dz (apply)

The exact families are those of tests/bn_ref.py (its module docstring): ReLU is exact on any operand, so the forward uses the
dyadic-statistics family with ACT = 0 operands (invstd in {1, 2, 4}; in the two-norm form both operands come from it and
z1 + z2 must stay on the 2^-5 grid within 24 bits: asserted), the backward the ACT = 0 integer family with a saved output
that holds zeros, negatives and positives: the masked dz is again an integer in [-4, 4], so every condition of that family
holds for it (asserted per operand with the masked gradient in da's place)."""
import collections
import math
import types

import torch

import bn_ref as B

F64 = torch.float64
EPS, MOMENTUM = B.EPS, B.MOMENTUM   # launch parameters: the statistics of bn_ref's family are built for these
WIDTHS = (8, 24, 56, 152, 368)   # a single octet, and RegNetX-200MF's widths: C8 = 1, 3, 7, 19, 46
NPIX = (64, 1024)
NSLOTS = (1, 16)


# ----------------------------------------------------------------------------------------------------------- the reference
def stats(x):
    x = x.to(F64)
    return x.sum(0), (x * x).sum(0)


def fwd(y1, scale1, shift1, relu, y2=None, scale2=None, shift2=None, res=None):
    assert y2 is None or res is None, "the ABI refuses a second norm operand together with a plain residual"
    z = y1.to(F64) * scale1.to(F64) + shift1.to(F64)
    if y2 is not None:
        z = z + (y2.to(F64) * scale2.to(F64) + shift2.to(F64))
    if res is not None:
        z = z + res.to(F64)
    return torch.clamp(z, min=0.0) if relu else z


def dz_of(da, a, relu):
    da = da.to(F64)
    return torch.where(a.to(F64) > 0, da, torch.zeros_like(da)) if relu else da


def bwd_norm(dz, y, mean, invstd, gamma, count):
    """-> s1 = sum dz (= dbeta), s2 = sum dz * xhat (= dgamma), dy (unrounded)"""
    xh = (y.to(F64) - mean.to(F64)) * invstd.to(F64)
    s1, s2 = dz.sum(0), (dz * xh).sum(0)
    dy = gamma.to(F64) * invstd.to(F64) * (dz - s1 / count - xh * (s2 / count))
    return s1, s2, dy


def bwd_res(dz, dres0=None):
    return dz.clone() if dres0 is None else dres0.to(F64) + dz


# ------------------------------------------------------------------------------------------------------------------ cases
Shape = collections.namedtuple("Shape", "C npix nslots")
FORMS = ("one", "two", "res")


def shapes():
    return [Shape(C, n, s) for C in WIDTHS for n in NPIX for s in NSLOTS]


def shape_id(s):
    return "c%d-n%d-s%d" % s


def lds(s, n, different):
    """n leading dimensions: C everywhere, or pairwise different multiples of 8 above C"""
    return [s.C + 8 * (i + 1) for i in range(n)] if different else [s.C] * n


def different_lds(s):
    """one shape per width carries pairwise different leading dimensions above C"""
    return s.npix == NPIX[0] and s.nslots == NSLOTS[-1]


def _k(npix):
    k = int(math.log2(npix))
    assert 2 ** k == npix
    return k


def fwd_operand(s, train, seed):
    """one norm operand of the dyadic family (bn_ref.make_fwd_operands, ACT = 0) with count = npix, and its reference over
    three launches (running statistics after each)"""
    c = B.FwdCase("br", s.C, s.npix, s.nslots, _k(s.npix), 0, False, train, None, "both", seed)
    o = B.make_fwd_operands(c)
    r = B.fwd_reference(c, o, 3)
    B.assert_fwd_conditions(c, o, r)
    return c, o, r


def fwd_case(s, form, relu, train, seed):
    c1, o1, r1 = fwd_operand(s, train, seed)
    k = types.SimpleNamespace(s=s, form=form, relu=relu, train=train, c=[c1], o=[o1], r=[r1], res=None)
    if form == "two":
        c2, o2, r2 = fwd_operand(s, train, seed + 1000)
        k.c.append(c2), k.o.append(o2), k.r.append(r2)
        z1 = o1.y * r1.scale + r1.shift
        z2 = o2.y * r2.scale + r2.shift
        assert B.on_grid(z1 + z2, 2.0 ** -5, 24), "z1 + z2 leaves the 2^-5 grid x 2^24"
        k.a_exact = fwd(o1.y, r1.scale, r1.shift, relu, o2.y, r2.scale, r2.shift)
    elif form == "res":
        g = torch.Generator().manual_seed(0xBE1 + seed)
        k.res = torch.randint(-32, 33, (s.npix, s.C), generator=g).to(F64)
        k.a_exact = fwd(o1.y, r1.scale, r1.shift, relu, res=k.res)
        assert B.on_grid(k.a_exact, 2.0 ** -5, 24)
    else:
        k.a_exact = fwd(o1.y, r1.scale, r1.shift, relu)
    k.a = B.bf16_rne(k.a_exact)
    if relu:
        assert bool((k.a_exact == 0).any()) and bool((k.a_exact > 0).any()), "the ReLU case clamps nothing / everything"
    return k


def bwd_case(s, form, relu, dres_mode, seed):
    """form one / two / res; dres_mode 0 absent, 1 overwritten, 2 accumulated (res only).  da, y and the statistics are
    bn_ref's integer family; a (the saved output) holds zeros, negatives and positives"""
    kk = _k(s.npix)
    mk = lambda sd: B.make_bwd_operands(B.BwdCase("br", s.C, s.npix, s.nslots, kk, 0, dres_mode, None, 1, 0, False, sd))
    o1 = mk(seed)
    g = torch.Generator().manual_seed(0xA5 + seed)
    a = torch.randint(-3, 4, (s.npix, s.C), generator=g).to(F64)
    assert bool((a == 0).any()) and bool((a < 0).any()) and bool((a > 0).any())
    dz = dz_of(o1.da, a, relu)
    k = types.SimpleNamespace(s=s, form=form, relu=relu, dres_mode=dres_mode, da=o1.da, a=a, dz=dz, o=[o1], count=o1.count,
                              dres0=o1.dres0, dres=None)
    if form == "two":
        o2 = mk(seed + 1000)
        o2.da = o1.da
        k.o.append(o2)
    k.r = []
    for o in k.o:
        # bn_ref's conditions with the masked gradient in da's place: the sums and every intermediate of THIS operand
        m = types.SimpleNamespace(**vars(o))
        m.da = dz
        cb = B.BwdCase("br", s.C, s.npix, s.nslots, kk, 0, 0, None, 1, 0, False, seed)
        B.assert_bwd_conditions(cb, m, B.bwd_reference(cb, m))
        s1, s2, dy = bwd_norm(dz, o.y, o.mean, o.invstd, o.gamma, float(o.count))
        k.r.append(types.SimpleNamespace(s1=s1, s2=s2, dy_exact=dy, dy=B.bf16_rne(dy), dgamma=s2, dbeta=s1))
    if dres_mode:
        d = bwd_res(dz, k.dres0 if dres_mode == 2 else None)
        assert B.on_grid(d, 1.0, 8)
        k.dres = d
    return k


def stats_case(s, seed):
    """an integer map: |x| <= 64, so a block's fp32 sums (at most 4096 pixels of one channel: < 2^24) and their fp64 total
    are exact in any order"""
    g = torch.Generator().manual_seed(0x57A7 + seed)
    x = torch.randint(-64, 65, (s.npix, s.C), generator=g).to(F64)
    assert s.npix * 64 * 64 < 2 ** 24
    return x
