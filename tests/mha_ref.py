"""Plain float64 reference of the attention core (csrc/mha.hip), an fp32 restatement of the kernels' arithmetic, and the
operand recipes / case table of tests/test_gpu_mha_exact.py.  Plain torch, CPU or device; nothing here needs a GPU.

Semantics (the header comment of mha.hip): O = softmax(scale Q K^T + key_padding_mask) V per (batch, head), head_dim 32, on
[L][B][E] operands; the softmax normaliser is taken BEFORE the attention-weight dropout (P is normalised over all live
keys, then multiplied by keep * drop_scale); dk = dv = 0 on padded keys; a query row whose keys are all padded gives O = 0,
lse = -inf and contributes nothing to any gradient.

The exact method.  A softmax is not exact on random data, but it is where the weights are dyadic:
  uniform  all scores 0 (Q = 0 or K = 0) and n = 2^k live keys: P = 1/n, O = sum V / n, every key weighs the same;
  gather   K rows are distinct +-1 codes, q_i is the code of a chosen live key, scale 64: the chosen key's score beats every
           other by >= 2 raw units = 184 in the exp2 domain, so every other weight underflows to exactly 0 in fp32 and
           O = V[chosen];
  dropout  uniform scores, 16 live keys, p = 0.5 (threshold 2^31, drop_scale 2): P keep drop_scale is 0 or 1/8.
With integer V / dO (and Q or K) every value a kernel rounds to bf16 on its way (P keep, dS) is representable in bf16 and
every fp32 sum is a sum of multiples of one unit with sum |terms| < 2^24 units, so ANY order of keys, chunks, waves and
blocks gives the float64 reference bit for bit (stored bf16 outputs: the reference rounded once).  assert_exact_conditions
checks these conditions on the float64 reference of a case before anything is launched."""
import collections
import math
import types

import torch

D = 32                    # head_dim
KC = 128                  # keys per chunk of the version-2 kernels
NEG = float("-inf")
LOG2E_F = float(torch.tensor(1.44269504088896341, dtype=torch.float32))
LN2_F = float(torch.tensor(0.69314718055994531, dtype=torch.float32))
UNIT = 4096.0             # every operand / intermediate of an exact case is a multiple of 1 / UNIT
# lse of the exact families: the normaliser is exact (l = n or 1, a power of two, so log2 l is an exact integer) and the
# kernel's value is fl(fl(fl(m sc2) + log2 l) ln2_f) with sc2 = scale log2e_f (exact: scale is a power of two).  Sources of
# error, in fp32 ulps of the result: the constants log2e_f and ln2_f (<= 1/2 each), the roundings of m sc2, of the sum and of
# the final product (<= 1/2 each; the first two vanish in the uniform families, where m = 0): <= 2.5 in the worst case.  On
# the exact cases themselves emulate_kernel is within 1 ulp everywhere (0.04 at worst, tests/test_mha_ref.py prints and
# asserts it); the tests allow 2: that 1 and one more for a device log2 / product whose last bit differs from the host's.
LSE_ULPS = 2


def heads(t, H):
    """[L][B][E] -> [B][H][L][32]"""
    L, B, E = t.shape
    assert E == H * D
    return t.reshape(L, B, H, D).permute(1, 2, 0, 3)


def rows(t):
    """[B][H][L][32] -> [L][B][E]"""
    B, H, L, _ = t.shape
    return t.permute(2, 0, 1, 3).reshape(L, B, H * D)


Ref = collections.namedtuple("Ref", "O O32 lse delta dq dk dv S P Pd dP dS")


def attention_reference(q, k, v, dout, mask, scale, H, keep=None, drop_scale=1.0, kill=None):
    """float64.  q, dout [Lq][B][E]; k, v [Lk][B][E]; mask bool / uint8 [B][Lk] (True = padded) or None; keep [B][H][Lq][Lk]
    (1 = the weight survives) or None.  kill: bool [B][H][Lq][Lk], scores removed on top of the mask (only the mutants of
    the tests use it).  Returns O, O32 (= O), dq [Lq][B][E]; dk, dv [Lk][B][E]; lse, delta [B][H][Lq]; and, as
    [B][H][Lq][Lk]: S (scaled scores, -inf where dead), P (softmax), Pd = P keep drop_scale, dP = (dO V^T) keep drop_scale,
    dS = P (dP - delta) (WITHOUT the factor scale, as the version-2 kernels round it)."""
    Q, K, V, DO = (heads(t.double(), H) for t in (q, k, v, dout))
    S = Q @ K.transpose(-1, -2) * scale
    if mask is not None:
        S = S.masked_fill(mask.bool()[:, None, None, :], NEG)
    if kill is not None:
        S = S.masked_fill(kill, NEG)
    m = S.amax(-1, keepdim=True)
    live = m > NEG
    e = torch.exp(S - torch.where(live, m, torch.zeros_like(m))) * live
    l = e.sum(-1, keepdim=True)
    P = e / torch.where(live, l, torch.ones_like(l))
    lse = torch.where(live, m + torch.log(torch.where(live, l, torch.ones_like(l))), torch.full_like(m, NEG)).squeeze(-1)
    kd = 1.0 if keep is None else keep.double() * drop_scale
    Pd = P * kd
    O = Pd @ V
    delta = (DO * O).sum(-1)
    dP = (DO @ V.transpose(-1, -2)) * kd
    dS = P * (dP - delta[..., None])
    dq = dS @ K * scale
    dk = dS.transpose(-1, -2) @ Q * scale
    dv = Pd.transpose(-1, -2) @ DO
    return Ref(rows(O), rows(O), lse, delta, rows(dq), rows(dk), rows(dv), S, P, Pd, dP, dS)


def bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


Emu = collections.namedtuple("Emu", "O O32 lse delta dq dk dv")


def emulate_kernel(q, k, v, dout, mask, scale, H, keep=None, drop_scale=1.0, o32=True):
    """fp32 restatement of the kernels' arithmetic with their bf16 rounding points (read off csrc/mha.hip; the backward's are
    the ones tools/attn_bwd_error.py writes down): P (after keep drop_scale) before P V, the normaliser from exactly those
    bf16 weights (no dropout) or from the fp32 weights before the drop; O stored bf16 and, separately, fp32; delta from the
    fp32 or the bf16 O; P recomputed from the saved lse; dS before its two products (without scale, which multiplies the
    accumulators); dq, dk, dv stored bf16.  The kernels work in the exp2 domain on chunks of 128 keys with the LAZY reference
    maximum (it moves when some score of a 16-query wave exceeds it by more than 8 / (scale log2 e)).  fp32 sums are taken
    in torch's order, not the MFMA's: the exact cases do not depend on it, the bounds of the numerics tests cover it."""
    f32 = torch.float32
    Q, K, V, DO = (heads(t.to(f32), H) for t in (q, k, v, dout))
    B, _, Lq, _ = Q.shape
    Lk = K.shape[2]
    dev = Q.device
    dead = torch.zeros(B, 1, 1, Lk, dtype=torch.bool, device=dev) if mask is None else mask.bool()[:, None, None, :]
    Sraw = (Q @ K.transpose(-1, -2)).masked_fill(dead, NEG)
    ks = torch.ones(1, 1, 1, 1, dtype=f32, device=dev) if keep is None else keep.to(f32) * drop_scale
    drop = keep is not None
    scale_t = torch.tensor(scale, dtype=f32, device=dev)
    sc2 = scale_t * LOG2E_F
    G = (Lq + 15) // 16
    Lp = G * 16
    Sp = torch.zeros(B, H, Lp, Lk, dtype=f32, device=dev).masked_fill(dead, NEG)
    Sp[:, :, :Lq] = Sraw
    ksp = ks
    if drop:
        ksp = torch.zeros(B, H, Lp, Lk, dtype=f32, device=dev)
        ksp[:, :, :Lq] = ks
    m_run = torch.full((B, H, Lp), NEG, dtype=f32, device=dev)
    oacc = torch.zeros(B, H, Lp, D, dtype=f32, device=dev)
    lacc = torch.zeros(B, H, Lp, dtype=f32, device=dev)
    one, zero = torch.ones((), dtype=f32, device=dev), torch.zeros((), dtype=f32, device=dev)
    step = KC
    for k0 in range(0, Lk, step):
        s = Sp[..., k0:k0 + step]
        mx = s.amax(-1)
        trig = (mx > m_run + 8.0 / sc2).view(B, H, G, 16).any(-1, keepdim=True).expand(B, H, G, 16).reshape(B, H, Lp)
        m_new = torch.where(trig, torch.maximum(m_run, mx), m_run)
        none = m_new == NEG
        dm = torch.where(none, zero, m_run - torch.where(none, zero, m_new))
        alpha = torch.where(trig & ~none, torch.exp2(dm * sc2), one)
        m_run = m_new
        mz = torch.where(none, zero, m_new)
        pe = torch.exp2(s * sc2 + (-mz * sc2)[..., None])
        pe = pe * ~none[..., None]
        pf = bf(pe * (ksp[..., k0:k0 + step] if drop else ks))
        oacc = oacc * alpha[..., None] + pf @ V[:, :, k0:k0 + step]
        lacc = lacc * alpha + (pe.sum(-1) if drop else pf.sum(-1))
    oacc, lacc, m_run = oacc[:, :, :Lq], lacc[:, :, :Lq], m_run[:, :, :Lq]
    some = lacc > 0
    inv = torch.where(some, 1.0 / torch.where(some, lacc, one), zero)
    O32 = oacc * inv[..., None]
    O = bf(O32)
    ml = torch.where(some, m_run, zero)
    ll = torch.log2(torch.where(some, lacc, one))
    lse = torch.where(some, (ml * sc2 + ll) * LN2_F, torch.full_like(ml, NEG))
    # ---- backward
    delta = (DO * (O32 if o32 else O)).sum(-1)
    lz = torch.where(some, lse, zero)
    pe = torch.exp2(Sraw * sc2 + (-lz * LOG2E_F)[..., None])
    pe = pe * some[..., None]
    dp = DO @ V.transpose(-1, -2)
    ds = pe * (dp * ks - delta[..., None])
    pf = bf(pe * ks)
    ds = bf(ds)
    dq = bf((ds @ K) * scale_t)
    dk = bf((ds.transpose(-1, -2) @ Q) * scale_t)
    dv = bf(pf.transpose(-1, -2) @ DO)
    return Emu(rows(O), rows(O32), lse, delta, rows(dq), rows(dk), rows(dv))


# ------------------------------------------------------------------------------------------------------------ comparing
def ulp32(x):
    """the fp32 unit in the last place at |x| (float64 tensor)"""
    a = x.abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def lse_mismatch(got, ref, ulps=LSE_ULPS):
    """rows whose lse is not within `ulps` fp32 ulps of the reference (-inf must be -inf, 0 must be 0)"""
    got, ref = got.double(), ref.double()
    fin = torch.isfinite(ref)
    ok = torch.where(fin, (got - torch.where(fin, ref, torch.zeros_like(ref))).abs() <= ulps * ulp32(ref) * (ref != 0), got == ref)
    return int((~ok).sum())


def exact_mismatches(got, ref, forward_only=False, lse_ulps=LSE_ULPS):
    """names of the tensors of `got` (O, O32, lse, delta, dq, dk, dv; None = not produced) that differ from the float64
    reference rounded ONCE to the stored type (lse: beyond lse_ulps)"""
    bad = []
    names = ("O", "O32", "lse") if forward_only else ("O", "O32", "lse", "delta", "dq", "dk", "dv")
    for n in names:
        g, r = getattr(got, n), getattr(ref, n)
        if g is None:
            continue
        if n == "lse":
            if lse_mismatch(g, r, lse_ulps):
                bad.append(n)
        elif n in ("O32", "delta"):
            if not torch.equal(g.float(), r.float()):
                bad.append(n)
        elif not torch.equal(g.to(torch.bfloat16), r.to(torch.bfloat16)):
            bad.append(n)
    return bad


FROB_TOL = {"O": 1e-2, "dq": 2e-2, "dk": 2e-2, "dv": 2e-2}     # tests/test_gpu_detr.py::test_mha_core_fwd_bwd (the dropout test: 2e-2 / 3e-2)


def frobenius_pass(got, ref, names=("O", "dq", "dk", "dv")):
    """the criterion of the older attention tests, |got - ref| < tol |ref| in the Frobenius norm per tensor, at the tighter
    of their tolerances; returns (passes, {name: ratio})"""
    rat = {}
    for n in names:
        g, r = getattr(got, n).double(), getattr(ref, n).double()
        d, nr = float((g - r).norm()), float(r.norm())
        if nr < 1e-9:           # a reference that is zero but for float64 rounding (the gather family's dq, dk): equal or not
            rat[n] = 0.0 if d < 1e-9 else float("inf")
        else:
            rat[n] = d / nr
    return all(rat[n] < FROB_TOL[n] for n in names), rat


# ------------------------------------------------------------------------------------------------------------ the cases
def mirror_waves(L, BH, ncu):
    """mha2_waves of csrc/mha.hip: waves (16 rows each) per block of a version-2 kernel"""
    gq = -(-L // 16)
    nwv = -(-gq * BH // ncu)
    nwv = min(max(nwv, 4), 12)
    if nwv > gq:
        nwv = 4 if gq < 4 else gq
    return nwv


def length_for_waves(w, BH, ncu):
    """the smallest L = 16 g - 5 (not a multiple of 16: a ragged last group) at which mirror_waves gives w"""
    for g in range(1, 400):
        if mirror_waves(16 * g - 5, BH, ncu) == w:
            return 16 * g - 5
    raise AssertionError((w, BH, ncu))


Case = collections.namedtuple("Case", "name family B H Lq Lk live zero scale o32 ld lse_null seed")
# ld: 'E' (dense), 'packed' (q and k are the two halves of one [T, 2E] buffer: ldq = ldk = 2E, k = q + E; Lq == Lk),
# 'wide' / 'wide2' (two unrelated wider strides).  live: live keys per image (0 = a fully masked image) or None = no mask.
# zero: which of Q / K is zero (uniform, dropout).  lse_null: the forward-only launch passes lse = NULL.
LDS = {"E": (0, 0), "wide": (8, 24), "wide2": (None, 40)}     # extra columns of q / k rows (None: E + 16 extra)


def strides(c):
    E = c.H * D
    if c.ld == "packed":
        return 2 * E, 2 * E
    a, b = LDS[c.ld]
    return E + (E + 16 if a is None else a), E + b


def _live(family, B, Lk, full_masked=None):
    if family == "uniform":
        n0 = 1 << (Lk.bit_length() - 1)
        lv = [max(1, n0 >> (b % 3)) for b in range(B)]
    elif family == "gather":
        lv = [max(1, (Lk - Lk // 7) >> (b % 3)) for b in range(B)]
    else:
        lv = [min(16, 1 << (Lk.bit_length() - 1))] * B
    if full_masked is not None and full_masked < B:
        lv[full_masked] = 0
    return tuple(lv)


def exact_cases(ncu=256):
    """the case table of tests/test_gpu_mha_exact.py for a device of ncu compute units: (sweep, extras).  sweep[family] is
    nine cases at B x H = 5 x 32 whose Lq / Lk give the forward and dQ kernels (by Lq) and the dK/dV kernel (by Lk) every
    wave count 4 .. 12; extras are the small shapes and parameter variants."""
    sweep = {}
    B, H = 5, 32
    lds = ["E", "wide", "E", "wide2"]
    for fi, fam in enumerate(("uniform", "gather", "dropout")):
        cs = []
        for w in range(4, 13):
            Lq, Lk = length_for_waves(w, B * H, ncu), length_for_waves(16 - w, B * H, ncu)
            cs.append(Case(f"{fam}-w{w}", fam, B, H, Lq, Lk, _live(fam, B, Lk, 3 if w % 2 else None), "qk"[(w + fi) % 2],
                           64.0 if fam == "gather" else 2.0 ** -(w % 4), w % 3 != 0, lds[(w + fi) % 4], w == 5, 100 * fi + w))
        sweep[fam] = cs
    Bc = ncu // 32 + 1            # B x 32 heads > ncu: nwv = ceil(gq B H / ncu) > gq >= 4 -> clamped to gq
    ex = []
    for fi, fam in enumerate(("uniform", "gather", "dropout")):
        sc = 64.0 if fam == "gather" else 0.25
        s0 = 1000 + 100 * fi
        nm = (16,) if fam == "dropout" else None
        ex += [
            Case(f"{fam}-L1", fam, 1, 1, 1, 1, None, "q", sc, True, "E", False, s0 + 1),
            Case(f"{fam}-Lk20", fam, 2, 3, 40, 20, (16, 8) if fam != "gather" else (13, 5), "k", sc, True, "wide", False, s0 + 2),
            Case(f"{fam}-Lk129", fam, 2, 8, 77, 129, _live(fam, 2, 129), "q", sc, False, "wide2", False, s0 + 3),
            Case(f"{fam}-Lk257-packed", fam, 2, 8, 257, 257, _live(fam, 2, 257, 1), "k", sc, True, "packed", True, s0 + 4),
            Case(f"{fam}-clamp", fam, Bc, 32, 75, 75, _live(fam, Bc, 75), "q", sc, True, "E", False, s0 + 5),
            # no mask (the dropout family needs its 16 live keys: there the mask stays)
            Case(f"{fam}-nomask-H1", fam, 1, 1, 100, 256, nm and nm * 1, "k", sc, False, "E", False, s0 + 6),
            Case(f"{fam}-nomask-packed", fam, 2, 3, 128, 128, nm and nm * 2, "q", sc, True, "packed", False, s0 + 7),
        ]
    return sweep, ex


def mutation_cases():
    """where the mutants are judged: Lk = 16 g + 1, so that the ragged last group of the
    dK/dV kernel is one key - the smallest thing it can leave unwritten - and B x H x Lq = 63200 query rows, so that one wholly
    wrong row (the gather family's dropped key) is 0.6 % of the output's norm"""
    out = []
    for fi, fam in enumerate(("uniform", "gather", "dropout")):
        sc = 64.0 if fam == "gather" else 0.5
        out += [Case(f"mut-{fam}", fam, 5, 32, 395, 193, _live(fam, 5, 193), "q", sc, True, "E", False, 3000 + fi)]
    return out


def make_mask(B, Lk, live, g):
    """bool [B][Lk], True = padded: live[b] live keys, scattered; by image in turn: anywhere / behind a run of leading masked
    keys / with the whole chunk [128, 256) masked / with the whole first chunk masked (where the shape has the room)"""
    if live is None:
        return None
    m = torch.ones(B, Lk, dtype=torch.bool)
    for b, n in enumerate(live):
        ok = torch.ones(Lk, dtype=torch.bool)
        kind = b % 4
        if kind == 1 and Lk - n >= 1:
            ok[:min(Lk - n, max(1, Lk // 5))] = False
        elif kind == 2 and Lk > 256 and Lk - 128 >= n:
            ok[128:256] = False
        elif kind == 3 and Lk > 128 and Lk - 128 >= n:
            ok[:128] = False
        idx = ok.nonzero().flatten()
        assert len(idx) >= n
        idx = idx[torch.randperm(len(idx), generator=g)]
        if kind == 0 and n >= -(-Lk // KC):         # the last key and one key of every other chunk are live: move them to the front
            lead = [Lk - 1] + [int(idx[(idx // KC == ch).nonzero()[0, 0]]) for ch in range((Lk - 1) // KC)]
            idx = torch.tensor(lead + [int(i) for i in idx if int(i) not in lead], dtype=torch.long)
        m[b, idx[:n]] = False
    return m


def make_operands(c):
    """float64 CPU operands of a case: q, dout [Lq][B][E]; k, v [Lk][B][E] (v: the backward's values, v_fwd: the values of
    the forward-only launch - the same except in the uniform family); mask; sel (gather: the chosen key [B][H][Lq])"""
    g = torch.Generator().manual_seed(c.seed)
    B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
    E = H * D
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).double()
    mask = make_mask(B, Lk, c.live, g)
    livem = torch.ones(B, Lk, dtype=torch.bool) if mask is None else ~mask
    sel = None
    if c.family == "gather":
        codes = ri(0, 1, B, H, Lk, D) * 2 - 1
        sel = torch.zeros(B, H, Lq, dtype=torch.long)
        nch = -(-Lk // KC)
        for b in range(B):
            lv = livem[b].nonzero().flatten()
            if len(lv) == 0:
                sel[b] = torch.randint(0, Lk, (H, Lq), generator=g)
                continue
            first, last = lv[lv < KC], lv[lv >= KC * (nch - 1)]
            pools = [first if len(first) else lv, last if len(last) else lv, lv]
            for r in range(3):
                n = len(range(r, Lq, 3))
                sel[b, :, r::3] = pools[r][torch.randint(0, len(pools[r]), (H, n), generator=g)]
        Qh = torch.gather(codes, 2, sel[..., None].expand(B, H, Lq, D))
        q, k = rows(Qh), rows(codes)
        v = ri(-100, 100, Lk, B, E)
        dout = ri(-2, 2, Lq, B, E)
        v_fwd = v
    else:
        q = torch.zeros(Lq, B, E, dtype=torch.float64) if c.zero == "q" else ri(-3, 3, Lq, B, E)
        k = torch.zeros(Lk, B, E, dtype=torch.float64) if c.zero == "k" else ri(-3, 3, Lk, B, E)
        if c.family == "uniform":
            v_fwd = ri(-9, 9, Lk, B, E)
            v = torch.zeros(Lk, B, E, dtype=torch.float64)
            for b in range(B):                      # live rows: a random permutation of r and -r, so that O = delta = 0
                lv = livem[b].nonzero().flatten()
                n = len(lv)
                if n >= 2:
                    half = ri(-3, 3, n // 2, E)
                    both = torch.cat([half, -half, torch.zeros(n % 2, E, dtype=torch.float64)])
                    v[lv, b] = both[torch.randperm(n, generator=g)]
            dout = ri(-1, 1, Lq, B, E)
        else:
            v = ri(-1, 1, Lk, B, E)
            v_fwd = v
            dh = torch.zeros(Lq, B, H, D, dtype=torch.float64)          # two non-zero entries per (query, head) row
            pos = torch.rand(Lq, B, H, D, generator=g).argsort(-1)[..., :2]
            dh.scatter_(-1, pos, ri(0, 1, Lq, B, H, 2) * 2 - 1)
            dout = dh.reshape(Lq, B, E)
    if mask is not None:                            # a leak of a padded key must show: a large finite value (NaN would not
        pad = mask.t()[:, :, None].expand(Lk, B, E)  # do: the kernels multiply a zero weight by these rows)
        v = torch.where(pad, torch.full_like(v, 100.0), v)
        v_fwd = torch.where(pad, torch.full_like(v_fwd, 100.0), v_fwd)
    return types.SimpleNamespace(q=q, k=k, v=v, v_fwd=v_fwd, dout=dout, mask=mask, sel=sel)


def random_keep(c, device="cpu"):
    """a stand-in keep mask for the CPU checks (the GPU tests take the device's own from mi_mha_dropout_mask)"""
    g = torch.Generator().manual_seed(7 + c.seed)
    return (torch.rand(c.B, c.H, c.Lq, c.Lk, generator=g) < 0.5).to(torch.uint8).to(device)


def _is_bf16(x):
    x = x.float().double()                          # (a float64 weight below fp32's range IS 0 in every kernel: see gather)
    return bool((x.to(torch.bfloat16).double() == x).all())


def _units(x):
    x = x.float().double() * UNIT
    return bool((x == x.round()).all())


def assert_exact_conditions(c, ops, ref, forward_only=False):
    """the conditions of the method on the float64 reference `ref` of case c (operands ops; ref of v_fwd if forward_only)"""
    H = c.H
    assert math.log2(c.scale) == round(math.log2(c.scale)), "scale must be a power of two"
    v = ops.v_fwd if forward_only else ops.v
    Q, K, V, DO = (heads(t.to(ref.P.device), H).abs() for t in (ops.q, ops.k, v, ops.dout))
    lim = 2.0 ** 24 / UNIT
    assert _is_bf16(ref.Pd) and _units(ref.Pd), "P keep drop_scale must be representable in bf16"
    assert float((Q @ K.transpose(-1, -2)).max()) < 2 ** 24
    assert float((ref.Pd.float().double().abs() @ V).max()) < lim and _units(ref.O32), "O: fp32 sums of dyadic terms"
    if c.family == "gather":
        # the best score beats the rest by >= 2 raw units: > 150 in the exp2 domain, so every other fp32 weight is exactly
        # 0, and above the lazy maximum's slack, so the version-2 forward's reference maximum is always the true one
        S = ref.S
        top = S.topk(min(2, S.shape[-1]), -1).values
        lv = top[..., 0] > NEG
        if S.shape[-1] > 1:
            gap = (top[..., 0] - top[..., 1])[lv & (top[..., 1] > NEG)] / c.scale
            assert gap.numel() == 0 or float(gap.min()) >= 2.0
        assert 2.0 * c.scale * LOG2E_F > 160 and 8.0 / (c.scale * LOG2E_F) < 2.0
        assert bool((ref.Pd.float()[lv].amax(-1) == 1).all())
    else:
        assert float(ref.S[ref.S > NEG].abs().max()) == 0 if bool((ref.S > NEG).any()) else True
    if forward_only:
        return
    assert _is_bf16(ref.dS) and _units(ref.dS), "dS must be representable in bf16"
    assert _is_bf16(ref.P), "the recomputed P must be representable in bf16"
    assert float((DO @ V.transpose(-1, -2)).max()) < 2 ** 24
    assert _units(ref.delta) and float((DO * heads(ref.O32, H).abs()).sum(-1).max()) < lim
    if c.family == "uniform":
        assert float(ref.O.abs().max()) == 0 and float(ref.delta.abs().max()) == 0
    dSa, Pda = ref.dS.float().double().abs(), ref.Pd.float().double().abs()
    assert float((dSa @ K).max()) < lim and float((dSa.transpose(-1, -2) @ Q).max()) < lim
    assert float((Pda.transpose(-1, -2) @ DO).max()) < lim


def reference_of(c, ops, keep=None, forward_only=False, kill=None, mask=None, device="cpu"):
    """the float64 reference of a case on `device` (keep: uint8 [B][H][Lq][Lk] for the dropout family)"""
    v = ops.v_fwd if forward_only else ops.v
    mk = ops.mask if mask is None else mask
    d = lambda t: None if t is None else t.to(device)
    if c.family == "dropout":
        assert keep is not None
    return attention_reference(d(ops.q), d(ops.k), d(v), d(ops.dout), d(mk), c.scale, c.H,
                               keep=d(keep) if c.family == "dropout" else None, drop_scale=2.0 if c.family == "dropout" else 1.0,
                               kill=d(kill))


def emulation_of(c, ops, keep=None, forward_only=False, device="cpu"):
    v = ops.v_fwd if forward_only else ops.v
    d = lambda t: None if t is None else t.to(device)
    return emulate_kernel(d(ops.q), d(ops.k), d(v), d(ops.dout), d(ops.mask), c.scale, c.H,
                          keep=d(keep) if c.family == "dropout" else None, drop_scale=2.0 if c.family == "dropout" else 1.0,
                          o32=c.o32)


# ------------------------------------------------------------------------------------------------------------ mutants
def mutants(c, ops, ref, keep=None, device="cpu", forward_only=False):
    """[(name, mutated float64 reference)] of case c: what a kernel wrong at ONE index would give.
      drop_key       one live key (gather: the chosen one, of a row whose runner-up is unique) missing from one query row;
      mask_boundary  the mask boundary moved by one key - a live key next to a padded one taken as padded - for one 16-query
                     group of one head (the reach of one wave's index error);
      keep_shift     one query row's keep bits taken from the neighbouring element (dropout family);
      dv_group       one head's dv rows of the ragged last 16-key group left zero;
      lse_off        lse of one row off by 2^-6.
    A dropped low-weight key of a random-data case is NOT here: a weight of 1e-3 sits under the 2^-8 rounding term of the
    bounds of the numerics tests, which therefore cannot see it - that mutant belongs to the exact families only.
    forward_only: mutants of the forward-only launch (v_fwd; the uniform family's backward operands make O = 0, so its O is
    judged there); compare them with forward_only = True."""
    B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
    out = []
    b = 0
    h = H // 2
    livem = torch.ones(Lk, dtype=torch.bool) if ops.mask is None else ~ops.mask[b]
    lv = livem.nonzero().flatten()
    i = min(Lq - 1, 21)
    if c.family == "gather":
        S = ref.S[b, h].cpu()
        top = S.topk(3, -1).values
        good = (top[:, 1] > top[:, 2]).nonzero().flatten()
        i = int(good[len(good) // 2])
        j = int(ops.sel[b, h, i])
    else:
        j = int(lv[len(lv) // 2])
    kill = torch.zeros(B, H, Lq, Lk, dtype=torch.bool)
    kill[b, h, i, j] = True
    out.append(("drop_key", reference_of(c, ops, keep, forward_only=forward_only, kill=kill, device=device)))
    if ops.mask is not None:
        edge = (livem[1:] & ~livem[:-1]).nonzero().flatten() + 1        # live keys whose left neighbour is padded
        if c.family == "gather":
            chosen = set(ops.sel[b, h, :16].tolist())
            edge = torch.tensor([int(e) for e in edge if int(e) in chosen], dtype=torch.long)
            if len(edge) == 0:                                           # take a chosen key of the group: a boundary moved INTO it
                edge = torch.tensor([int(ops.sel[b, h, 3])])
        kill = torch.zeros(B, H, Lq, Lk, dtype=torch.bool)
        kill[b, h, :16, int(edge[0])] = True
        out.append(("mask_boundary", reference_of(c, ops, keep, forward_only=forward_only, kill=kill, device=device)))
    if c.family == "dropout":
        k2 = keep.clone()
        k2[b, h, i] = torch.roll(keep[b, h, i], 1)
        out.append(("keep_shift", reference_of(c, ops, k2, forward_only=forward_only, device=device)))
    r0 = (Lk - 1) // 16 * 16
    dv = ref.dv.clone()
    bb = [x for x in range(B) if float(dv[r0:, x, h * D:(h + 1) * D].abs().max()) > 0][0]     # an image where they are not 0 anyway
    dv[r0:, bb, h * D:(h + 1) * D] = 0
    out.append(("dv_group", ref._replace(dv=dv)))
    lse = ref.lse.clone()
    lse[b, h, i] += 2.0 ** -6
    out.append(("lse_off", ref._replace(lse=lse)))
    return out


def check_mutants(c, ops, keep, result_of, device="cpu"):
    """result_of(forward_only) -> the correct result (the emulation's here, the kernels' on the device).  Every mutant must
    differ from it in the exact comparison AND be accepted by the Frobenius criterion of the older tests at their tighter
    tolerances (FROB_TOL): the error a norm cannot see.  The uniform family's backward operands give O = 0, so O is judged on the
    forward-only launch and the gradients on the other; elsewhere one launch serves both."""
    seen = set()
    for fwd in ((True, False) if c.family == "uniform" else (False,)):
        ref = reference_of(c, ops, keep, forward_only=fwd, device=device)
        got = result_of(fwd)
        assert exact_mismatches(got, ref, forward_only=fwd) == [], (c.name, "the unmutated reference must match")
        names = ("O",) if fwd else (("dq", "dk", "dv") if c.family == "uniform" else ("O", "dq", "dk", "dv"))
        for name, mut in mutants(c, ops, ref, keep, device=device, forward_only=fwd):
            if fwd and name == "dv_group":
                continue
            diff = exact_mismatches(got, mut, forward_only=fwd)
            ok, rat = frobenius_pass(got, mut, names=names)
            print(c.name, "forward" if fwd else "backward", name, diff, {k: "%.1e" % v for k, v in rat.items()})
            assert diff != [], (c.name, name, "the exact comparison must reject this mutant")
            assert ok, (c.name, name, rat, "the Frobenius criterion of the older tests must accept this mutant")
            seen.add(name)
    want = {"drop_key", "dv_group", "lse_off"} | ({"mask_boundary"} if ops.mask is not None else set())
    assert seen == want | ({"keep_shift"} if c.family == "dropout" else set()), seen


# ------------------------------------------------------------------------------------------------------------ numerics
U16 = 2.0 ** -8           # unit roundoff of bf16: 8 significant bits, round to nearest -> |fl(x) - x| <= 2^-8 |x|
U32 = 2.0 ** -24          # unit roundoff of fp32
NSCALE = D ** -0.5
# V and dO are Gaussian about a common part of one standard deviation.  An element of O = sum_j P_ij v_j or of dv = sum_i P_ij dO_i
# over zero-mean values is a sum that cancels to ~ 1 / sqrt(n) of its terms while every rounding of the row can align: a
# worst-case elementwise bound is then several per cent of a typical element whatever the kernel does (4.7e-3 sqrt(n_eff) of
# |O|: 2e-2 .. 9e-2 at these shapes), and says nothing relative.  With the common part |O| ~ |dv| / sum_i P_ij ~ 1, the bounds
# themselves (u sum_j P_ij |v_j - O_i|, 2 u sum_i P_ij |dO_i|) keep their size, and bound / |value| is ~ u (0.8 + 1) = 7e-3 for
# O and ~ u (2 x 1.17 + 1) = 1.3e-2 for dv: the elementwise statement is then tighter than the 2e-2 of the older norm test.
VMEAN = 1.0
NCase = collections.namedtuple("NCase", "name B H Lq Lk kind o32 seed")


def numerics_cases():
    """random data, scale 1/sqrt(32), scattered / leading / whole-chunk masks (make_mask), three key chunks, three query
    blocks: Gaussian operands (V and dO about a common part, see VMEAN); peaked scores (Q, K x 3); keys ordered so that the reference maximum rises in every chunk
    (by more than the lazy maximum's slack) or never moves after the first; the "alike values" regime of
    tests/test_gpu_detr.py (a common part far above the per-key part of V: dS is a small difference of large numbers); and
    the Gaussian case with delta taken from the bf16 O (o_f32 = NULL)"""
    return [NCase("gauss", 2, 8, 150, 300, "gauss", True, 1), NCase("peaked", 2, 8, 150, 300, "peaked", True, 2),
            NCase("rising", 2, 3, 150, 300, "rising", True, 3), NCase("falling", 2, 3, 150, 300, "falling", True, 4),
            NCase("alike", 2, 8, 100, 300, "alike", True, 5), NCase("gauss-bf16-O", 3, 3, 77, 200, "gauss", False, 6)]


def make_numerics_operands(nc):
    g = torch.Generator().manual_seed(500 + nc.seed)
    B, H, Lq, Lk = nc.B, nc.H, nc.Lq, nc.Lk
    E = H * D
    rn = lambda n: torch.randn(n, B, E, generator=g)
    q, k, v, do = rn(Lq), rn(Lk), rn(Lk) + VMEAN, rn(Lq) + VMEAN
    if nc.kind == "peaked":
        q, k = q * 3, k * 3
    elif nc.kind in ("rising", "falling"):          # score ~ scale * 32 * 1.5 * a_j: a ramp of 24 nats over the keys
        ramp = torch.linspace(0, 1, Lk) if nc.kind == "rising" else torch.linspace(1, 0, Lk)
        q = 0.5 * q + 1.5
        k = 0.5 * k + (24.0 / (1.5 * 32 * 32 ** -0.5)) * ramp[:, None, None]
    elif nc.kind == "alike":
        q, k = q * 0.3, k * 0.3
        v = torch.randn(1, B, E, generator=g) + 0.008 * (v - VMEAN)
    mask = make_mask(B, Lk, tuple(Lk - Lk // (3 + b) for b in range(B)), g)
    bfd = lambda t: t.to(torch.bfloat16).double()
    return types.SimpleNamespace(q=bfd(q), k=bfd(k), v=bfd(v), v_fwd=bfd(v), dout=bfd(do), mask=mask, sel=None)


def error_bounds(ref, q, k, v, dout, scale, H, o32=True):
    """First-order, worst-case elementwise error bounds of the version-2 kernels (no dropout) against the float64 reference
    `ref`, from the reference's own intermediates.  Constants: u = 2^-8 (bf16), e = 2^-24 (fp32); nothing is fitted.  One term
    per rounding point of csrc/mha.hip:

    scores and weights.  The kernel forms p^_ij = bf16(exp2(fma(s_ij, sc2, -m sc2))) with s the 32-term fp32 MFMA sum.  In
    natural-log units the argument is off by  e (32 scale A_ij + 8 Smax_i + 2),  A_ij = sum_d |q_id k_jd|, Smax_i = max_j
    |S_ij|: the accumulation of s (31 e sum |terms|), the constant sc2 (its rounding and log2e's, coherent over (s - m):
    2 e |S - M| <= 4 e Smax), the rounding of -m sc2 (e Smax; the lazy maximum is some |S_ij| of the row), the fma's own
    rounding (e |S - m| <= 2 e Smax) and the hardware exp2 (2 e).  Call it h_ij.  The bf16 rounding of the weight adds u:
        p^_ij = p_ij (1 + eta_ij),  |eta_ij| <= u + h_ij.     (the lazy maximum only scales a row: O and l carry the same factor)
    O.  The normaliser sums exactly the bf16 weights that entered P V, so dO_i = sum_j P_ij eta_ij (v_j - O_i):
        B_O32 = sum_j P_ij (u + h_ij) |v_jd - O_id| + c (sum_j P_ij |v_jd| + |O_id|) + 3 e |O_id|
    with c = (Lk + 16) e the fp32 accumulation of Lk terms in any order plus the rescales by alpha, and 3 e the reciprocal, the
    product and the fp32 store.  B_O = B_O32 + u |O| (the bf16 store).
    lse = (m sc2 + log2 l^) ln2:  l^ = l (1 + sum_j P_ij eta_ij), so
        B_lse = u + sum_j P_ij h_ij + c + e (4 |LSE_i| + 4 Smax_i + 4)
    (the last: the roundings of m sc2, of the sum and of the product, the constant ln2 and the hardware log2).
    delta_i = sum_d dO_id O^_id from o_f32, or from the bf16 O when it is NULL:
        B_delta = sum_d |dO_id| B_O^,id + 33 e sum_d |dO_id O_id|.
    The backward recomputes P~_ij = exp2(fma(s_ij, sc2, -lse log2e)) = P_ij (1 + r_ij) with
        |r_ij| <= B_lse,i + h_ij + 2 e |LSE_i|      (the lse error enters every weight of the row coherently)
    dP_ij = sum_d dO_id v_jd - delta_i in the MFMA (33 e sum_d |dO_id v_jd| =: B_dP), and dS~ = bf16(P~ (dP - delta)):
        B_dS = |dS_ij| (r_ij + u + 2 e) + P_ij (B_delta,i + B_dP,ij)
        B_dq = scale (sum_j B_dS,ij |k_jd| + c sum_j |dS_ij k_jd|) + (u + 2 e) |dq_id|
        B_dk = scale (sum_i B_dS,ij |q_id| + c' sum_i |dS_ij q_id|) + (u + 2 e) |dk_jd|,     c' = (Lq + 16) e
        B_dv = sum_i P_ij (r_ij + u) |dO_id| + c' sum_i P_ij |dO_id| + u |dv_jd|             (bf16(P~) enters P^T dO)
    Every bound gets + 1e-30 for results below the normal range (flushed weights).  Second-order terms (u^2 = 4e-6 relative)
    are not included.  A dropped key of weight 1e-3 moves O by 1e-3 |v - O| < u sum_j P_ij |v_j - O_i|: these bounds cannot
    see it, which is why that mutant belongs to the exact families."""
    Q, K, V, DO = (heads(t.double(), H) for t in (q, k, v, dout))
    P, S, dS = ref.P, ref.S, ref.dS
    Lq, Lk = P.shape[-2:]
    u, e = U16, U32
    c, c2 = (Lk + 16) * e, (Lq + 16) * e
    live = S > NEG
    Sab = torch.where(live, S.abs(), torch.zeros_like(S))
    Smax = Sab.amax(-1, keepdim=True)
    A = Q.abs() @ K.abs().transpose(-1, -2)
    h = e * (32 * scale * A + 8 * Smax + 2)
    W = P * (u + h)
    O = heads(ref.O, H)
    LSE = torch.where(torch.isfinite(ref.lse), ref.lse, torch.zeros_like(ref.lse))[..., None].abs()
    dev = (V[:, :, None, :, :] - O[:, :, :, None, :]).abs()                  # [B][H][Lq][Lk][32]
    B_O32 = (W[..., None] * dev).sum(-2) + c * (P @ V.abs() + O.abs()) + 3 * e * O.abs()
    B_O = B_O32 + u * O.abs()
    B_lse = u + (P * h).sum(-1, keepdim=True) + c + e * (4 * LSE + 4 * Smax + 4)
    B_delta = (DO.abs() * (B_O32 if o32 else B_O)).sum(-1, keepdim=True) + 33 * e * (DO * O).abs().sum(-1, keepdim=True)
    r = B_lse + h + 2 * e * LSE
    B_dP = 33 * e * (DO.abs() @ V.abs().transpose(-1, -2))
    B_dS = dS.abs() * (r + u + 2 * e) + P * (B_delta + B_dP)
    dq, dk, dv = heads(ref.dq, H), heads(ref.dk, H), heads(ref.dv, H)
    B_dq = scale * (B_dS @ K.abs() + c * (dS.abs() @ K.abs())) + (u + 2 * e) * dq.abs()
    B_dk = scale * (B_dS.transpose(-1, -2) @ Q.abs() + c2 * (dS.abs().transpose(-1, -2) @ Q.abs())) + (u + 2 * e) * dk.abs()
    B_dv = (P * (r + u)).transpose(-1, -2) @ DO.abs() + c2 * (P.transpose(-1, -2) @ DO.abs()) + u * dv.abs()
    t = 1e-30
    return dict(O=rows(B_O) + t, O32=rows(B_O32) + t, lse=B_lse.squeeze(-1) + t, delta=B_delta.squeeze(-1) + t,
                dq=rows(B_dq) + t, dk=rows(B_dk) + t, dv=rows(B_dv) + t)


def bound_ratios(got, ref, bounds):
    """{tensor: (max |got - ref| / bound, median bound / |ref|)}; lse = -inf must be -inf (ratio 0) and nothing may be NaN"""
    out = {}
    for n, bd in bounds.items():
        g = getattr(got, n)
        if g is None:
            continue
        g, r = g.double(), getattr(ref, n).double()
        fin = torch.isfinite(r)
        assert bool((g[~fin] == r[~fin]).all()) and bool(torch.isfinite(g[fin]).all()), n
        err = (g[fin] - r[fin]).abs() / bd[fin]
        nz = fin & (r != 0)
        out[n] = (float(err.max()), float((bd[nz] / r[nz].abs()).median()))
    return out
