"""Reference of the SMCA attention core (csrc/mha.hip, PRIOR instantiations; modeling/smca.py): float64, and an fp32
restatement with the kernels' bf16 rounding points; the integer recipe that fills the parameters and inputs of the fixture
tests/golden/smca.npz (tools/gen_smca_golden.py loads it into the reference's modules, the tests into ours); and the operand
recipes of tests/test_gpu_smca_exact.py.  Plain torch on the CPU; nothing here needs a GPU.

    logit[q][key] = scale Q[q].K[key] + (mask[key] ? -inf : 0) + G[q][key]
    G[q][key]     = -| a dx^2 + b dy^2 + c dx^2 dy^2 | inv_smooth,   dx = px - key % W,  dy = py - key // W
    O = (softmax(logit) keep drop_scale) V

point [Lq][B][H][2] = (px, py), coef [Lq][B][H][3] = (a, b, c).  d|x|/dx = sign(x), 0 at 0.  With dS = P (dP - delta) the
gradient of the logits, w = dS sign(x):
    dcoef  = -inv_smooth sum_key w {dx^2, dy^2, dx^2 dy^2}
    dpoint = -2 inv_smooth sum_key w {dx (a + c dy^2), dy (b + c dx^2)}

The exact families (conditions asserted by the functions below before anything is launched; scale and inv_smooth are powers
of two there):
  uniform      Q = 0 and coefficients that are 0, or 2^-100 (the prior is then far below one fp32 ulp of the normaliser:
               numerically absent from the logits, but its sign is +1 where a zero coefficient has sign(0) = 0 and, as torch,
               no coefficient gradient at all), n = 2^k live keys: P = 1/n.  The backward recomputes P from the stored lse:
               exp2(-fl(fl(k ln2_f) log2e_f)), exactly 2^-k for the k used here (asserted).  Every term of the three
               coefficient sums is a multiple of one unit with sum |terms| < 2^24 units, so any order gives the float64 sum.
  gather       Q = 0, the point ON a live grid cell, coefficients so large that every other weight underflows to 0: one-hot.
  equidistant  the four live keys of the 2 x 2 block around a half-integer point, a = b: P = 1/4 with a nonzero maximum.
"""
import zlib

import numpy as np
import torch

import mha_ref as M

HD = 32
NEG = float("-inf")
TYPES = ("type1", "type2", "type3", "type4")
CORE_OUT = ("O", "dq", "dk", "dv", "dpoint", "dcoef")


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-300))


def rel_max(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-300))


# ------------------------------------------------------------------ the core
def prior_terms(point, coef, map_hw, dtype):
    """dx, dy, dx^2, dy^2, a, b, c as [B][H][Lq][Lk] (a, b, c: [B][H][Lq][1]) and x = a dx^2 + b dy^2 + c dx^2 dy^2"""
    Hm, W = map_hw
    key = torch.arange(Hm * W)
    kx, ky = (key % W).to(dtype), (key // W).to(dtype)
    p, c = point.to(dtype).permute(1, 2, 0, 3), coef.to(dtype).permute(1, 2, 0, 3)
    dx, dy = p[..., 0:1] - kx, p[..., 1:2] - ky
    dx2, dy2 = dx * dx, dy * dy
    a, b, cc = c[..., 0:1], c[..., 1:2], c[..., 2:3]
    x = dx2 * (cc * dy2 + a) + b * dy2          # the kernels' association
    return dx, dy, dx2, dy2, a, b, cc, x


def dense_prior(point, coef, map_hw, inv_smooth, dtype=torch.float64):
    """G as the reference's dense tensor [Lq][Lk][B*H]"""
    x = prior_terms(point, coef, map_hw, dtype)[-1]
    B, H, Lq, Lk = x.shape
    return (-x.abs() * inv_smooth).permute(2, 3, 0, 1).reshape(Lq, Lk, B * H)


def core(ops, dtype=torch.float64, emulate=False):
    """ops: dict q, k, v, dout [L][B][E], mask bool [B][Lk] or None, point, coef, map_hw, inv_smooth, scale, H, and optionally keep
    [B][H][Lq][Lk] + drop_scale.  emulate: the kernels' bf16 rounding points (the weights before P V, the stored O beside its
    fp32 copy, P recomputed from lse in the backward, dS before its two products - NOT before the prior's sums -, the stored
    gradients).  Returns a dict: O, O32, lse, dq, dk, dv, dpoint, dcoef and P, dS, x (as [B][H][Lq][Lk])."""
    H, scale, inv_smooth = ops["H"], ops["scale"], ops["inv_smooth"]
    r = (lambda t: t.to(torch.bfloat16).to(dtype)) if emulate else (lambda t: t)
    Q, K, V, DO = (M.heads(ops[n].to(dtype), H) for n in ("q", "k", "v", "dout"))
    dx, dy, dx2, dy2, a, b, c, x = prior_terms(ops["point"], ops["coef"], ops["map_hw"], dtype)
    S = (Q @ K.transpose(-1, -2)) * scale - x.abs() * inv_smooth
    if ops.get("mask") is not None:
        S = S.masked_fill(ops["mask"].bool()[:, None, None, :], NEG)
    kd = 1.0 if ops.get("keep") is None else ops["keep"].to(dtype) * ops["drop_scale"]
    if emulate:
        oacc, l, mz = _forward_chunks(S, V, kd, ops.get("keep") is not None, r)
        live = l > 0
        e = None
    else:
        m = S.amax(-1, keepdim=True)
        live = m > NEG
        mz = torch.where(live, m, torch.zeros_like(m))
        e = torch.exp(S - mz) * live
        l = e.sum(-1, keepdim=True)
        oacc = (e * kd) @ V
    lz = torch.where(live, l, torch.ones_like(l))
    O32 = oacc / lz
    O = r(O32)
    lse = torch.where(live, mz + torch.log(lz), torch.full_like(mz, NEG))
    delta = (DO * O32).sum(-1, keepdim=True)
    if emulate:
        P = torch.exp(torch.where(live, S - torch.where(live, lse, torch.zeros_like(lse)), torch.full_like(S, NEG))) * live
    else:
        P = e / lz
    dP = DO @ V.transpose(-1, -2)
    dS = P * (dP * kd - delta)
    dSr, Pd = r(dS), r(P * kd)
    out = {"O": M.rows(O), "O32": M.rows(O32), "lse": lse.squeeze(-1), "P": P, "dS": dS, "x": x,
           "dq": M.rows(r((dSr @ K) * scale)), "dk": M.rows(r((dSr.transpose(-1, -2) @ Q) * scale)),
           "dv": M.rows(r(Pd.transpose(-1, -2) @ DO))}
    w = dS * torch.sign(x)
    dcoef = torch.stack([(w * dx2).sum(-1), (w * dy2).sum(-1), (w * dx2 * dy2).sum(-1)], -1) * -inv_smooth
    dpoint = torch.stack([(w * dx * (a + c * dy2)).sum(-1), (w * dy * (b + c * dx2)).sum(-1)], -1) * (-2 * inv_smooth)
    out["dcoef"], out["dpoint"] = dcoef.permute(2, 0, 1, 3).contiguous(), dpoint.permute(2, 0, 1, 3).contiguous()
    out["terms"] = {"a": w * dx2, "b": w * dy2, "c": w * dx2 * dy2}
    return out


def _forward_chunks(S, V, kd, drop, r):
    """the forward kernel's online softmax on logits S [B][H][Lq][Lk]: chunks of 128 keys and the LAZY reference maximum - it
    moves when some score of a 16-query wave exceeds it by more than 8 in the exp2 domain (8 ln 2 in logits), so the weights
    that are rounded to bf16 reach 2^8 and their mantissas are not those of exp(S - max).  Returns the unnormalised output, the
    normaliser (from the bf16 weights; with dropout from the fp32 weights before the drop) and the reference maximum (0 on a
    dead row), the last two as [B][H][Lq][1]"""
    B, H, Lq, Lk = S.shape
    G = (Lq + 15) // 16
    Lp = G * 16
    Sp = torch.full((B, H, Lp, Lk), NEG, dtype=S.dtype)
    Sp[:, :, :Lq] = S
    kdp = kd
    if torch.is_tensor(kd):
        kdp = torch.zeros(B, H, Lp, Lk, dtype=S.dtype)
        kdp[:, :, :Lq] = kd
    m_run = torch.full((B, H, Lp), NEG, dtype=S.dtype)
    oacc = torch.zeros(B, H, Lp, V.shape[-1], dtype=S.dtype)
    lacc = torch.zeros(B, H, Lp, dtype=S.dtype)
    zero, one = torch.zeros((), dtype=S.dtype), torch.ones((), dtype=S.dtype)
    for k0 in range(0, Lk, M.KC):
        s = Sp[..., k0:k0 + M.KC]
        mx = s.amax(-1)
        trig = (mx > m_run + 8.0 * 0.6931471805599453).view(B, H, G, 16).any(-1, keepdim=True).expand(B, H, G, 16).reshape(B, H, Lp)
        m_new = torch.where(trig, torch.maximum(m_run, mx), m_run)
        none = m_new == NEG
        mzn = torch.where(none, zero, m_new)
        alpha = torch.where(trig & ~none, torch.exp(torch.where(none, zero, m_run - mzn)), one)
        m_run = m_new
        pe = torch.exp(s - mzn[..., None]) * ~none[..., None]
        pf = r(pe * (kdp[..., k0:k0 + M.KC] if torch.is_tensor(kdp) else kdp))
        oacc = oacc * alpha[..., None] + pf @ V[:, :, k0:k0 + M.KC]
        lacc = lacc * alpha + (pe.sum(-1) if drop else pf.sum(-1))
    mz = torch.where(m_run == NEG, zero, m_run)
    return oacc[:, :, :Lq], lacc[:, :, :Lq, None], mz[:, :, :Lq, None]


def coef_of_type(kind, s, Lq, B, H, dtype=torch.float64):
    """the (a, b, c) of a dynamic_scale type from the raw scale head output s ([Lq, B, H * n] or None), squares taken here"""
    one, zero = torch.ones(Lq, B, H, 1, dtype=dtype), torch.zeros(Lq, B, H, 1, dtype=dtype)
    if kind == "type1":
        return torch.cat([one, one, zero], -1)
    s = (s * s).to(dtype)
    if kind == "type2":
        s = s.view(Lq, B, H, 1)
        return torch.cat([s, s, zero], -1)
    if kind == "type3":
        return torch.cat([s.view(Lq, B, H, 2), zero], -1)
    return s.view(Lq, B, H, 3)


# ------------------------------------------------------------------ the fixture's recipe
def recipe(name, shape, dtype=torch.float64):
    """bf16-representable values as a function of (name, flat index): k in [-16, 16] from an integer hash;
    matrices k / 256, LayerNorm weights 1 + k / 64, every other vector (biases) k / 128, inputs (name 'in/...') k / 16"""
    n = int(np.prod(shape))
    idx = np.arange(n, dtype=np.uint64)
    h = (idx * np.uint64(2654435761) + np.uint64(zlib.crc32(name.encode())) * np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    k = ((h >> np.uint64(9)) % np.uint64(33)).astype(np.float64) - 16.0
    if name.startswith("in/"):
        v = k / 16.0
    elif len(shape) >= 2:
        v = k / 256.0
    elif "norm" in name and name.endswith("weight"):
        v = 1.0 + k / 64.0
    else:
        v = k / 128.0
    return torch.from_numpy(v.reshape(shape)).to(dtype)


def fill(module):
    with torch.no_grad():
        for name, p in module.named_parameters():
            p.copy_(recipe(name, tuple(p.shape), p.dtype))
    return module


GOLD_CASE = dict(d_model=256, nhead=8, layers=2, dim_feedforward=32, B=2, Q=9, map_hw=(5, 7), smooth=8)


def gold_inputs(dtype=torch.float64):
    """src, mask, query_embed, pos_embed, h_w and the cotangent of hs for the fixture's case: image 1 with columns 5.. padded,
    h_w = (image width, image height), not square"""
    c = GOLD_CASE
    Hm, W = c["map_hw"]
    src = recipe("in/src", (c["B"], c["d_model"], Hm, W), dtype)
    pos = recipe("in/pos", (c["B"], c["d_model"], Hm, W), dtype)
    qe = recipe("in/query_embed", (c["Q"], c["d_model"]), dtype)
    dhs = recipe("in/dhs", (c["layers"], c["B"], c["Q"], c["d_model"]), dtype)
    mask = torch.zeros(c["B"], Hm, W, dtype=torch.bool)
    mask[1, :, 5:] = True
    h_w = torch.tensor([[[224.0, 160.0], [160.0, 144.0]]], dtype=dtype)
    return src, mask, qe, pos, h_w, dhs


PARAM_GRAD_TYPES = ("type3", "type4")     # the fixture holds parameter gradients for these (1 MiB does not hold all four)


def holds_param_grad(kind, name):
    """whether the fixture holds the gradient of parameter `name` for dynamic_scale `kind`: every parameter for
    PARAM_GRAD_TYPES; for the other types the point / scale heads point2 and point3, the parameters whose use differs by type"""
    return kind in PARAM_GRAD_TYPES or ".point2." in name or ".point3." in name


def reduce_grad(g):
    """what the fixture keeps of a gradient.  Vectors: whole up to 256 elements, beyond that as the [-1, 256] view below.
    Matrices: whole up to 512 elements, beyond that the row sums and the column sums.  [B, C, H, W] maps: the sums over
    (H, W) and the sums over C."""
    g = np.asarray(g, dtype=np.float64)
    if g.ndim == 4:
        return {"rows": g.sum((2, 3)), "cols": g.sum(1)}
    if g.ndim == 1 and g.size > 256:
        g = g.reshape(-1, 256)
    elif g.ndim < 2 or g.size <= 512:
        return {"full": g}
    return {"rows": g.sum(1), "cols": g.sum(0)}


# ------------------------------------------------------------------ operand recipes of the GPU tests
def _ints(g, shape, lo, hi, density=1.0):
    v = torch.randint(lo, hi + 1, shape, generator=g).double()
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density)
    return v


def live_runs(Lk, B, W):
    """per image a run of keys straddling a chunk boundary of 128 keys inside ONE row of the map (image 0: 8 keys; the others:
    4), the images starting their search at different boundaries"""
    bounds = list(range(128, Lk, 128))
    runs = []
    for i in range(B):
        n = 8 if i == 0 else 4
        order = bounds[i % len(bounds):] + bounds[:i % len(bounds)]
        bd = next(b for b in order if (b - n // 2) // W == (b + n // 2 - 1) // W)
        runs.append(list(range(bd - n // 2, bd + n // 2)))
    return runs


def run_mask(Lk, runs):
    mask = torch.ones(len(runs), Lk, dtype=torch.bool)
    for i, r in enumerate(runs):
        mask[i, r] = False
    return mask


def uniform_case(B, H, Lq, map_hw, coef_value, seed):
    """Q = 0; K, V, dO small integers (dO sparse: dS must fit bf16); dyadic points near each image's run of live keys; every
    coefficient = coef_value (0 or 2^-100)"""
    g = torch.Generator().manual_seed(seed)
    Hm, W = map_hw
    Lk, E = Hm * W, H * HD
    runs = live_runs(Lk, B, W)
    ops = dict(q=torch.zeros(Lq, B, E, dtype=torch.float64), k=_ints(g, (Lk, B, E), -2, 2), v=_ints(g, (Lk, B, E), -1, 1),
               dout=_ints(g, (Lq, B, E), -1, 1, 0.125), mask=run_mask(Lk, runs), map_hw=map_hw, inv_smooth=0.125, scale=0.25, H=H)
    point = torch.zeros(Lq, B, H, 2, dtype=torch.float64)
    for b in range(B):
        cx, cy = runs[b][len(runs[b]) // 2] % W, runs[b][len(runs[b]) // 2] // W
        for q in range(Lq):
            for h in range(H):
                point[q, b, h, 0] = cx + 0.5 * ((q + h) % 5) - 0.75
                point[q, b, h, 1] = cy + 0.5 * ((q + 2 * h + b) % 3) - 0.25
    ops["point"] = point
    ops["coef"] = torch.full((Lq, B, H, 3), float(coef_value), dtype=torch.float64)
    return ops


def assert_uniform_conditions(ops, ref):
    """what makes the uniform family exact (module docstring), checked on the float64 reference"""
    n = (~ops["mask"]).sum(1)
    for cnt in n.tolist():
        k = int(round(np.log2(cnt)))
        assert 2 ** k == cnt
        lse = np.float32(k) * np.float32(M.LN2_F)
        assert float(np.float32(lse) * np.float32(M.LOG2E_F)) == float(k), k      # the backward's exp2 argument is -k exactly
    P = ref["P"]
    live = (~ops["mask"])[:, None, None, :].expand_as(P)
    assert torch.equal(P[live], (1.0 / n.double())[:, None, None, None].expand_as(P)[live]) and float(P[~live].abs().max()) == 0
    # the prior is absent from the logits: |G| below half an ulp of 1 in the exp2 domain by a wide margin
    assert float((ref["x"].abs() * ops["inv_smooth"]).max()) < 2.0 ** -60
    for t in (ref["dS"], P):
        assert torch.equal(t.to(torch.bfloat16).double(), t)                       # the bf16 packs are exact
    for n_, t in ref["terms"].items():
        u = t * 65536.0
        assert torch.equal(u, u.round()), n_                                          # multiples of one unit (2^-16)
        assert float(u.abs().sum(-1).max()) < 2.0 ** 24, n_                         # any order of summation is exact
    for n_ in ("O", "dq", "dk", "dv"):
        u = ref[n_] * M.UNIT
        assert torch.equal(u, u.round()), n_


def gather_case(B, H, Lq, map_hw, seed):
    """Q = 0; image 1 with its last three columns padded; the point of (q, b, h) ON the live cell chosen[b][h][q], coefficients
    (1024, 2048, 512): the nearest other cell has G <= -1024 / 8 = -128, weight exp(-128) * ... = 0 after the fp32 exp2"""
    g = torch.Generator().manual_seed(seed)
    Hm, W = map_hw
    Lk, E = Hm * W, H * HD
    mask = torch.zeros(B, Hm, W, dtype=torch.bool)
    mask[1:, :, W - 3:] = True
    mask = mask.flatten(1)
    ops = dict(q=torch.zeros(Lq, B, E, dtype=torch.float64), k=_ints(g, (Lk, B, E), -2, 2), v=_ints(g, (Lk, B, E), -8, 8),
               dout=_ints(g, (Lq, B, E), -4, 4), mask=mask, map_hw=map_hw, inv_smooth=0.125, scale=0.25, H=H)
    chosen = torch.zeros(B, H, Lq, dtype=torch.long)
    point = torch.zeros(Lq, B, H, 2, dtype=torch.float64)
    for b in range(B):
        live = [i for i in range(Lk) if not bool(mask[b, i])]
        # every chunk boundary's two neighbours are among the choices
        pick = [i for i in live if i % 128 in (0, 127)] + live
        for h in range(H):
            for q in range(Lq):
                key = pick[(7 * q + 3 * b + 5 * h) % len(pick)]
                chosen[b, h, q] = key
                point[q, b, h, 0], point[q, b, h, 1] = key % W, key // W
    ops["point"] = point
    ops["coef"] = torch.tensor([1024.0, 2048.0, 512.0], dtype=torch.float64).expand(Lq, B, H, 3).contiguous()
    return ops, chosen


def gather_expected(ops, chosen):
    """O = V[chosen]; dv = the scatter of dO over the chosen keys"""
    H = ops["H"]
    V, DO = M.heads(ops["v"], H), M.heads(ops["dout"], H)
    idx = chosen[..., None].expand(-1, -1, -1, HD)
    O = torch.gather(V, 2, idx)
    dv = torch.zeros_like(V).scatter_add(2, idx, DO)
    return M.rows(O), M.rows(dv)


def assert_gather_conditions(ops, ref, chosen):
    P = ref["P"]
    onehot = torch.zeros_like(P).scatter(3, chosen[..., None], 1.0)
    # float64 leaves exp(-128) ~ 1e-56 where fp32 has 0: every other weight is below the smallest fp32 subnormal times 2^-20
    assert float((P - onehot).abs().max()) < 2.0 ** -170
    logit = -ref["x"].abs() * ops["inv_smooth"]
    other = logit.masked_fill(onehot.bool(), NEG).masked_fill(ops["mask"][:, None, None, :], NEG)
    assert float(other.max()) * 1.4426950408889634 < -170.0          # exp2 argument below fp32's range (2^-149)


def equidistant_case(B, H, Lq, map_hw, seed):
    """live keys: the 2 x 2 block with corner (cx, cy) per image; every point = the block's centre; a = b = 4, c = 0:
    G = -(4 * 1/4 + 4 * 1/4) / 8 = -1/4 on each of the four; Q = 0: P = 1/4"""
    g = torch.Generator().manual_seed(seed)
    Hm, W = map_hw
    Lk, E = Hm * W, H * HD
    mask = torch.ones(B, Hm, W, dtype=torch.bool)
    point = torch.zeros(Lq, B, H, 2, dtype=torch.float64)
    for b in range(B):
        # image 0: the block that straddles key 128 if the map has one (x = 127 % W, 128 % W in one row), else the middle
        cx, cy = (127 % W, 127 // W) if (Lk > 128 and 127 % W < W - 1) else (W // 2, Hm // 2)
        if b > 0:
            cx, cy = (cx + 2 * b) % (W - 1), (cy + b) % (Hm - 1)
        cy = min(cy, Hm - 2)
        mask[b, cy:cy + 2, cx:cx + 2] = False
        point[:, b, :, 0], point[:, b, :, 1] = cx + 0.5, cy + 0.5
    ops = dict(q=torch.zeros(Lq, B, E, dtype=torch.float64), k=_ints(g, (Lk, B, E), -2, 2), v=_ints(g, (Lk, B, E), -2, 2),
               dout=_ints(g, (Lq, B, E), -2, 2), mask=mask.flatten(1), map_hw=map_hw, inv_smooth=0.125, scale=0.25, H=H, point=point)
    ops["coef"] = torch.tensor([4.0, 4.0, 0.0], dtype=torch.float64).expand(Lq, B, H, 3).contiguous()
    return ops


def random_case(B, H, Lq, map_hw, kind, seed, negative=False):
    """random bf16 operands; points inside the map; coefficients of `kind` from random scales (negative: signs mixed, so that
    |.| and its sign work); image 1 with its last three columns padded"""
    g = torch.Generator().manual_seed(seed)
    Hm, W = map_hw
    Lk, E = Hm * W, H * HD
    bfr = lambda t: t.to(torch.bfloat16).double()
    mask = torch.zeros(B, Hm, W, dtype=torch.bool)
    mask[1:, :, W - 3:] = True
    ops = dict(q=bfr(torch.randn(Lq, B, E, generator=g)), k=bfr(torch.randn(Lk, B, E, generator=g)),
               v=bfr(torch.randn(Lk, B, E, generator=g)), dout=bfr(torch.randn(Lq, B, E, generator=g)), mask=mask.flatten(1),
               map_hw=map_hw, inv_smooth=0.125, scale=HD ** -0.5, H=H)
    pt = torch.rand(Lq, B, H, 2, generator=g) * torch.tensor([W - 1.0, Hm - 1.0])
    ops["point"] = pt.float().double()
    n = {"type1": 0, "type2": 1, "type3": 2, "type4": 3}[kind]
    s = None if n == 0 else (0.3 + 0.7 * torch.rand(Lq, B, H * n, generator=g)).double()
    coef = coef_of_type(kind, s, Lq, B, H)
    if kind == "type4":
        coef[..., 2] = coef[..., 2] * 0.05          # (dx^2 dy^2 reaches 10^5 on these maps)
    if negative:
        coef = coef * torch.where(torch.rand(Lq, B, H, 3, generator=g) < 0.5, -1.0, 1.0)
    ops["coef"] = coef.float().double()
    return ops
