"""Restatement of row-column decoupled attention (csrc/rcda.hip, modeling/rcda.py), written from its definition:

    Qr = lin0(query_row)  Qc = lin1(query_col)  Kr = lin2(mean over H of key_row)  Kc = lin3(mean over W of key_col)  V = lin4(value)
    A_row[b,n,q,:] = softmax over w of scale Qr[b,q,n,:] . Kr[b,w,n,:]   (-inf where mask[b, 0, w])
    A_col[b,n,q,:] = softmax over h of scale Qc[b,q,n,:] . Kc[b,h,n,:]   (-inf where mask[b, h, 0])
    O[b,q,n,:]     = sum over h, w of A_col[b,n,q,h] A_row[b,n,q,w] V[b,h,w,n,:]          out = out_proj(O) as (L, B, E)

`core` / `module` are differentiable torch code in whatever dtype the operands have (float64: the reference).  With
emulate=True they are the fp32 restatement of the kernels' arithmetic: the same graph with a bf16 rounding wherever the kernels
store or feed the matrix cores in bf16 - in the forward pass (the weight A_col A_row, the output, every projected tensor, the
key means), in the backward pass (the two softmax gradients, every gradient tensor) or both.  Its error against float64 on the
same operands is the floor the device tests derive their bounds from.  A query whose row or column keys are all padded gives
O = 0 and no gradient in both (the reference gives NaN: the one deliberate difference).

The exact families (uniform, gather) and their exactness conditions are at the end.
"""

import numpy as np
import torch

HD = 32
LOG2E = 1.4426950408889634


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


class _Round(torch.autograd.Function):
    """bf16 rounding in the forward pass (fwd), of the gradient in the backward pass (bwd), or both"""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return bf16_round(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (bf16_round(g) if ctx.bwd else g), None, None


def _r(x, on, fwd=True, bwd=True):
    return _Round.apply(x, fwd, bwd) if on else x


def _softmax(z, mask):
    """softmax over the last axis of z [B, n, L, K] with mask [B, K] (True = padded); all padded: zeros, no NaN anywhere"""
    if mask is not None:
        z = z.masked_fill(mask[:, None, None, :].bool(), float("-inf"))
    m = z.max(-1, keepdim=True).values
    dead = torch.isinf(m)
    p = torch.exp(z - torch.where(dead, torch.zeros_like(m), m))     # (exp, not exp2: its gradient is p itself, exact for dyadic p)
    l = p.sum(-1, keepdim=True)
    return p / torch.where(dead, torch.ones_like(l), l), dead[..., 0]


def core(q_row, q_col, k_row, k_col, v, mask_row, mask_col, heads, emulate=False, scale=None):
    """q_row, q_col [B, L, E]; k_row [B, W, E]; k_col [B, H, E]; v [B, H, W, E]; masks [B, W] / [B, H] or None -> O [B, L, E].
    emulate: operands are taken as the bf16 tensors the kernels read (their gradients are rounded to bf16)"""
    B, Lq, E = q_row.shape
    hd = E // heads
    scale = hd ** -0.5 if scale is None else scale
    sp = lambda x: _r(x, emulate, fwd=True, bwd=True).reshape(*x.shape[:-1], heads, hd)
    qr, qc, kr, kc, vv = sp(q_row), sp(q_col), sp(k_row), sp(k_col), sp(v)
    zr = _r(torch.einsum("blnd,bwnd->bnlw", qr, kr) * scale, emulate, fwd=False, bwd=True)
    zc = _r(torch.einsum("blnd,bhnd->bnlh", qc, kc) * scale, emulate, fwd=False, bwd=True)
    ar, dead_r = _softmax(zr, mask_row)
    ac, dead_c = _softmax(zc, mask_col)
    live = (~(dead_r | dead_c))[..., None].to(ar.dtype)
    ar, ac = ar * live, ac * live
    p = _r(ac[..., :, None] * ar[..., None, :], emulate, fwd=True, bwd=False)           # [B, n, L, H, W]
    o = torch.einsum("bnlhw,bhwnd->blnd", p, vv).reshape(B, Lq, E)
    return _r(o, emulate, fwd=True, bwd=True)


def module(params, query_row, query_col, key_row, key_col, value, mask, heads, emulate=False, mean_first=True):
    """MultiheadRCDA.forward -> out (L, B, E).  params: dict with in_proj_weight [5E, E], in_proj_bias [5E], out_proj.weight,
    out_proj.bias.  mean_first=False: project the key maps, then average (the reference's order)"""
    E = query_row.shape[-1]
    w, b = params["in_proj_weight"], params["in_proj_bias"]

    def lin(x, i):
        x = _r(x, emulate)
        return _r(x @ _r(w[i * E:(i + 1) * E], emulate, bwd=False).t() + b[i * E:(i + 1) * E], emulate)

    if mean_first:
        kr, kc = lin(_r(_r(key_row, emulate).mean(1), emulate), 2), lin(_r(_r(key_col, emulate).mean(2), emulate), 3)
    else:
        kr, kc = lin(key_row, 2).mean(1), lin(key_col, 3).mean(2)
    mr = mc = None
    if mask is not None:
        mr, mc = mask[:, 0, :], mask[:, :, 0]
    o = core(lin(query_row, 0), lin(query_col, 1), kr, kc, lin(value, 4), mr, mc, heads, emulate)
    out = _r(o @ _r(params["out_proj.weight"], emulate, bwd=False).t() + params["out_proj.bias"], emulate)
    return out.transpose(0, 1)


# ------------------------------------------------------------------ errors
def rel_l2(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def rel_max(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------ random operands
CORE_NAMES = ("q_row", "q_col", "k_row", "k_col", "v")


def fixture_mask(B, H, W):
    """image 1 (when there is one) with columns 5.. and rows 4.. padded, scaled to the map: W * 5 // 7, H * 4 // 5"""
    m = torch.zeros(B, H, W, dtype=torch.bool)
    if B > 1:
        m[1, :, max(1, W * 5 // 7):] = True
        m[1, max(1, H * 4 // 5):, :] = True
    return m


def random_core_case(B, heads, Lq, H, W, seed):
    """bf16-representable float64 operands of `core`, the cotangent and the masks (image 1 partly padded)"""
    g = torch.Generator().manual_seed(seed)
    E = heads * HD
    rnd = lambda *s: bf16_round(torch.randn(*s, generator=g, dtype=torch.float64))
    ops = dict(q_row=rnd(B, Lq, E) * 2, q_col=rnd(B, Lq, E) * 2, k_row=rnd(B, W, E), k_col=rnd(B, H, E), v=rnd(B, H, W, E))
    m = fixture_mask(B, H, W)
    return ops, rnd(B, Lq, E), m[:, 0, :].clone(), m[:, :, 0].clone()


def core_with_grads(ops, dout, mask_row, mask_col, heads, dtype, emulate, scale=None):
    xs = [ops[n].to(dtype).clone().requires_grad_(True) for n in CORE_NAMES]
    o = core(*xs, mask_row, mask_col, heads, emulate=emulate, scale=scale)
    o.backward(dout.to(dtype))
    return o.detach(), {n: x.grad for n, x in zip(CORE_NAMES, xs)}


# ------------------------------------------------------------------ exact families
# A softmax is exact where its weights are dyadic.
#   uniform: k_row = k_col = 0: every score is 0, A_col A_row = 1 / (nW nH) with nW, nH the live counts, powers of two (where
#     W or H is not one, the mask leaves a power of two live - in EVERY image: 1 / 35 is not dyadic).  V[h, w, d] =
#     c[d] (a[w] + b[h] + 3) with small integers, sum of a over the live columns = sum of b over the live rows = 0, and the
#     cotangent has one entry +-1 or +-2 per (query, head): then T = dO . V = s (a[w] + b[h] + 3), delta = 3 s, and the softmax gradients are
#     dS_row = s a[w] / nW, dS_col = s b[h] / nH: a few bits each, so that the bf16 operands of every matrix product are the
#     exact values, every fp32 sum is exact, and each stored bf16 is the float64 reference rounded once.
#   gather: the rows of k_row and of k_col are distinct +-1 codes (pairwise Hamming distance >= 4) and query q carries G times
#     the codes of one live (h*, w*): its score leads every other by >= 8 G scale, and with G = 512 every other weight
#     underflows to exactly 0 in fp32.  O = V[h*, w*]; dS = 0 exactly, dV[h, w] = the sum of the integer cotangents that chose it.
GATHER_GAIN = 512.0
UNIFORM_OFFSET = 3.0     # O = c[d] * UNIFORM_OFFSET: not zero


def _live_counts(n):
    """(live count of image 0, of image 1): powers of two, different, <= n"""
    p = 1 << (n.bit_length() - 1)
    return p, max(1, p // 2)


def uniform_case(B, heads, Lq, H, W, seed):
    rs = np.random.RandomState(seed)
    E = heads * HD
    nW, nH = [_live_counts(W)[min(b, 1)] for b in range(B)], [_live_counts(H)[min(b, 1)] for b in range(B)]
    mask_row, mask_col = torch.zeros(B, W, dtype=torch.bool), torch.zeros(B, H, dtype=torch.bool)
    v = torch.zeros(B, H, W, E, dtype=torch.float64)
    c = torch.from_numpy(rs.choice([-1.0, 1.0], size=E))

    def zero_sum(n_live, n):
        x = rs.randint(-2, 3, size=n).astype(np.float64)
        x[n_live - 1] -= x[:n_live].sum()          # (n_live = 1: the one live entry is 0)
        if abs(x[n_live - 1]) > 16:
            x[:n_live] = 0
        return torch.from_numpy(x)

    for b in range(B):
        mask_row[b, nW[b]:] = True
        mask_col[b, nH[b]:] = True
        a, bb = zero_sum(nW[b], W), zero_sum(nH[b], H)
        v[b] = (a[None, :, None] + bb[:, None, None] + UNIFORM_OFFSET) * c[None, None, :]
    q = lambda: torch.from_numpy(rs.randint(-3, 4, size=(B, Lq, E)).astype(np.float64))
    ops = dict(q_row=q(), q_col=q(), k_row=torch.zeros(B, W, E, dtype=torch.float64), k_col=torch.zeros(B, H, E, dtype=torch.float64), v=v)
    dout = torch.zeros(B, Lq, heads, HD, dtype=torch.float64)
    pos = torch.from_numpy(rs.randint(0, HD, size=(B, Lq, heads, 1)))
    dout.scatter_(3, pos, torch.from_numpy(rs.choice([-2.0, -1.0, 1.0, 2.0], size=(B, Lq, heads, 1))))
    return ops, dout.reshape(B, Lq, E), mask_row, mask_col


def _codes(n):
    """n <= 256 distinct +-1 rows of 32: the 8 bits of the index, four times over (pairwise Hamming distance >= 4)"""
    idx = np.arange(n)
    bits = ((idx[:, None] >> np.arange(8)[None, :]) & 1).astype(np.float64) * 2 - 1
    return np.tile(bits, (1, 4))


def gather_case(B, heads, Lq, H, W, seed):
    rs = np.random.RandomState(seed)
    E = heads * HD
    m = fixture_mask(B, H, W)
    mask_row, mask_col = m[:, 0, :].clone(), m[:, :, 0].clone()
    kr = np.tile(_codes(W)[None, :, None, :], (B, 1, heads, 1)) * rs.choice([-1.0, 1.0], size=(1, 1, heads, HD))
    kc = np.tile(_codes(H)[None, :, None, :], (B, 1, heads, 1)) * rs.choice([-1.0, 1.0], size=(1, 1, heads, HD))
    hs, ws = np.zeros((B, Lq, heads), dtype=np.int64), np.zeros((B, Lq, heads), dtype=np.int64)
    for b in range(B):
        live_w, live_h = np.nonzero(~mask_row[b].numpy())[0], np.nonzero(~mask_col[b].numpy())[0]
        ws[b], hs[b] = rs.choice(live_w, size=(Lq, heads)), rs.choice(live_h, size=(Lq, heads))
    bi, ni = np.arange(B)[:, None, None], np.arange(heads)[None, None, :]
    ops = dict(q_row=torch.from_numpy(kr[bi, ws, ni] * GATHER_GAIN).reshape(B, Lq, E),
               q_col=torch.from_numpy(kc[bi, hs, ni] * GATHER_GAIN).reshape(B, Lq, E),
               k_row=torch.from_numpy(kr).reshape(B, W, E), k_col=torch.from_numpy(kc).reshape(B, H, E),
               v=bf16_round(torch.from_numpy(rs.standard_normal((B, H, W, E)))))
    dout = torch.from_numpy(rs.randint(-4, 5, size=(B, Lq, E)).astype(np.float64))
    return ops, dout, mask_row, mask_col, torch.from_numpy(hs), torch.from_numpy(ws)


def gather_expected(ops, dout, hs, ws, heads):
    """(O, dV) of a gather case from its choices alone: O[b, q, n] = V[b, h*, w*, n], dV = the scatter of dout"""
    v = ops["v"]
    B, H, W, E = v.shape
    Lq = dout.shape[1]
    vv, dd = v.reshape(B, H, W, heads, HD), dout.reshape(B, Lq, heads, HD)
    bi, ni = torch.arange(B)[:, None, None], torch.arange(heads)[None, None, :]
    o = vv[bi, hs, ws, ni].reshape(B, Lq, E)
    dv = torch.zeros_like(vv)
    dv.index_put_((bi.expand_as(hs), hs, ws, ni.expand_as(hs)), dd, accumulate=True)
    return o, dv.reshape(B, H, W, E)


def is_bf16(x):
    return bool((bf16_round(x) == x).all())


def check_uniform_conditions(ops, dout, mask_row, mask_col, heads):
    """the exactness conditions of a uniform case, from float64 intermediates"""
    B, Lq, E = dout.shape
    nW, nH = (~mask_row).sum(1), (~mask_col).sum(1)
    for n in list(nW) + list(nH):
        assert int(n) >= 1 and int(n) & (int(n) - 1) == 0, "live counts must be powers of two"
    assert float(ops["k_row"].abs().max()) == 0 and float(ops["k_col"].abs().max()) == 0
    for x in list(ops.values()) + [dout]:
        assert is_bf16(x) and bool((x == x.round()).all()) and float(x.abs().max()) <= 64
    v = ops["v"].reshape(B, *ops["v"].shape[1:3], heads, HD)
    d = dout.reshape(B, Lq, heads, HD)
    T = torch.einsum("blnd,bhwnd->bnlhw", d, v)
    lw, lh = (~mask_row).double()[:, None, None, None, :], (~mask_col).double()[:, None, None, :, None]
    ar, ac = lw / nW.double()[:, None, None, None, None], lh / nH.double()[:, None, None, None, None]
    da_r, da_c = (ac * T).sum(3, keepdim=True), (ar * T).sum(4, keepdim=True)
    delta = (ar * da_r).sum(4, keepdim=True)
    ds_r, ds_c = ar * (da_r - delta), ac * (da_c - delta)
    assert is_bf16(ds_r) and is_bf16(ds_c) and is_bf16(ac * ar), "softmax gradients / weights must be bf16 numbers"
    for x in (T, da_r, da_c, delta):     # fp32 holds every partial sum exactly: dyadic with a small numerator
        assert bool((x * 4096 == (x * 4096).round()).all()) and float(x.abs().max()) < 4096


def check_gather_conditions(ops, mask_row, mask_col, hs, ws, heads):
    """every chosen key is live, its score leads all others by enough that exp2 underflows to 0 in fp32"""
    B, Lq, E = ops["q_row"].shape
    scale = HD ** -0.5
    for q, k, mask, ch in ((ops["q_row"], ops["k_row"], mask_row, ws), (ops["q_col"], ops["k_col"], mask_col, hs)):
        z = torch.einsum("blnd,bknd->bnlk", q.reshape(B, Lq, heads, HD), k.reshape(B, -1, heads, HD)) * scale * LOG2E
        top = z.gather(3, ch.permute(0, 2, 1)[..., None])
        assert not bool(mask.gather(1, ch.reshape(B, -1)).any())
        other = z.masked_fill(torch.zeros_like(z, dtype=torch.bool).scatter_(3, ch.permute(0, 2, 1)[..., None], True), float("-inf"))
        assert float((top - other.max(-1, keepdim=True).values).min()) > 160, "the runner-up must underflow (2^-149 is the least fp32)"
        assert is_bf16(q) and is_bf16(k)


# shapes (B, heads, L, H, W) of the exact families
EXACT_SHAPES = [(2, 2, 70, 5, 7), (1, 8, 130, 16, 32), (2, 1, 64, 25, 42), (1, 2, 3, 1, 1), (1, 2, 1, 1, 1), (1, 1, 16, 4, 8)]
