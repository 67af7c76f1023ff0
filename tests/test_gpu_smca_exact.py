"""GPU (-m gpu): attention with SMCA's Gaussian prior (csrc/mha.hip PRIOR instantiations, modeling/smca.py) against
tests/smca_ref.py, through the C entries mi_smca_fwd / mi_smca_bwd on guarded buffers: every operand sits between NaN guards,
every output view is pre-filled with NaN between sentinel guards; every element must have been written and every guard must
come back untouched.

Shapes: B 2, H 2 (one case H 8); Lq 21 (a ragged 16-row group) and 130 (two chunks of queries for the dK / dV kernel); maps
5 x 27 (Lk 135: one chunk boundary, ragged tail, W no power of two, Hm != W) and 13 x 21 (273: three chunks, both LDS buffers
reused); image 1 padded.  At these sizes mha2_waves gives every kernel 4 waves per block (mirrored and asserted below): one
block shape is reachable, so there is nothing to count.

  1  zero coefficients: bit for bit what mi_mha_*_dropout_ld gives on the same buffers, with and without dropout; dpoint = 0;
  2  uniform family: everything exact; dcoef = 0 exactly for coefficients 0 (sign(0) = 0, as torch) and, for coefficients
     2^-100 (numerically absent from the logits, sign +1), dcoef = -inv_smooth sum dS {dx^2, dy^2, dx^2 dy^2} = the float64
     value rounded once;
  3  gather by the prior: O = V[chosen], dv = the scatter of dO, dq = dk = dpoint = dcoef = 0;
  4  equidistant family: P = 1/4 over a nonzero maximum, dpoint != 0; the forward is exact, the backward within EPS (below);
  5  random operands, four types, dropout 0 and 0.5: within twice the error of the fp32 / bf16 restatement against float64;
  6  SMCATransformer against the fixture tests/golden/smca.npz;
  7  smca_core forward + backward captured in a graph: two replays equal the eager result bit for bit.

EPS of 4.  The backward recomputes P = exp2(e2), e2 = fl(s sc2 + neg_l), neg_l = fl(-lse log2e_f); the true exponent is -2.
Errors of e2 in units of 2^-23 (one fp32 ulp at [1, 2)): the stored lse, LSE_ULPS = 2 ulps at lse = 1.14, times log2 e: 2.9;
the constant log2e_f in neg_l (|neg_l| = 1.64): 1; the rounding of neg_l: 0.5; the constant inside sc2 (|s sc2| = 1.44): 1; the
fma's rounding at 2: 1 - together 6.4, times ln 2 = 4.5 relative units in P; the device exp2: 1; the product P (dP - delta):
0.5; four-term sums in fp32: 2.  8 units = 2^-20 = EPS, applied to the sum of the magnitudes of each output's terms; a bf16
output may in addition sit on the other side of a rounding boundary: one bf16 ulp of the reference."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mha_ref as M
import smca_ref as R
from yolov7_d2_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENT = -1536.0      # exact in bf16 and fp32
NAN = float("nan")
EPS = 2.0 ** -20
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smca.npz")
SHAPES = [(2, 2, 21, (5, 27)), (2, 2, 130, (13, 21)), (2, 8, 21, (5, 27))]        # B, H, Lq, map
BF, F32 = torch.bfloat16, torch.float32


class Buf:
    """a contiguous tensor between two guards: NaN around an operand; around an output the sentinel, NaN inside"""

    def __init__(self, shape, dtype, src=None):
        n = int(np.prod(shape))
        self.is_out = src is None
        fill = SENT if self.is_out else (1 if dtype == torch.uint8 else NAN)     # (uint8 has no NaN: padded flags)
        self.flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.flat[GUARD:GUARD + n].view(*shape)
        if src is None:
            self.t.fill_(NAN)
        else:
            self.t.copy_(src.to(dtype))

    def guards_ok(self):
        g = torch.cat([self.flat[:GUARD], self.flat[-GUARD:]])
        if self.is_out:
            return bool((g == SENT).all())
        return bool((g == 1).all()) if g.dtype == torch.uint8 else bool(torch.isnan(g).all())

    def written(self):
        return not bool(torch.isnan(self.t).any())


def mirror_check(B, H, Lq, Lk):
    n = torch.cuda.get_device_properties(0).multi_processor_count
    assert M.mirror_waves(Lq, B * H, n) == 4 and M.mirror_waves(Lk, B * H, n) == 4


class Job:
    def __init__(self, ops, drop_p=0.0, seed=0):
        Lq, B, E = ops["q"].shape
        Lk, H = ops["k"].shape[0], ops["H"]
        self.dims = (B, H, Lq, Lk, E)
        mirror_check(B, H, Lq, Lk)
        self.ops, self.p, self.seed = ops, drop_p, seed
        self.inp = {n: Buf(ops[n].shape, BF, ops[n]) for n in ("q", "k", "v", "dout")}
        self.inp.update({n: Buf(ops[n].shape, F32, ops[n]) for n in ("point", "coef")})
        if ops.get("mask") is not None:
            self.inp["mask"] = Buf(ops["mask"].shape, torch.uint8, ops["mask"])

    def outputs(self, smca):
        B, H, Lq, Lk, E = self.dims
        out = {"O": Buf((Lq, B, E), BF), "O32": Buf((Lq, B, E), F32), "lse": Buf((B, H, Lq), F32), "delta": Buf((B, H, Lq), F32),
               "dq": Buf((Lq, B, E), BF), "dk": Buf((Lk, B, E), BF), "dv": Buf((Lk, B, E), BF)}
        if smca:
            out.update({"dpoint": Buf((Lq, B, H, 2), F32), "dcoef": Buf((Lq, B, H, 3), F32)})
        return out

    def desc(self, out):
        B, H, Lq, Lk, E = self.dims
        d = L.mi_smca_desc()
        for n in ("q", "k", "v", "dout", "point", "coef"):
            setattr(d, n, self.inp[n].t.data_ptr())
        d.mask = self.inp["mask"].t.data_ptr() if "mask" in self.inp else None
        for n, f in (("O", "o"), ("O32", "o_f32"), ("lse", "lse"), ("delta", "delta"), ("dq", "dq"), ("dk", "dk"), ("dv", "dv"),
                     ("dpoint", "dpoint"), ("dcoef", "dcoef")):
            setattr(d, f, out[n].t.data_ptr())
        d.B, d.H, d.Lq, d.Lk, d.E, d.ldq, d.ldk = B, H, Lq, Lk, E, E, E
        d.map_h, d.map_w = self.ops["map_hw"]
        d.scale, d.inv_smooth, d.drop_p, d.seed = self.ops["scale"], self.ops["inv_smooth"], self.p, self.seed
        return d

    def finish(self, out):
        torch.cuda.synchronize()
        for n, b in list(self.inp.items()) + list(out.items()):
            assert b.guards_ok(), n
        for n, b in out.items():
            assert b.written(), n
        return out

    def run_smca(self):
        out = self.outputs(True)
        d = self.desc(out)
        L.check(L.lib().mi_smca_fwd(C.byref(d), L.stream_ptr()), "mi_smca_fwd")
        L.check(L.lib().mi_smca_bwd(C.byref(d), L.stream_ptr()), "mi_smca_bwd")
        return self.finish(out)

    def run_mha(self):
        B, H, Lq, Lk, E = self.dims
        out = self.outputs(False)
        i, o = self.inp, out
        mk = i["mask"].t.data_ptr() if "mask" in i else None
        lib, sc = L.lib(), self.ops["scale"]
        L.check(lib.mi_mha_fwd_dropout_ld(i["q"].t.data_ptr(), E, i["k"].t.data_ptr(), E, i["v"].t.data_ptr(), mk, o["O"].t.data_ptr(),
                                          o["O32"].t.data_ptr(), o["lse"].t.data_ptr(), B, H, Lq, Lk, E, sc, self.p, self.seed,
                                          L.stream_ptr()), "mi_mha_fwd_dropout_ld")
        L.check(lib.mi_mha_bwd_dropout_ld(i["q"].t.data_ptr(), E, i["k"].t.data_ptr(), E, i["v"].t.data_ptr(), mk, o["O"].t.data_ptr(),
                                          o["O32"].t.data_ptr(), o["lse"].t.data_ptr(), i["dout"].t.data_ptr(), o["delta"].t.data_ptr(),
                                          o["dq"].t.data_ptr(), o["dk"].t.data_ptr(), o["dv"].t.data_ptr(), B, H, Lq, Lk, E, sc, self.p,
                                          self.seed, L.stream_ptr()), "mi_mha_bwd_dropout_ld")
        return self.finish(out)

    def keep(self):
        B, H, Lq, Lk, _ = self.dims
        k = torch.empty(B, H, Lq, Lk, dtype=torch.uint8, device=DEV)
        L.check(L.lib().mi_mha_dropout_mask(k.data_ptr(), B, H, Lq, Lk, self.p, self.seed, L.stream_ptr()), "mi_mha_dropout_mask")
        torch.cuda.synchronize()
        return k.cpu()


def host(out):
    return {n: b.t.double().cpu() for n, b in out.items()}


def stored(x):
    return x.float().to(BF).double()


def f32(x):
    return x.float().double()


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", SHAPES)
def test_zero_coefficients_are_plain_attention_bit_for_bit(shape, p):
    B, H, Lq, mp = shape
    ops = R.random_case(B, H, Lq, mp, "type1", seed=11)
    ops["coef"] = torch.zeros_like(ops["coef"])
    job = Job(ops, p, 0x5DEECE66D if p else 0)
    a, b = job.run_smca(), job.run_mha()
    for n in ("O", "O32", "lse", "delta", "dq", "dk", "dv"):
        x, y = a[n].t, b[n].t
        bits = torch.int16 if x.dtype == BF else torch.int32
        assert torch.equal(x.view(bits), y.view(bits)), (n, float((x.double() - y.double()).abs().max()))
    assert float(a["dpoint"].t.abs().max()) == 0 and float(a["dcoef"].t.abs().max()) == 0
    assert float(a["dq"].t.float().abs().max()) > 0 and float(a["O"].t.float()[:, 1].abs().max()) > 0


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("cv", [0.0, 2.0 ** -100])
@pytest.mark.parametrize("shape", SHAPES)
def test_uniform_family_bit_exact(shape, cv):
    B, H, Lq, mp = shape
    ops = R.uniform_case(B, H, Lq, mp, cv, seed=1)
    ref = R.core(ops)
    R.assert_uniform_conditions(ops, ref)
    got = host(Job(ops).run_smca())
    for n in ("O", "dq", "dk", "dv"):
        assert torch.equal(got[n], stored(ref[n])), (n, float((got[n] - ref[n]).abs().max()))
    assert torch.equal(got["O32"], f32(ref["O32"]))
    assert M.lse_mismatch(got["lse"], ref["lse"]) == 0
    want = f32(ref["dcoef"])
    assert torch.equal(got["dcoef"], want), float((got["dcoef"] - want).abs().max())
    assert (float(want.abs().max()) > 0) == (cv > 0)
    if cv == 0:
        assert float(got["dpoint"].abs().max()) == 0
    else:   # (2^-100 times a few cells: far below anything, and not part of the exact claim)
        assert float(got["dpoint"].abs().max()) < 1e-25


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("shape", SHAPES)
def test_gather_by_the_prior(shape):
    B, H, Lq, mp = shape
    ops, chosen = R.gather_case(B, H, Lq, mp, seed=2)
    R.assert_gather_conditions(ops, R.core(ops), chosen)
    eo, edv = R.gather_expected(ops, chosen)
    got = host(Job(ops).run_smca())
    assert torch.equal(got["O"], stored(eo)) and torch.equal(got["O32"], eo)
    assert torch.equal(got["dv"], stored(edv)), float((got["dv"] - edv).abs().max())
    for n in ("dq", "dk", "dpoint", "dcoef"):
        assert float(got[n].abs().max()) == 0, n
    assert float(got["lse"].abs().max()) == 0


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("shape", SHAPES)
def test_equidistant_family(shape):
    B, H, Lq, mp = shape
    ops = R.equidistant_case(B, H, Lq, mp, seed=3)
    ref = R.core(ops)
    P = ref["P"]
    assert torch.equal(P[P > 0], torch.full_like(P[P > 0], 0.25)) and float(ref["dpoint"].abs().max()) > 0
    got = host(Job(ops).run_smca())
    assert torch.equal(got["O"], stored(ref["O"])) and torch.equal(got["O32"], f32(ref["O32"]))
    assert M.lse_mismatch(got["lse"], ref["lse"]) == 0
    assert float(got["dk"].abs().max()) == 0                          # Q = 0
    # sums of the magnitudes of each output's terms
    Hh = ops["H"]
    K, DO = M.heads(ops["k"], Hh), M.heads(ops["dout"], Hh)
    dx, dy, dx2, dy2, a, b, c, x = R.prior_terms(ops["point"], ops["coef"], ops["map_hw"], torch.float64)
    aS = ref["dS"].abs()
    mags = {"dq": M.rows(aS @ K.abs()) * ops["scale"], "dv": M.rows(P.transpose(-1, -2) @ DO.abs()),
            "dcoef": (torch.stack([(aS * dx2).sum(-1), (aS * dy2).sum(-1), (aS * dx2 * dy2).sum(-1)], -1) * ops["inv_smooth"]).permute(2, 0, 1, 3),
            "dpoint": (torch.stack([(aS * (dx * (a + c * dy2)).abs()).sum(-1), (aS * (dy * (b + c * dx2)).abs()).sum(-1)], -1)
                       * 2 * ops["inv_smooth"]).permute(2, 0, 1, 3)}
    for n in ("dq", "dv", "dpoint", "dcoef"):
        tol = EPS * mags[n] + (2.0 ** -8 * ref[n].abs() if n in ("dq", "dv") else 0.0)
        err = (got[n] - ref[n]).abs()
        print(f"smca equidistant {shape} {n:7s} max err {float(err.max()):.3e}  max allowed {float(tol.max()):.3e}  max |ref| {float(ref[n].abs().max()):.3e}")
        assert bool((err <= tol).all()), (n, float((err - tol).max()))


# ------------------------------------------------------------------ 5
RANDOM = [((2, 2, 21, (5, 27)), "type1", False), ((2, 2, 130, (13, 21)), "type2", False), ((2, 8, 21, (5, 27)), "type3", False),
          ((2, 2, 130, (5, 27)), "type4", False), ((2, 2, 21, (13, 21)), "type4", True)]


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape,kind,negative", RANDOM)
def test_random_operands_within_twice_the_emulation_floor(shape, kind, negative, p):
    B, H, Lq, mp = shape
    ops = R.random_case(B, H, Lq, mp, kind, seed=7, negative=negative)
    job = Job(ops, p, 0x2545F4914F6CDD1D if p else 0)
    if p:
        ops["keep"], ops["drop_scale"] = job.keep(), 1.0 / (1.0 - p)
        assert 0.4 < float(ops["keep"].double().mean()) < 0.6
    r64, r32 = R.core(ops), R.core(ops, torch.float32, True)
    if negative:
        assert float(r64["x"].min()) < 0 < float(r64["x"].max())
    got = host(job.run_smca())
    fails = []
    for n in R.CORE_OUT:
        for metric in (R.rel_l2, R.rel_max):
            floor, err = metric(r32[n], r64[n]), metric(got[n], r64[n])
            print(f"smca random {shape} {kind} p {p} {n:7s} {metric.__name__}: floor {floor:.3e}  device {err:.3e}")
            assert floor > 0
            if not err <= 2 * floor:
                fails.append((n, metric.__name__, floor, err))
    assert not fails, fails


def test_fully_padded_rows_and_reproducibility():
    ops = R.random_case(2, 2, 21, (5, 27), "type3", seed=9)
    ops["mask"][1, :] = True                    # image 1: every key padded
    job = Job(ops)
    a, b = host(job.run_smca()), host(job.run_smca())
    for n in a:
        assert torch.equal(a[n], b[n]), n
    assert bool((a["lse"][1] == float("-inf")).all()) and bool(torch.isfinite(a["lse"][0]).all())
    for n in ("O", "dq", "dk", "dv", "dpoint", "dcoef"):
        assert float(a[n][:, 1].abs().max()) == 0 and float(a[n][:, 0].abs().max()) > 0, n


def test_core_refuses_wrong_shapes_by_name():
    from yolov7_d2_amd.modeling import smca_core
    q, k = torch.zeros(3, 1, 64, device=DEV, dtype=BF), torch.zeros(6, 1, 64, device=DEV, dtype=BF)
    pt, cf = torch.zeros(3, 1, 2, 2, device=DEV), torch.zeros(3, 1, 2, 3, device=DEV)
    for bad_pt, bad_cf in ((pt[:2], cf), (pt, cf[..., :2]), (pt.view(3, 2, 1, 2), cf), (cf, pt)):
        with pytest.raises(ValueError, match="point .* coef"):
            smca_core(q, k, k, bad_pt, bad_cf, (2, 3), 8.0, None, 2)
    with pytest.raises(ValueError, match="6 keys are not a 2 x 4 map"):
        smca_core(q, k, k, pt, cf, (2, 4), 8.0, None, 2)
    assert smca_core(q, k, k, pt, cf, (2, 3), 8.0, None, 2).shape == (3, 1, 64)


# ------------------------------------------------------------------ 6
def _module_run(kind):
    from yolov7_d2_amd.modeling import SMCATransformer
    c = R.GOLD_CASE
    net = SMCATransformer(d_model=c["d_model"], nhead=c["nhead"], num_encoder_layers=0, num_decoder_layers=c["layers"],
                          dim_feedforward=c["dim_feedforward"], dropout=0.0, return_intermediate_dec=True, smooth=c["smooth"],
                          dynamic_scale=kind)
    R.fill(net).to(DEV)
    src, mask, qe, pos, h_w, dhs = R.gold_inputs(torch.float32)
    src, qe, pos = (t.to(DEV, BF).requires_grad_(True) for t in (src, qe, pos))
    hs, points = net(src, mask.to(DEV), qe, pos, h_w.to(DEV))
    hs.backward(dhs.to(DEV, hs.dtype))
    torch.cuda.synchronize()
    return net, hs.detach().double().cpu(), points.detach().double().cpu(), {"src": src.grad, "query_embed": qe.grad, "pos_embed": pos.grad}


def _rel(a, b, floor=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), floor, 1e-300))


@pytest.mark.parametrize("kind", R.TYPES)
def test_transformer_against_the_reference_fixture(kind):
    """the bounds are those of tests/test_gpu_detr.py::test_transformer_against_reference_golden - a bf16 transformer against its
    float64 / fp32 reference fixture, relative l2: 3e-2 for hs (and the points, an output of the same depth), 8e-2 for the input
    gradients, 1.5e-1 for parameter gradients; layer 0's self-attention in-projection weight (tgt = 0: a mathematically zero q / k / v
    weight gradient; the bias has a value part that is not zero and is compared like every other parameter) must be noise-small,
    below 3e-2 of the same parameter's gradient one layer up.  The RCDA module test's rule
    (twice a bf16 emulation of the whole module) would need a bf16 restatement of the whole transformer.  Row / column sums are
    compared at the scale of the tensor they sum (tests/test_smca_ref.py)."""
    gold = dict(np.load(GOLD))
    net, hs, points, gin = _module_run(kind)
    p = kind + "/"
    figures = [("hs", _rel(hs.numpy(), gold[p + "hs"]), 3e-2), ("points", _rel(points.numpy(), gold[p + "points"]), 3e-2),
               ("d query_embed", _rel(gin["query_embed"].double().cpu().numpy(), gold[p + "grad_in/query_embed"]), 8e-2)]
    for n in ("src", "pos_embed"):
        g = gin[n].double().cpu()
        for k, v in R.reduce_grad(g.numpy()).items():
            figures.append((f"d {n}/{k}", _rel(v, gold[f"{p}grad_in/{n}/{k}"], float(g.norm())), 8e-2))
    grads = {n: prm.grad.double().cpu() for n, prm in net.named_parameters()}
    for n, g in grads.items():
        if R.holds_param_grad(kind, n):
            for k, v in R.reduce_grad(g.numpy()).items():
                want = gold[f"{p}grad_param/{n}/{k}"]
                if n == "decoder.layers.0.self_attn.in_proj_weight":
                    up = float(grads[n.replace("layers.0", "layers.1")].norm())
                    figures.append((f"{n}/{k} (zero)", float(np.linalg.norm(v - want)) / up, 3e-2))
                else:
                    figures.append((f"{n}/{k}", _rel(v, want, float(g.norm())), 1.5e-1))
    bad = []
    for name, err, tol in figures:
        print(f"smca module {kind} {name:60s} {err:.3e} (allowed {tol:.1e})")
        if not err <= tol:
            bad.append((name, err, tol))
    assert not bad, bad


# ------------------------------------------------------------------ 7
def test_core_captured_equals_eager_bit_for_bit():
    from yolov7_d2_amd.modeling import smca_core
    ops = R.random_case(2, 2, 130, (13, 21), "type4", seed=13, negative=True)
    mask, dout = ops["mask"].to(DEV), ops["dout"].to(DEV, BF)

    def leaves():
        return ([ops[n].to(DEV, BF).requires_grad_(True) for n in ("q", "k", "v")]
                + [ops[n].to(DEV, F32).requires_grad_(True) for n in ("point", "coef")])

    def run(ts):
        for t in ts:
            t.grad = None
        o = smca_core(*ts, ops["map_hw"], 8.0, mask, ops["H"])
        o.backward(dout)
        return o

    # the eager result from leaves of its own, and nothing of its autograd graph kept: a leaf's gradient accumulator lives
    # as long as a graph that uses it and belongs to the stream it was created on - the captured backward must not find one
    # from the default stream (it would make that stream wait on the capturing one)
    ets = leaves()
    eo = run(ets)
    torch.cuda.synchronize()
    eager = [eo.detach().clone()] + [t.grad.clone() for t in ets]
    del eo, ets
    ts = leaves()
    step = lambda: run(ts)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = step()
    for _ in range(2):
        for t in ts:
            t.grad.fill_(NAN)
        o.detach().fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip([o.detach()] + [t.grad for t in ts], eager):
            assert torch.equal(x, y)
    r64 = R.core(ops)
    assert R.rel_l2(eager[0].double().cpu(), r64["O"]) < 1e-2
