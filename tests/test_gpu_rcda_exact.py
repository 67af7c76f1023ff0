"""GPU: row-column decoupled attention (csrc/rcda.hip, modeling/rcda.py) against tests/rcda_ref.py.

Exact families (conditions checked on the CPU in tests/test_rcda_ref.py): `uniform` - all scores 0 with power-of-two live
counts, the output and all five gradients equal the float64 reference rounded once, bit for bit; `gather` - one-hot softmaxes,
O = V[h*, w*], zero query / key gradients and dV = the scatter of the cotangent.  (The uniform family masks EVERY image where
H or W is not a power of two - 1 / 35 is not dyadic; the gather and the random cases mask image 1 only.)  Every operand sits
between NaN guards and every output between sentinel guards that must come back untouched.

Random operands against float64: the allowed error of every quantity is twice the error of the bf16-rounding fp32 restatement
(rcda_ref.core / module with emulate=True) against float64 on the same operands, computed here, as relative l2 and as
maximum over the reference's maximum; the factor 2 covers a device exp2 and accumulation orders whose last bits differ."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rcda_ref as R
from yolov7_d2_amd import _lib as L

DEV = "cuda"
GUARD = 64
SENT = -1536.0      # exact in bf16 and fp32
NAMES = R.CORE_NAMES
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rcda.npz")
INPUTS = ("query_row", "query_col", "key_row", "key_col", "value")
PARAMS = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")


class Buf:
    """a contiguous tensor between two guards: NaN around an operand, a sentinel in and around an output"""

    def __init__(self, shape, dtype, src=None):
        n = int(np.prod(shape))
        fill = SENT if src is None else (1 if dtype == torch.uint8 else float("nan"))     # (uint8 has no NaN: padded flags)
        self.flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.flat[GUARD:GUARD + n].view(*shape)
        if src is not None:
            self.t.copy_(src.to(dtype))
        self.is_out = src is None

    def guards_ok(self):
        g = torch.cat([self.flat[:GUARD], self.flat[-GUARD:]])
        if self.is_out:
            return bool((g == SENT).all())
        return bool((g == 1).all()) if g.dtype == torch.uint8 else bool(torch.isnan(g).all())

    def untouched(self):
        return bool((self.flat == SENT).all())


def make_desc(ops, mask_row, mask_col, heads):
    """device buffers + descriptor of one case: operands, dout to be filled, outputs, workspace"""
    B, Lq, E = ops["q_row"].shape
    H, W = ops["v"].shape[1:3]
    bufs = {n: Buf(ops[n].shape, torch.bfloat16, ops[n]) for n in NAMES}
    bufs["o"] = Buf((B, Lq, E), torch.bfloat16)
    bufs["lse_row"], bufs["lse_col"] = Buf((B, heads, Lq), torch.float32), Buf((B, heads, Lq), torch.float32)
    for n in NAMES:
        bufs["d" + n] = Buf(ops[n].shape, torch.bfloat16)
    if mask_row is not None:
        bufs["mask_row"], bufs["mask_col"] = Buf((B, W), torch.uint8, mask_row), Buf((B, H), torch.uint8, mask_col)
    d = L.mi_rcda_desc()
    for n in NAMES:
        setattr(d, n, bufs[n].t.data_ptr())
        setattr(d, "d" + n, bufs["d" + n].t.data_ptr())
    d.o, d.lse_row, d.lse_col = bufs["o"].t.data_ptr(), bufs["lse_row"].t.data_ptr(), bufs["lse_col"].t.data_ptr()
    if mask_row is not None:
        d.mask_row, d.mask_col = bufs["mask_row"].t.data_ptr(), bufs["mask_col"].t.data_ptr()
    d.B, d.heads, d.L, d.H, d.W, d.E = B, heads, Lq, H, W, E
    d.ldq = d.ldk = d.ldv = d.ldo = E
    d.scale = R.HD ** -0.5
    need = L.lib().mi_rcda_bwd_ws_bytes(C.byref(d))
    assert need == B * heads * (H + W) * ((Lq + 31) // 32 * 32) * 2
    bufs["ws"] = Buf((need // 2,), torch.bfloat16)
    d.ws, d.ws_bytes = bufs["ws"].t.data_ptr(), need
    return d, bufs


def run_core(ops, dout, mask_row, mask_col, heads):
    """forward + backward through the C entries on guarded buffers -> (o, {name: gradient}) on the host, float64"""
    d, bufs = make_desc(ops, mask_row, mask_col, heads)
    bufs["dout"] = Buf(dout.shape, torch.bfloat16, dout)
    d.dout = bufs["dout"].t.data_ptr()
    L.check(L.lib().mi_rcda_fwd(C.byref(d), L.stream_ptr()), "mi_rcda_fwd")
    L.check(L.lib().mi_rcda_bwd(C.byref(d), L.stream_ptr()), "mi_rcda_bwd")
    torch.cuda.synchronize()
    for n, b in bufs.items():
        assert b.guards_ok(), n
    o = bufs["o"].t.double().cpu()
    grads = {n: bufs["d" + n].t.double().cpu() for n in NAMES}
    for n, x in [("o", o)] + list(grads.items()):
        assert bool(torch.isfinite(x).all()) and not bool((x == SENT).all()), n       # every element written
    return o, grads, bufs


def stored(x):
    """what a bf16 store of the float64 value x holds, through the fp32 the kernels accumulate in"""
    return x.float().to(torch.bfloat16).double()


SCALE32 = float(np.float32(R.HD ** -0.5))       # the scale the kernels multiply by


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.EXACT_SHAPES)
def test_uniform_family_bit_exact(shape):
    heads = shape[1]
    ops, dout, mr, mc = R.uniform_case(*shape, seed=1)
    # the reference at scale 1, where every float64 operation of a uniform case is exact (dyadic numbers of a few bits); the
    # scores are 0 at any scale and the query / key gradients are linear in it: one exact multiplication by the fp32 scale
    # afterwards.  (Evaluated at the scale itself, float64 leaves 1e-17 where sums of non-dyadic terms cancel to exactly 0.)
    o_ref, g_ref = R.core_with_grads(ops, dout, mr, mc, heads, torch.float64, False, scale=1.0)
    for n in ("q_row", "q_col", "k_row", "k_col"):
        g_ref[n] = g_ref[n] * SCALE32
    o, g, bufs = run_core(ops, dout, mr, mc, heads)
    assert torch.equal(o, stored(o_ref)), float((o - o_ref).abs().max())
    for n in NAMES:
        assert torch.equal(g[n], stored(g_ref[n])), (n, float((g[n] - g_ref[n]).abs().max()))
    # lse in base-2 units: log2 of the live count
    live = ((~mr).sum(1).double().log2()[:, None, None], (~mc).sum(1).double().log2()[:, None, None])
    assert torch.equal(bufs["lse_row"].t.double().cpu(), live[0].expand(-1, heads, shape[2]))
    assert torch.equal(bufs["lse_col"].t.double().cpu(), live[1].expand(-1, heads, shape[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.EXACT_SHAPES)
def test_gather_family_bit_exact(shape):
    heads = shape[1]
    ops, dout, mr, mc, hs, ws = R.gather_case(*shape, seed=2)
    eo, edv = R.gather_expected(ops, dout, hs, ws, heads)
    o, g, _ = run_core(ops, dout, mr, mc, heads)
    assert torch.equal(o, eo), float((o - eo).abs().max())
    assert torch.equal(g["v"], stored(edv))
    for n in ("q_row", "q_col", "k_row", "k_col"):
        assert float(g[n].abs().max()) == 0, n


RANDOM_SHAPES = [(2, 2, 70, 5, 7), (1, 8, 130, 25, 42)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_random_operands_within_twice_the_emulation_floor(shape):
    heads = shape[1]
    ops, dout, mr, mc = R.random_core_case(*shape, seed=7)
    o64, g64 = R.core_with_grads(ops, dout, mr, mc, heads, torch.float64, False)
    o32, g32 = R.core_with_grads(ops, dout, mr, mc, heads, torch.float32, True)
    o, g, _ = run_core(ops, dout, mr, mc, heads)
    fails = []
    for n, got, emu, ref in [("o", o, o32, o64)] + [("d" + k, g[k], g32[k], g64[k]) for k in NAMES]:
        for metric in (R.rel_l2, R.rel_max):
            floor, err = metric(emu, ref), metric(got, ref)
            print(f"rcda random {shape} {n:8s} {metric.__name__}: floor {floor:.3e}  device {err:.3e}")
            assert floor > 0
            if not err <= 2 * floor:
                fails.append((n, metric.__name__, floor, err))
    assert not fails, fails


@pytest.mark.gpu
def test_backward_is_bit_reproducible_and_dead_queries_give_zero():
    shape = (2, 2, 70, 5, 7)
    ops, dout, mr, mc = R.random_core_case(*shape, seed=9)
    mr[1, :] = True                     # image 1: every row key padded
    o1, g1, _ = run_core(ops, dout, mr, mc, 2)
    o2, g2, _ = run_core(ops, dout, mr, mc, 2)
    assert torch.equal(o1, o2) and all(torch.equal(g1[n], g2[n]) for n in NAMES)
    assert float(o1[1].abs().max()) == 0 and float(o1[0].abs().max()) > 0
    for n in NAMES:
        assert float(g1[n][1].abs().max()) == 0 and float(g1[n][0].abs().max()) > 0, n
    o64, g64 = R.core_with_grads(ops, dout, mr, mc, 2, torch.float64, False)
    assert R.rel_l2(o1, o64) < 1e-2 and all(R.rel_l2(g1[n], g64[n]) < 3e-2 for n in NAMES)


@pytest.mark.gpu
def test_refused_calls_leave_the_outputs_untouched():
    ops, dout, mr, mc = R.random_core_case(2, 2, 70, 5, 7, seed=3)
    d, bufs = make_desc(ops, mr, mc, 2)
    bufs["dout"] = Buf(dout.shape, torch.bfloat16, dout)
    d.dout = bufs["dout"].t.data_ptr()
    lib = L.lib()
    outs = ["o", "lse_row", "lse_col", "ws"] + ["d" + n for n in NAMES]

    def refused(word, **kw):
        saved = {k: getattr(d, k) for k in kw}
        for k, v in kw.items():
            setattr(d, k, v)
        for fn in (lib.mi_rcda_fwd, lib.mi_rcda_bwd):
            assert fn(C.byref(d), L.stream_ptr()) == -1 and word in lib.mi_last_error(), (kw, lib.mi_last_error())
        for k, v in saved.items():
            setattr(d, k, v)

    refused(b"heads *", E=96)
    refused(b"positive", L=0)
    refused(b"served size", H=97)
    refused(b"null", q_col=None)
    refused(b"aligned", v=bufs["v"].t.data_ptr() + 2)
    refused(b"ldq", ldq=60)
    d.ws_bytes -= 2
    assert lib.mi_rcda_bwd(C.byref(d), L.stream_ptr()) == -1 and b"workspace" in lib.mi_last_error()
    torch.cuda.synchronize()
    for n in outs:
        assert bufs[n].untouched(), n


# ------------------------------------------------------------------ the module
def _gold_module():
    from yolov7_d2_amd.modeling import MultiheadRCDA
    gold = dict(np.load(GOLD))
    m = MultiheadRCDA(64, int(gold["heads"]))
    m.load_state_dict({k: torch.from_numpy(gold["param/" + k]).float() for k in PARAMS})
    return gold, m.to(DEV)


def _module_run(m, gold):
    xs = [torch.from_numpy(gold["in/" + k]).to(DEV, torch.bfloat16).requires_grad_(True) for k in INPUTS]
    m.zero_grad(set_to_none=True)
    out, w = m(*xs, key_padding_mask=torch.from_numpy(gold["mask"]).to(DEV))
    assert w is None
    out.backward(torch.from_numpy(gold["dout"]).to(DEV, torch.bfloat16))
    torch.cuda.synchronize()
    res = {"out": out.detach()}
    res.update({"grad_in/" + k: x.grad for k, x in zip(INPUTS, xs)})
    res.update({"grad_param/" + k: p.grad for k, p in m.named_parameters()})
    return {k: v.double().cpu() for k, v in res.items()}


@pytest.mark.gpu
def test_module_against_the_reference_fixture():
    gold, m = _gold_module()
    got = _module_run(m, gold)
    # the floor: the module restated with bf16 storage, fp32, on the same operands
    xs = [torch.from_numpy(gold["in/" + k]).float().requires_grad_(True) for k in INPUTS]
    ps = {k: torch.from_numpy(gold["param/" + k]).float().requires_grad_(True) for k in PARAMS}
    out = R.module(ps, *xs, torch.from_numpy(gold["mask"]), int(gold["heads"]), emulate=True)
    out.backward(torch.from_numpy(gold["dout"]).float())
    emu = {"out": out.detach()}
    emu.update({"grad_in/" + k: x.grad for k, x in zip(INPUTS, xs)})
    emu.update({"grad_param/" + k: p.grad for k, p in ps.items()})
    assert got["out"].shape == gold["out"].shape == (70, 2, 64)
    fails = []
    for k in emu:
        ref = torch.from_numpy(gold[k])
        for metric in (R.rel_l2, R.rel_max):
            floor, err = metric(emu[k], ref), metric(got[k], ref)
            print(f"rcda module {k:28s} {metric.__name__}: floor {floor:.3e}  device {err:.3e}")
            if not err <= 2 * floor:
                fails.append((k, metric.__name__, floor, err))
    assert not fails, fails


@pytest.mark.gpu
def test_module_eval_no_grad_and_dropout_modes():
    gold, m = _gold_module()
    from yolov7_d2_amd.modeling import MultiheadRCDA
    xs = [torch.from_numpy(gold["in/" + k]).to(DEV, torch.bfloat16) for k in INPUTS]
    mask = torch.from_numpy(gold["mask"]).to(DEV)
    train_out = m(*xs, key_padding_mask=mask)[0]
    assert train_out.grad_fn is not None
    m.eval()
    assert torch.equal(m(*xs, key_padding_mask=mask)[0], train_out)
    with torch.no_grad():
        ng = m(*xs, key_padding_mask=mask)[0]
    assert ng.grad_fn is None and not ng.requires_grad and torch.equal(ng, train_out)
    d = MultiheadRCDA(64, 2, dropout=0.1).to(DEV)
    d.load_state_dict(m.state_dict())
    assert torch.equal(d.eval()(*xs, key_padding_mask=mask)[0], train_out)
    with pytest.raises(NotImplementedError, match="dropout"):
        d.train()(*xs, key_padding_mask=mask)
    # no mask at all
    assert bool(torch.isfinite(m(*xs)[0].float()).all())


@pytest.mark.gpu
def test_module_step_captured_equals_eager_bit_for_bit():
    gold, m = _gold_module()
    eager = _module_run(m, gold)
    xs = [torch.from_numpy(gold["in/" + k]).to(DEV, torch.bfloat16).requires_grad_(True) for k in INPUTS]
    mask = torch.from_numpy(gold["mask"]).to(DEV)
    dout = torch.from_numpy(gold["dout"]).to(DEV, torch.bfloat16)

    def step():
        for t in xs + list(m.parameters()):
            t.grad = None
        out = m(*xs, key_padding_mask=mask)[0]
        out.backward(dout)
        return out

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    from yolov7_d2_amd.ops import WgradBatch
    graph = torch.cuda.CUDAGraph()
    with WgradBatch.step_capture():             # (the grouped weight gradients' job tables, as graph_step.py captures a step)
        with torch.cuda.graph(graph):
            out = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        res = {"out": out.detach()}
        res.update({"grad_in/" + k: x.grad for k, x in zip(INPUTS, xs)})
        res.update({"grad_param/" + k: p.grad for k, p in m.named_parameters()})
        for k, v in res.items():
            assert torch.equal(v.double().cpu(), eager[k]), k
