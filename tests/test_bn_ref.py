"""CPU: tests/bn_ref.py - the float64 reference of the BatchNorm + SiLU ABI that tests/test_gpu_bn_exact.py holds the kernels
of csrc/bn_act.hip to - pinned to torch's float64 batch_norm + silu autograd (running statistics included), its bf16
rounding pinned to torch's, the conditions of the exact families checked on every case together with an fp32 emulation in
two summation orders that must reproduce the reference bit for bit, the derived sigmoid bounds checked against an fp32
emulation of sigmoidf_ over every finite bf16 argument, and the mutants checked against both kinds of criterion."""
import math

import pytest
import torch
import torch.nn.functional as F

import bn_ref as R

F64 = torch.float64


def test_bf16_rne_is_torchs_rounding_and_rounds_once():
    """every bf16 value is a fixed point; every midpoint between neighbours goes to the even one; random fp32 values round as
    torch's fp32 -> bf16 conversion does; a float64 just above a midpoint that fp32 would first round ONTO the midpoint still
    goes up (one rounding, from float64); overflow to inf from max + half an ulp; subnormals on the 2^-133 grid"""
    allv = R.all_finite_bf16().to(F64)
    assert torch.equal(R.bf16_rne(allv), allv)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(200000, generator=g) * torch.exp2(torch.randint(-140, 127, (200000,), generator=g).float())).float()
    x = x[torch.isfinite(x)]
    assert torch.equal(R.bf16_rne(x.to(F64)), x.to(torch.bfloat16).to(F64))
    pos = allv[(allv > 0)].sort().values
    mid = (pos[:-1] + pos[1:]) / 2
    r = R.bf16_rne(mid)
    even = torch.where((pos[:-1].to(torch.bfloat16).view(torch.int16) & 1) == 0, pos[:-1], pos[1:])
    assert torch.equal(r, even) and torch.equal(R.bf16_rne(-mid), -even)
    assert torch.equal(R.bf16_half_ulp(pos[:-1]), (pos[1:] - pos[:-1]) / 2)
    w = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -40, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, R.BF16_MAX + 2.0 ** 118, R.BF16_MAX + 2.0 ** 119,
                      2.0 ** -134, 3 * 2.0 ** -134, -0.0], dtype=F64)
    exp = torch.tensor([1 + 2.0 ** -7, 1.0, 1 + 2.0 ** -6, R.BF16_MAX, math.inf, 0.0, 2.0 ** -132, -0.0], dtype=F64)
    assert torch.equal(R.bf16_rne(w), exp)
    assert float(w[0].float()) == 1 + 2.0 ** -8          # the double-rounding trap is real: fp32 lands on the tie


@pytest.mark.parametrize("C,npix,nslots,act,res", [(24, 50, 3, 1, True), (8, 7, 16, 0, False), (40, 33, 1, 1, False), (264, 20, 5, 0, True)])
def test_reference_is_batch_norm_silu_autograd(C, npix, nslots, act, res):
    """forward prologue + apply, running statistics and nbt, backward sums + apply (dy, dgamma, dbeta, dres) against float64
    torch.nn.functional.batch_norm(training=True) + silu + residual add and its autograd, at 1e-11"""
    g = torch.Generator().manual_seed(C + npix)
    y = (torch.randn(npix, C, generator=g, dtype=F64) * 1.5 + 0.3).requires_grad_()
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).requires_grad_()
    beta = (torch.randn(C, generator=g, dtype=F64) * 0.1).requires_grad_()
    resid = torch.randn(npix, C, generator=g, dtype=F64).requires_grad_() if res else None
    da = torch.randn(npix, C, generator=g, dtype=F64)
    rm0, rv0 = torch.randn(C, generator=g, dtype=F64), torch.rand(C, generator=g, dtype=F64) + 0.5
    eps, mom = R.eps_double(R.EPS), 0.03
    rm, rv = rm0.clone(), rv0.clone()
    yn = F.batch_norm(y.t()[None], rm, rv, gamma, beta, True, mom, eps)[0].t()
    a = F.silu(yn) if act else yn
    if res:
        a = a + resid
    a.backward(da)
    # the accumulators: (sum y, sum y^2) spread over the slots, NaN in the unused ones
    CA = R.acc_c(C)
    acc = torch.full((R.SLOTS, CA, 2), math.nan, dtype=F64)
    yd = y.detach()
    chunks = torch.tensor_split(yd, nslots, dim=0)
    for k, ch in enumerate(chunks):
        acc[k, :C, 0], acc[k, :C, 1] = ch.sum(0), (ch * ch).sum(0)
    p = R.fwd_prologue(acc, nslots, npix, gamma.detach(), beta.detach(), R.EPS, mom, rm0, rv0, 7)
    tol = dict(rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(p.mean, yd.mean(0), **tol)
    torch.testing.assert_close(p.var, yd.var(0, unbiased=False), **tol)
    torch.testing.assert_close(p.rmean, rm, **tol)
    torch.testing.assert_close(p.rvar, rv, **tol)
    assert p.nbt == 8
    torch.testing.assert_close(R.fwd_apply(yd, p.scale, p.shift, act, None if resid is None else resid.detach()), a.detach(), **tol)
    s1, s2 = R.bwd_sums(da, yd, p.scale, p.shift, p.mean, p.invstd, act)
    dy, dg, db, dres = R.bwd_apply(da, yd, p.scale, p.shift, p.mean, p.invstd, gamma.detach(), s1, s2, npix, act,
                                   torch.ones_like(da) if res else None, 2 if res else 0)
    torch.testing.assert_close(dy, y.grad, **tol)
    torch.testing.assert_close(dg, gamma.grad, **tol)
    torch.testing.assert_close(db, beta.grad, **tol)
    if res:
        torch.testing.assert_close(dres, 1 + resid.grad, **tol)
    # eval mode: the affine of the running statistics
    sc, sh = R.eval_affine(gamma.detach(), beta.detach(), rm, rv, R.EPS)
    ye = F.batch_norm(yd.t()[None], rm, rv, gamma.detach(), beta.detach(), False, mom, eps)[0].t()
    torch.testing.assert_close(R.fwd_apply(yd, sc, sh, 0), ye, **tol)


def test_saturated_sigmoid_is_the_fp32_limit_of_the_true_one():
    """the limits the saturated family uses are what the true sigmoid rounds to in fp32 arithmetic of sigmoidf_'s form:
    1 + e == 1 from z = 32 up (e < 2^-24) and e = exp(-z) beyond the fp32 range from z = -100 down"""
    z = torch.tensor([32.0, 64.0, 2368.0, -100.0, -128.0, -2500.0], dtype=F64)
    e = torch.exp(-z)
    assert bool((e[:3] < 2.0 ** -25).all()) and bool((e[3:] > 3.4028235e38).all())
    assert torch.equal(R.sat_sigmoid(z), torch.tensor([1.0, 1, 1, 0, 0, 0], dtype=F64))
    assert torch.equal(R.act_grad(z, "sat"), torch.tensor([1.0, 1, 1, 0, 0, 0], dtype=F64))
    assert bool(R.sat_sigmoid(torch.tensor([31.0, -99.0], dtype=F64)).isnan().all())


def _fwd_fp32(c, o, r, flip):
    """the forward apply in fp32, a = bf16(act(y * scale + shift) + res)"""
    y, sc, sh = o.y.float(), r.scale.float(), r.shift.float()
    z = (sh + sc * y) if flip else (y * sc + sh)
    if c.act == "sat":
        z = z * R.sat_sigmoid(z.to(F64)).float()
    if o.res is not None:
        z = z + o.res.float()
    return z.to(torch.bfloat16).to(F64)


@pytest.mark.parametrize("c", R.fwd_cases() + [R.fwd_mutation_case()], ids=lambda c: c.name)
def test_forward_family_conditions_and_fp32_emulation(c):
    """the conditions hold on every forward case (three launches), the slot sums are exact in reversed order too, and an
    fp32 evaluation of the apply in either operand order rounds to the reference's bf16 values"""
    o = R.make_fwd_operands(c)
    r = R.fwd_reference(c, o, 3)
    R.assert_fwd_conditions(c, o, r)
    if c.train:
        n = R.norm_slots(c.nslots)
        assert torch.equal(R.slot_sums(o.acc[:n].flip(0), n)[:c.C], R.slot_sums(o.acc, n)[:c.C])
        for t in (r.scale, r.shift, r.mean, r.invstd):
            assert torch.equal(R.f32(t), t)
        if c.running != "none":
            assert all(torch.equal(R.f32(t), t) for t in r.rmean) and torch.equal(R.f32(r.rvar[0]), r.rvar[0])
            assert bool((r.rvar_tol[0] == 0).all()) and all(float((t / v).max()) < 10 * R.U32 for t, v in zip(r.rvar_tol[1:], r.rvar[1:]))
            assert r.nbt == ([o.nbt0 + 1, o.nbt0 + 2, o.nbt0 + 3] if c.running == "both" else [None] * 3)
    for flip in (False, True):
        assert torch.equal(_fwd_fp32(c, o, r, flip), r.a)


def test_forward_cap_case_makes_a_second_partial_trip():
    c = R.fwd_cap_case()
    C8, _, T = R.tpb(c.C)
    total = c.npix * C8
    assert R.ew_blocks(total) == 1024 and 1024 * T * 4 < total < 1024 * T * 5


def test_backward_cap_cases_give_the_apply_loop_a_third_item():
    for c in R.bwd_cap_cases():
        C8, _, T = R.tpb(c.C)
        total = c.npix * C8
        assert c.nblk == R.ew_blocks(total) == 1024 and 1024 * T * 2 < total < 1024 * T * 3


@pytest.mark.parametrize("c", R.bwd_cases() + R.bwd_cap_cases() + R.fused_capacity_cases() + [R.bwd_mutation_case()], ids=lambda c: c.name)
def test_backward_family_conditions_and_fp32_emulation(c):
    """the conditions hold on every backward case, and an fp32 evaluation with the channel sums taken in two different
    orders (torch's pairwise sum; a sequential sum over the reversed pixels, in blocks of 7) gives dy, dgamma, dbeta, dres
    bit for bit"""
    o = R.make_bwd_operands(c)
    r = R.bwd_reference(c, o)
    R.assert_bwd_conditions(c, o, r)
    f = lambda t: t.float()
    act = R.act_grad((o.y * o.scale + o.shift), c.act).float()
    dz = f(o.da) * act
    xh = (f(o.y) - f(o.mean)) * f(o.invstd)
    for order in (0, 1):
        if order == 0:
            s1, s2 = dz.sum(0), (dz * xh).sum(0)
        else:
            s1, s2 = torch.zeros(c.C), torch.zeros(c.C)
            for ch in torch.split((dz.flip(0)), 7):
                s1 = s1 + ch.sum(0)
            for ch in torch.split((dz * xh).flip(0), 7):
                s2 = s2 + ch.sum(0)
        k1 = (s1.to(F64) / o.count).float()
        k2 = (s2.to(F64) / o.count).float()
        dy = (f(o.gamma) * f(o.invstd)) * (dz - k1 - xh * k2)
        assert torch.equal(dy.to(torch.bfloat16).to(F64), r.dy)
        assert torch.equal(s2.to(F64), r.dgamma) and torch.equal(s1.to(F64), r.dbeta)
    if c.dres == 2:
        assert torch.equal((f(o.dres0) + f(o.da)).to(torch.bfloat16).to(F64), r.dres)
    elif c.dres == 1:
        assert torch.equal(r.dres, o.da)


def test_group_case_conditions():
    kinds = set()
    for g in R.group_cases():
        assert len(g.jobs) == g.n and len({(c.C, c.npix) for c in g.jobs}) == g.n
        kinds.add((g.kind, g.n))
        for c in g.jobs:
            if g.kind == 0:
                o = R.make_fwd_operands(c)
                R.assert_fwd_conditions(c, o, R.fwd_reference(c, o, 1))
            else:
                o = R.make_bwd_operands(c)
                R.assert_bwd_conditions(c, o, R.bwd_reference(c, o))
    assert kinds == {(k, n) for k in (0, 12, 3) for n in (1, 3, 8)}


def test_fused_capacity_cases_pin_the_grid_and_the_item_counts():
    """with the capacity of each case the launcher's arithmetic gives nb = cap in {1, 2, 15, 16, 17, 33}, and the threads hold
    0, 1, 13, 14, 15, 16, 17, 19 (and more) items: either side of R = 14 and R = 16, odd and even streaming tails"""
    nbs, items = set(), set()
    for c in R.fused_capacity_cases():
        nb = R.fused_blocks(c.npix, c.C, c.cap)
        assert nb == c.cap
        nbs.add(nb)
        items |= R.nmine_set(c.npix, c.C, nb)
    assert nbs == {1, 2, 15, 16, 17, 33}
    assert items >= {0, 1, 13, 14, 15, 16, 17, 19}, sorted(items)
    assert len({(nb - g + 15) // 16 for nb in (17, 33) for g in range(16)}) > 1        # uneven barrier groups
    w = R.barrier_expected([17, 17, 17])
    assert int(w.sum()) == 48 and int(w[64]) == 3 and int(w[64 * 16]) == 3 and int(w[64 * 17]) == 0
    assert int(R.barrier_expected([2])[64 * 3]) == 0


def test_leading_dimensions_differ_pairwise_in_one_case_per_entry_point():
    assert any(len(set(R.fwd_lds(c))) == 3 for c in R.fwd_cases())
    assert any(len(set(R.bwd_lds(c))) == 4 for c in R.bwd_cases())
    assert any(len(set(R.bwd_lds(c))) == 4 for c in R.fused_capacity_cases())
    for g in R.group_cases():
        if g.n > 1:
            assert any(len(set(R.fwd_lds(c) if g.kind == 0 else R.bwd_lds(c))) == (3 if g.kind == 0 else 4) for c in g.jobs)


def test_instantiation_table_is_complete():
    t = R.instantiations()
    assert len(t) == len(set(t)) == 2 * 4 * 2                   # 6 streaming + 2 one-launch, single and grouped
    assert R.kernel_name("bn_bwd_fused", "sat", True) == "bn_bwd_fused_group_kernel<1>"
    assert R.kernel_name("bn_bwd_fused", 0) == "bn_bwd_fused_kernel<0>" and R.kernel_name("bn_act_fwd", 1) in t


def test_sigmoid_bounds_hold_for_an_fp32_emulation_and_are_not_vacuous():
    """sigmoidf_'s expression in fp32 on the host (correctly rounded operations: inside the bound derived for 1-ulp
    hardware exp and rcp) over every finite bf16 argument: z * s and s * (1 + z * (1 - s)) stay inside silu_bound /
    silu_grad_bound before rounding to bf16.  The bounds are tight enough to mean something: below 2^-17 relative for SiLU
    over |z| <= 16 where |silu| >= 2^-20, i.e. 1/512 of the bf16 half-ulp that is added at the store."""
    z = R.all_finite_bf16().float()
    s = R.emulate_sigmoid_fp32(z)
    zd = z.to(F64)
    silu = zd * torch.sigmoid(zd)
    sd = torch.sigmoid(zd)
    grad = sd * (1 + zd * (1 - sd))
    e1 = ((z * s).to(F64) - silu).abs()
    e2 = ((s * (1.0 + z * (1.0 - s))).to(F64) - grad).abs()
    b1, b2 = R.silu_bound(zd), R.silu_grad_bound(zd)
    print("fp32 emulation / bound: silu %.3f, silu' %.3f" % (float((e1 / b1).max()), float((e2 / b2).max())))
    assert bool((e1 <= b1).all()) and bool((e2 <= b2).all())
    m = (zd.abs() <= 16) & (silu.abs() >= 2.0 ** -20)
    rel = float((b1[m] / silu[m].abs()).max())
    print("largest relative silu bound over |z| <= 16: 2^%.2f" % math.log2(rel))
    assert rel < 2.0 ** -17


def test_mutants_differ_from_the_reference_and_pass_the_old_criteria():
    """on the CPU, mutant against reference: every mutant's `exact` view differs from the reference in at least one output
    element, and its `old` view passes the criteria of the older tests"""
    c = R.fwd_mutation_case()
    o = R.make_fwd_operands(c)
    r = R.fwd_reference(c, o, 1)
    ref = R.fwd_outputs(r)
    muts = R.fwd_mutants(c, o, r)
    assert len(muts) == 3
    for name, (exact, old) in muts.items():
        assert not all(R.same(exact[k], ref[k]) for k in ref), name
        assert R.old_criteria_accept(ref, old), name
    c = R.bwd_mutation_case()
    o = R.make_bwd_operands(c)
    r = R.bwd_reference(c, o)
    ref = R.bwd_outputs(r)
    ldda = R.bwd_lds(c)[0]
    flat = torch.full((c.npix * ldda,), math.nan, dtype=F64)
    flat.view(c.npix, ldda)[:, :c.C] = o.da
    for Rr in (14, 16):
        muts = R.bwd_mutants(c, o, r, R.fused_blocks(c.npix, c.C, c.cap), Rr, flat)
        assert len(muts) == 4
        for name, (exact, old) in muts.items():
            assert not all(R.same(exact[k], ref[k]) for k in ref), name
            assert R.old_criteria_accept(ref, old), name


@pytest.mark.parametrize("nc", R.numerics_cases(), ids=lambda c: c.name)
def test_numerics_bounds_hold_for_the_fp32_emulation(nc):
    """random data: the fp32 emulation of the kernels' expressions (statistics rounded to fp32 as the device would hand them
    over) stays inside the derived elementwise bounds; the bounds are not vacuous: the median bound of a and dy is below one
    bf16 ulp of the value (2^-7 relative)"""
    o = R.make_numerics_operands(nc)
    p = R.fwd_prologue(o.acc, nc.nslots, o.count, o.gamma, o.beta, R.EPS, R.MOMENTUM, o.rmean0, o.rvar0)
    sc, sh, mu, is_ = R.f32(p.scale), R.f32(p.shift), R.f32(p.mean), R.f32(p.invstd)
    sb = R.stats_bounds(p, o.gamma, o.beta, R.MOMENTUM, o.rmean0, o.rvar0)
    for name, dev in (("scale", sc), ("shift", sh), ("mean", mu), ("invstd", is_)):
        assert bool(((dev - getattr(p, name)).abs() <= getattr(sb, name)).all()), name
    a, ab = R.numerics_fwd(o, sc, sh)
    ref, bound = R.numerics_bwd(o, sc, sh, mu, is_, o.gamma, R.chain_length(nc.npix, nc.C, 1), nc.dres)
    ref["a"], bound["a"] = a, ab
    emu = R.emulate_numerics_fp32(o, sc, sh, mu, is_, o.gamma, nc.dres)
    for k in ref:
        ratio = float(((emu[k] - ref[k]).abs() / bound[k].clamp_min(1e-300)).max()) if k != "dres" or nc.dres == 2 else 0.0
        print(nc.name, k, "emulation / bound %.3f" % ratio)
        assert bool(((emu[k] - ref[k]).abs() <= bound[k]).all()), k
    for k in ("a", "dy"):
        assert float((bound[k] / ref[k].abs().clamp_min(1e-30)).median()) < 2.0 ** -7
