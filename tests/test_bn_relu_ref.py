"""CPU: the float64 restatement of the BatchNorm + ReLU ABI (tests/bn_relu_ref.py) equals torch's float64 autograd of
relu(batch_norm(y1) + batch_norm(y2)), of relu(batch_norm(y1) + res) and of the plain layer, with and without the ReLU; and
every case of the exact GPU test builds: the conditions of its operand families hold on the reference."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as B
import bn_relu_ref as R

F64 = torch.float64
EPS = 1e-5


def _prologue(y, gamma, beta, nslots):
    """statistics through the ABI's accumulators: the sums split over the slots, then bn_ref.fwd_prologue"""
    C, CA = y.shape[1], B.acc_c(y.shape[1])
    s1, s2 = R.stats(y)
    acc = torch.zeros(B.SLOTS, CA, 2, dtype=F64)
    w = torch.rand(nslots, 1, dtype=F64)
    w = w / w.sum()
    acc[:nslots, :C, 0] = w * s1
    acc[:nslots, :C, 1] = w * s2
    return B.fwd_prologue(acc, nslots, y.shape[0], gamma, beta, EPS)


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("relu", [0, 1])
def test_restatement_equals_float64_autograd(form, relu):
    g = torch.Generator().manual_seed(7 + relu)
    n, C = 96, 24
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    y = [(rnd(n, C) * 2 + 0.5).requires_grad_() for _ in range(2 if form == "two" else 1)]
    gamma = [(rnd(C) + 1.5).requires_grad_() for _ in y]
    beta = [rnd(C).requires_grad_() for _ in y]
    res = rnd(n, C).requires_grad_() if form == "res" else None
    bn = lambda k: F.batch_norm(y[k].t()[None], None, None, gamma[k], beta[k], True, 0.1, EPS)[0].t()
    z = bn(0)
    if form == "two":
        z = z + bn(1)
    if form == "res":
        z = z + res
    out = torch.relu(z) if relu else z
    da = rnd(n, C)
    out.backward(da)
    p = [_prologue(y[k].detach(), gamma[k].detach(), beta[k].detach(), 1 + 3 * k) for k in range(len(y))]
    a = R.fwd(y[0].detach(), p[0].scale, p[0].shift, relu, *((y[1].detach(), p[1].scale, p[1].shift) if form == "two" else ()),
              res=None if res is None else res.detach())
    assert torch.allclose(a, out.detach(), rtol=1e-12, atol=1e-12)
    dz = R.dz_of(da, a, relu)
    for k in range(len(y)):
        s1, s2, dy = R.bwd_norm(dz, y[k].detach(), p[k].mean, p[k].invstd, gamma[k].detach(), float(n))
        assert torch.allclose(dy, y[k].grad, rtol=1e-10, atol=1e-12)
        assert torch.allclose(s2, gamma[k].grad, rtol=1e-10, atol=1e-12) and torch.allclose(s1, beta[k].grad, rtol=1e-10, atol=1e-12)
    if res is not None:
        assert torch.equal(R.bwd_res(dz), res.grad)
        d0 = rnd(n, C)
        assert torch.equal(R.bwd_res(dz, d0), d0 + res.grad)


def test_both_residual_kinds_are_refused_by_the_restatement_too():
    y = torch.zeros(4, 8, dtype=F64)
    v = torch.ones(8, dtype=F64)
    with pytest.raises(AssertionError):
        R.fwd(y, v, v, 1, y, v, v, res=y)


def test_stats_equal_float64_sums():
    x = R.stats_case(R.Shape(24, 64, 1), 3)
    s1, s2 = R.stats(x)
    assert torch.equal(s1, x.sum(0)) and torch.equal(s2, (x * x).sum(0))


@pytest.mark.parametrize("s", R.shapes(), ids=R.shape_id)
def test_every_exact_case_builds(s):
    """the families' conditions are asserted while a case is built (bn_ref.assert_*_conditions, the z1 + z2 grid, the mask)"""
    seed = R.shapes().index(s)
    for form in R.FORMS:
        for relu in (0, 1):
            for train in (True, False):
                k = R.fwd_case(s, form, relu, train, seed)
                assert k.a.shape == (s.npix, s.C)
            for mode in ((0,) if form != "res" else (1, 2)):
                k = R.bwd_case(s, form, relu, mode, seed)
                assert len(k.r) == (2 if form == "two" else 1)
                if relu:
                    assert bool((k.dz != k.da).any())
