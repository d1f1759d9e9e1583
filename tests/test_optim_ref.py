"""CPU: the float64 restatements of tests/optim_ref.py against torch.optim.Adam / AdamW and torch.norm run in float64, the
conditioning of every case table entry, and the proof that the bound of tests/test_gpu_optim.py can fail: a step evaluated
with a neighbouring step count, or with the betas swapped, lies outside it."""
import math

import pytest
import torch

from tests import optim_ref as R

LR, B1, B2, EPS = R.LR, R.B1, R.B2, R.EPS


def _torch_steps(c, decoupled, wd, grad_scale, coef, steps):
    """torch.optim on float64 copies, with the betas / lr / eps / wd the C ABI receives; the gradient of step k is g * (k + 1)"""
    ref = torch.nn.Parameter(c["p"].double().clone())
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([ref], lr=R.f32(LR), betas=(R.f32(B1), R.f32(B2)), eps=R.f32(EPS),
                                                                 weight_decay=R.f32(wd), foreach=False)
    out = []
    for k in range(steps):
        ref.grad = c["g"].double() * (k + 1) * R.f32(grad_scale) * coef
        opt.step()
        st = opt.state[ref]
        out.append((ref.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return out


@pytest.mark.parametrize("name", sorted(R.OPTIONS))
def test_adam_step64_is_torch_adam_in_float64(name):
    decoupled, wd, grad_scale, clip_mult = R.OPTIONS[name]
    c = R.adam_case("opt-%s-1027" % name, 1027)
    steps = 3
    # torch clips before the optimizer sees the gradient; here the coefficient is part of the step.  One gnorm for all steps:
    # the restatement takes it as an input
    gnorm = R.f32(R.grad_norm64(c["g"], grad_scale))
    clip = clip_mult * gnorm
    coef = min(1.0, R.f32(clip) / (gnorm + 1e-6)) if clip > 0 else 1.0
    want = _torch_steps(c, decoupled, wd, grad_scale, coef, steps)
    p, m, v = c["p"].double(), c["m"].double(), c["v"].double()
    for k in range(steps):
        p, m, v, u = R._adam(p, c["g"].double() * (k + 1), m, v, k + 1, LR, B1, B2, EPS, wd, decoupled, grad_scale, clip, gnorm,
                             torch.float64)
        for got, w, what in zip((p, m, v), want[k], "pmv"):
            assert R.rel(got, w) < 1e-12, (k, what, R.rel(got, w))
    assert float(u.abs().max()) > 0


def test_twin_is_torch_adam_in_float32():
    """the twin is the same single-tensor path on float32 tensors: against torch.optim.Adam in float32 it differs by roundings
    only (torch fuses some products), far below what it differs from float64 by"""
    c = R.adam_case("twin", 1027)
    ref = torch.nn.Parameter(c["p"].clone())
    opt = torch.optim.Adam([ref], lr=R.f32(LR), betas=(R.f32(B1), R.f32(B2)), eps=R.f32(EPS), foreach=False)
    ref.grad = c["g"].clone()
    opt.step()
    p32 = R.adam_step32(c["p"], c["g"], c["m"], c["v"], 1, LR, B1, B2, EPS, 0.0, False, 1.0, 0.0, 0.0)[0]
    p64 = R.adam_step64(c["p"], c["g"], c["m"], c["v"], 1, LR, B1, B2, EPS, 0.0, False, 1.0, 0.0, 0.0)[0]
    assert R.rel(p32, ref.detach()) <= 4 * R.FLOOR
    assert R.rel(ref.detach(), p64) <= R.twin_bound(p32, p64)


def test_case_tables_are_well_conditioned():
    # clip coefficients stay clear of 1: which side of the threshold a case is on does not hang on a rounding
    for name, (_, _, grad_scale, clip_mult) in R.OPTIONS.items():
        if clip_mult > 0:
            for n in R.OPTION_SIZES:
                g = R.adam_case("opt-%s-%d" % (name, n), n)["g"]
                gnorm = R.grad_norm64(g, grad_scale)
                coef = clip_mult * gnorm / (gnorm + 1e-6)
                assert abs(coef - 1.0) > 0.4, (name, n, coef)
    # every group in every pass of the 512 x 256-quad grid and in the scalar tail, wherever there are three elements to hold them
    per_pass = 512 * 256 * 4
    for n in R.SIZES:
        grp = R.group(n)
        tail0 = n // 4 * 4
        pieces = [(lo, min(lo + per_pass, tail0)) for lo in range(0, tail0, per_pass)] + [(tail0, n)]
        for lo, hi in pieces:
            if hi - lo >= 3:
                assert sorted(set(grp[lo:hi].tolist())) == [0, 1, 2], (n, lo, hi)
    c = R.adam_case("block1-1027", 1027)
    g = c["g"]
    nz = g[g != 0].abs()
    assert int((g == 0).sum()) > 50 and float(nz.min()) < 1e-5 and float(nz.max()) > 10.0
    assert bool((c["p"][c["grp"] == 0] == 0).all()) and bool((c["p"][c["grp"] != 0] != 0).all())
    # moments of the step-count cases: non-zero everywhere, v positive
    c = R.adam_case("step-10", R.STEP_N[0], with_moments=True)
    assert bool((c["m"] != 0).all()) and bool((c["v"] > 0).all())


def test_zero_gradient_zero_moment_is_the_identity():
    c = R.adam_case("block1-1027", 1027)
    p, m, v, u = R.adam_step64(c["p"], c["g"], c["m"], c["v"], 1, LR, B1, B2, EPS, 0.0, False, 1.0, 0.0, 0.0)
    z = c["g"] == 0
    assert bool((u[z] == 0).all()) and torch.equal(p[z], c["p"][z].double()) and bool((m[z] == 0).all()) and bool((v[z] == 0).all())


def test_bc_term():
    # t = 1: 2^-23 (9 + 999 / 2) with the float betas; decreasing in t; nothing left once b2^t is gone
    assert abs(R.bc_term(B1, B2, 1) / (2.0 ** -23 * (9.0 + 499.5)) - 1.0) < 1e-4
    vals = [R.bc_term(B1, B2, t) for t in R.STEP_COUNTS]
    assert all(a > b for a, b in zip(vals, vals[1:]))
    assert vals[-1] < 1e-40
    # it is the first-order effect of a relative error 2^-23 in b^t: perturb b^t in the float64 step and compare
    for t in (2, 10, 1000):
        q1, q2 = R.f32(B1) ** t, R.f32(B2) ** t
        e = 2.0 ** -23
        exact = (1 - q1) / (1 - q1 * (1 + e)) * math.sqrt((1 - q2 * (1 + e)) / (1 - q2))       # eps = 0: update ~ sqrt(bc2) / bc1
        worst = (1 - q1) / (1 - q1 * (1 + e)) * math.sqrt((1 - q2 * (1 - e)) / (1 - q2))
        assert abs(exact - 1.0) <= R.bc_term(B1, B2, t) * 1.001
        assert abs(worst - 1.0) == pytest.approx(R.bc_term(B1, B2, t), rel=1e-3)


def _step_case(t):
    c = R.adam_case("step-%d" % t, R.STEP_N[0], with_moments=True)
    args = (LR, B1, B2, EPS, 0.0, False, 1.0, 0.0, 0.0)
    with R.one_thread():
        r64 = R.adam_step64(c["p"], c["g"], c["m"], c["v"], t, *args)
        r32 = R.adam_step32(c["p"], c["g"], c["m"], c["v"], t, *args)
    z = c["grp"] == 0
    return c, r64, r32, z, R.update_bound(r32[0][z], r64[0][z], B1, B2, t)


@pytest.mark.parametrize("t,alt", [(t, a) for t in R.STEP_COUNTS for a in ("t-1", "t+1", "swapped") if not (t == 1 and a == "t-1")])
def test_a_wrong_step_count_or_swapped_betas_is_outside_the_bound(t, alt):
    """the bound the GPU test holds the update to (twin_bound + bc_term, on the p = 0 group) separates step t from steps
    t - 1 and t + 1 and from a step with beta1 and beta2 exchanged.  (There is no step 0: (1, "t-1") is not a case.)"""
    c, r64, r32, z, bound0 = _step_case(t)
    if alt != "swapped" and 1.0 - R.f32(B2) ** (t - 1) == 1.0:
        pytest.skip("1 - beta^t is exactly 1 in double at t - 1, t and t + 1 = %d: beta^t has underflowed below 2^-53, the step "
                    "count no longer enters the update and no bound can tell two counts apart" % (t + 1))
    if alt == "swapped":
        wrong = R.adam_step64(c["p"], c["g"], c["m"], c["v"], t, LR, B2, B1, EPS, 0.0, False, 1.0, 0.0, 0.0)
    else:
        wrong = R.adam_step64(c["p"], c["g"], c["m"], c["v"], t + (1 if alt == "t+1" else -1), LR, B1, B2, EPS, 0.0, False, 1.0, 0.0, 0.0)
    dev = R.rel(wrong[0][z], r64[0][z])
    print("t=%d %s: update off by %.3e, bound %.3e (twin %.3e + bc_term %.3e)" % (
        t, alt, dev, bound0, bound0 - R.bc_term(B1, B2, t), R.bc_term(B1, B2, t)))
    assert dev > 2.0 * bound0, (dev, bound0)
    if alt == "swapped":        # and the moments give it away on their own
        assert R.rel(wrong[1], r64[1]) > R.twin_bound(r32[1], r64[1]) and R.rel(wrong[2], r64[2]) > R.twin_bound(r32[2], r64[2])


def test_twin_is_inside_the_elementwise_allowance():
    """the elementwise allowance of the p != 0 groups, MARGIN roundings of p plus |u64| times the update's bound, holds for a
    float32 evaluation of the step at every step count and option -- elements whose sums cancel included"""
    cases = [("step-%d" % t, R.STEP_N[0], True, t, (0.0, False, 1.0)) for t in R.STEP_COUNTS]
    cases += [("opt-%s-1027" % k, 1027, False, 1, (wd, dec, gs)) for k, (dec, wd, gs, _) in R.OPTIONS.items()]
    for tag, n, moments, t, (wd, dec, gs) in cases:
        c = R.adam_case(tag, n, with_moments=moments)
        args = (t, LR, B1, B2, EPS, wd, dec, gs, 0.0, 0.0)
        r64, r32 = R.adam_step64(c["p"], c["g"], c["m"], c["v"], *args), R.adam_step32(c["p"], c["g"], c["m"], c["v"], *args)
        z = c["grp"] == 0
        allow = R.others_allowance(r64[0], r64[3], R.update_bound(r32[3][z], r64[3][z], B1, B2, t))
        assert bool(((r32[0].double() - r64[0]).abs()[~z] <= allow[~z]).all()), tag


@pytest.mark.parametrize("n", R.NORM_SIZES)
def test_grad_norm64_is_torch_norm_in_float64(n):
    for scale in R.NORM_SCALES:
        g = R.norm_case("n%d" % n, n)
        x = (g * torch.tensor(scale, dtype=torch.float32)).double()
        want = float(torch.linalg.vector_norm(x))
        assert abs(R.grad_norm64(g, scale) - want) <= 1e-12 * want
        assert abs(R.grad_norm32(g, scale) - want) <= 4 * R.FLOOR * want * max(1.0, math.log2(n + 1))
        assert R.norm_bound(g, scale) <= 1e-5          # float32 accumulation over n terms: a bound that still bounds


def test_wide_norm_cases_defeat_float32_accumulation():
    """NORM_WIDE is what it claims: squares summed in float32 overflow ("wide") or vanish ("tiny"), the float64 norm is an
    ordinary float32 number, and the twin (scaled by a power of two) still measures a rounding error"""
    for name, (n, lo, hi) in R.NORM_WIDE.items():
        g = R.norm_case(name, n, lo, hi)
        naive = float((g * g).sum().sqrt())
        want = R.grad_norm64(g, 1.0)
        assert (math.isinf(naive) if name == "wide" else naive == 0.0), (name, naive)
        assert 1e-30 < want < 1e30
        assert abs(R.grad_norm32(g, 1.0) - want) <= 1e-5 * want
        assert R.norm_bound(g, 1.0) <= 1e-5
    g = R.norm_case("wide", *R.NORM_WIDE["wide"])
    assert float(g.abs().min()) < 1e-24 and float(g.abs().max()) > 1e17


def test_ema_step32_is_the_float32_expression():
    p, e = torch.randn(1027), torch.randn(1027)
    want = 0.999 * e.double() + (1 - 0.999) * p.double()
    assert R.rel(R.ema_step32(e, p, 0.999), want) <= 4 * R.FLOOR
