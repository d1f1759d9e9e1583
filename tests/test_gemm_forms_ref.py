"""CPU: the case table of tests/gemm_forms_ref.py.  (1) Every integer case is exact in fp32 in any summation order; (2) the
forms the table reaches, as erc_gemm_f32_stream_form / erc_gemm_bf16a_stream_form report them, are exactly the literal lists
below -- a dispatch threshold that moves makes this fail instead of shrinking what the GPU tests cover; (3) no override of the
dispatch is set.  The queries run on stand-in addresses: they dereference nothing."""
import os

import numpy as np
import pytest
import torch

from tests import gemm_forms_ref as R

LIMIT = float(2 ** 24)


@pytest.fixture(scope="module")
def capi():
    from erc_amd import capi as c
    c.build()
    c.lib()
    return c


def test_no_dispatch_override_is_set():
    assert "ERC_GEMM_BIG_TILE" not in os.environ and "ERC_PERSIST_MIN_M" not in os.environ


# ------------------------------------------------------------------------------------------------ (1) integer bound
def _exact_in_fp32(A64, B64, mag, what):
    assert float(mag.max()) < LIMIT, what
    assert torch.equal((A64.float() @ B64.float()).double(), A64 @ B64), what


def test_f32_integer_cases_are_exact_in_any_order():
    cases = R.f32_integer_cases()
    assert len(cases) > 2000
    for c in cases:
        o = R.f32_operands(c)
        for t in (o["A64"], o["B64"], o["bias64"], o["C_old"]):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3, c
        exp, exp_bo, mag = R.f32_expected(c, o)
        _exact_in_fp32(o["A64"], o["B64"], mag, c)
        assert torch.equal(exp, exp.round()) and float(exp.abs().max()) < LIMIT, c


def test_sweep_blocks_are_exact_in_any_order():
    for (A, B) in (R.f32_sweep_blocks(), tuple(t.t() if i else t for i, t in enumerate(R.bf_sweep_blocks()))):
        assert float(A.abs().max()) <= 3 and float(B.abs().max()) <= 3 and torch.equal(A, A.round()) and torch.equal(B, B.round())
        assert float((A.abs().double() @ B.abs().double()).max()) < LIMIT
        assert torch.equal(R.prefix_products(A, B, torch.float32).double(), R.prefix_products(A, B))
        assert torch.equal(A.bfloat16().float(), A) and torch.equal(B.bfloat16().float(), B)


def test_bf16a_integer_cases_are_exact_in_any_order():
    for c in R.bf_integer_cases():
        o = R.bf_operands(c)
        for t in (o["X64"], o["W64"], o["bias64"]):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3, c
        exp, mag = R.bf_expected(c, o)
        _exact_in_fp32(o["X64"], o["W64"].t(), mag, c)


def test_rounding_weights_sit_on_the_boundaries():
    W, cls, kinds = R.rounding_weights()
    bits = torch.from_numpy(W.numpy().view(np.uint32).astype(np.int64))
    up = (W.bfloat16().float().abs() > W.abs())             # torch rounds to nearest even
    assert bool(((W.abs() >= 1) & (W.abs() < 2)).all())
    for i, kind in enumerate(kinds):
        sel = cls == i
        assert int(sel.sum()) >= 200
        lsb, low = R.ROUND_LOW16[kind]
        assert bool(((bits[sel] & 0xFFFF) == low).all())
        want_up = {"tie, even below": False, "tie, even above": True, "one ulp below a tie": False, "one ulp above a tie": True}[kind]
        assert bool((up[sel] == want_up).all()), kind
    # a truncating conversion differs on the "up" classes, round-half-up on "tie, even below": both change the expectation
    c, o = R.rounding_case(1)
    trunc = torch.from_numpy((bits & 0xFFFF0000).numpy().astype(np.uint32).view(np.float32).copy()).double()
    half_up = torch.from_numpy(((bits + 0x8000) & 0xFFFF0000).numpy().astype(np.uint32).view(np.float32).copy()).double()
    exp = o["X64"] @ o["W64"].t()
    assert not torch.equal(o["X64"] @ trunc.t(), exp) and not torch.equal(o["X64"] @ half_up.t(), exp)
    assert torch.equal((o["X64"].float() @ o["W64"].float().t()).double(), exp)
    assert float((exp * 128).abs().max()) < 2 ** 15 and torch.equal(exp * 128, (exp * 128).round())


def test_checker_notices_one_wrong_element_and_one_stray_write():
    c = R.f32_every_form()[0]
    o = R.f32_operands(c)
    exp, _, _ = R.f32_expected(c, o)
    got = o["C"].clone()
    got[:, :c["M"], :c["N"]] = exp.float()
    R.f32_check(c, o, got, None)
    bad = got.clone()
    bad[0, 3, 5] += 1
    with pytest.raises(AssertionError, match="wrong elements"):
        R.f32_check(c, o, bad, None)
    bad = got.clone()
    bad[0, c["M"], 0] = 0.0
    with pytest.raises(AssertionError, match="outside"):
        R.f32_check(c, o, bad, None)
    bad = got.clone()
    bad[0, 0, 0] = R.NAN
    with pytest.raises(AssertionError, match="NaN in the result"):
        R.f32_check(c, o, bad, None)


# ------------------------------------------------------------------------------------------------- (2) form coverage
def test_f32_table_reaches_exactly_the_43_forms(capi):
    literal = set()
    for nw in (1, 4, 8):
        literal |= {(0, 0, nw, 0, 0, 1, 1, 2), (0, 0, nw, 0, 0, 0, 1, 2), (0, 0, nw, 1, 0, 1, 1, 2), (0, 0, nw, 1, 0, 0, 1, 2)}   # NT
        literal |= {(0, 1, nw, 0, 0, 1, 1, 2), (0, 1, nw, 0, 0, 0, 1, 2), (0, 1, nw, 1, 0, 1, 1, 2), (0, 1, nw, 1, 0, 0, 1, 2),   # NN
                    (0, 1, nw, 0, 1, 1, 1, 2), (0, 1, nw, 0, 1, 0, 1, 2), (0, 1, nw, 1, 1, 1, 1, 2), (0, 1, nw, 1, 1, 0, 1, 2)}
        literal |= {(1, 1, nw, 0, 0, 0, 1, 2), (1, 1, nw, 0, 1, 0, 1, 2)}                                                       # TN
    literal.add((0, 0, 4, 0, 0, 1, 2, 4))                                                                                   # big tile
    assert len(literal) == 43 and literal == set(R.F32_FORMS)

    def reached(cases):
        out = set()
        for c in cases:
            o = R.f32_operands(c)
            form = capi.gemm_f32_stream_form(*R.f32_args(c, o, R.host_addr(o)))
            assert form == R.f32_form(c), (c, form)
            out.add(form)
        return out
    assert reached(R.f32_every_form()) == literal
    assert reached(R.f32_every_form(real=True)) == literal
    assert reached(R.f32_integer_cases()) == literal
    # the K sweep: every K of 1 .. 1100 in the three ungathered layouts, at a fixed pitch
    for layout in R.SWEEP_LAYOUTS:
        a_k, b_k = R.LAYOUT[layout]
        nws = []
        for K in range(1, R.SWEEP_K + 1):
            lda, ldb = (R.SWEEP_M + 3 if a_k else R.SWEEP_LD), (R.SWEEP_N + 3 if b_k else R.SWEEP_LD)
            form = capi.gemm_f32_stream_form(R.BASE, lda, a_k, None, 2 * R.BASE, ldb, b_k, None, 3 * R.BASE, R.SWEEP_N + 3, R.SWEEP_M,
                                             R.SWEEP_N, K)
            assert form == R.f32_form(R.f32_sweep_case(layout, K)) == (a_k, b_k, form[2], 0, 0, int(layout != "TN"), 1, 2)
            nws.append(form[2])
        assert nws == [1] * 80 + [4] * 416 + [8] * 604
    # the big tile starts exactly where the table says it does
    assert {R.f32_form(c) for c in R.f32_big_cases()} == {(0, 0, 4, 0, 0, 1, 2, 4)}
    for c in (R.f32case("NT", 2047, 64, 4096), R.f32case("NT", 2048, 63, 4096), R.f32case("NT", 2048, 64, 4095)):
        o = R.f32_operands(c)
        assert capi.gemm_f32_stream_form(*R.f32_args(c, o, R.host_addr(o))) == R.f32_form(c) == (0, 0, 8, 0, 0, 1, 1, 2)


def test_f32_table_has_the_edges_it_claims():
    every = R.f32_every_form()
    assert {c["M"] % 16 for c in every} == {1, 15} and {c["N"] % 32 for c in every} == {1, 17, 31}
    for c in every:
        o = R.f32_operands(c)
        for name, n in (("ia", c["M"]), ("ib", c["K"])):
            if o[name] is not None:
                idx = o[name][:n].long()
                assert len(set(idx.tolist())) < n and not bool((idx[1:] >= idx[:-1]).all()), c
    splits = R.f32_split_cases()
    assert {2, 3, 5} <= {c["split"] for c in splits}
    assert {R.f32_form(c)[2] for c in splits if R.has_empty_last_split(c)} == {1, 4, 8}
    assert {c["layout"] for c in splits if R.has_empty_last_split(c)} == set(R.LAYOUT)
    for nw in (1, 4, 8):
        assert {K % 16 for K in R.OTHER_K[nw]} >= {0, 1, 15} and {R.f32_nw(K) for K in R.OTHER_K[nw]} == {nw}
        assert R.f32_nw(R.K_OF_NW[nw]) == nw and R.bf_nw(R.BF_K_OF_NW[nw]) == nw
    edges = R.f32_tile_edges("NT", 4)
    assert any(c["ones"] == 1 and c["N"] % 32 == 0 for c in edges) and any(c["ones"] == 2 and c["M"] % 16 == 0 for c in edges)
    # per-wavefront remainders 0 .. 3 and the partial block on every wavefront, at every wavefront count of the sweep
    for nw, Ks in ((1, range(1, 81)), (4, range(81, 497)), (8, range(497, 1101))):
        rems, tails = set(), set()
        for K in Ks:
            full = K // 16
            for w in range(nw):
                mine = len(range(w, full, nw))
                rems.add(mine % 4)        # what the batched main loop (4 blocks a turn) leaves
            if K % 16:
                tails.add(full % nw)
        assert rems == {0, 1, 2, 3} and tails == set(range(nw)), (nw, rems, tails)


def test_bf16a_table_reaches_exactly_its_forms(capi):
    literal = {(1, 8, 1, 6, 1, 1)}                                                     # the persistent kernel
    for nw in (1, 4, 8):
        for a_vec in (2, 1, 4, 0):
            literal |= {(0, nw, 1, 6, a_vec, 2), (0, nw, 1, 6, a_vec, 1), (0, nw, 1, 6, a_vec, 4), (0, nw, 1, 6, a_vec, 0)}   # bf16 W
            literal |= {(0, nw, 0, 6, a_vec, 1), (0, nw, 0, 6, a_vec, 3), (0, nw, 0, 6, a_vec, 0)}                           # fp32 W
    assert len(literal) == 85 and literal == set(R.BF_FORMS)
    reached = set()
    for c in R.bf_integer_cases() + R.bf_streaming_cases(real=True) + [R.bf_persist_real_case()] + [R.rounding_case(b)[0] for b in R.B_SEL[False]]:
        o = R.bf_operands(c)
        form = capi.gemm_bf16a_stream_form(*R.bf_args(c, o, R.host_addr(o)))
        assert form == R.bf_form(c), (c, form)
        reached.add(form)
    assert reached == literal
    for M in R.PERSIST_M:
        assert {R.bf_form(c) for c in R.bf_persist_cases(M)} == {(1, 8, 1, 6, 1, 1)}
    assert {R.bf_form(c) for c in R.bf_beyond_persist_cases()} == {(0, 8, 1, 6, 2, 2)}
    assert R.bf_form(R.bfcase(1023, 100, 1380, True)) == (0, 8, 1, 6, 2, 2)
    # the sweep: every K of 1 .. 600 at a fixed pitch, both W types
    for wb in (True, False):
        nws = [capi.gemm_bf16a_stream_form(R.BASE, R.BF_SWEEP_LD, None, 2 * R.BASE, R.BF_SWEEP_LD, 3 * R.BASE, R.BF_SWEEP_N + 3,
                                           R.BF_SWEEP_M, R.BF_SWEEP_N, K, w_is_bf16=wb) for K in range(1, R.BF_SWEEP_K + 1)]
        assert nws == [(0, R.bf_nw(K), int(wb), 6, 2, 2 if wb else 1) for K in range(1, R.BF_SWEEP_K + 1)]
        assert [f[1] for f in nws] == [1] * 96 + [4] * 384 + [8] * 120


def test_form_queries_run_the_launchers_argument_checks(capi):
    with pytest.raises(capi.ErcGraftError, match="not built"):
        capi.gemm_f32_stream_form(R.BASE, 8, 1, None, R.BASE, 8, 0, None, R.BASE, 8, 4, 4, 4)
    with pytest.raises(capi.ErcGraftError, match="exceeds"):
        capi.gemm_f32_stream_form(R.BASE, 8, 0, None, R.BASE, 8, 0, None, R.BASE, 8, 4, 4, 4, split_k=2)
    with pytest.raises(capi.ErcGraftError, match="act 2"):
        capi.gemm_bf16a_stream_form(R.BASE, 8, None, R.BASE, 8, R.BASE, 8, 4, 4, 4, act=2, w_is_bf16=True)
