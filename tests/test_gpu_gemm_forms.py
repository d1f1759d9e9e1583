"""GPU: every dispatched form of erc_gemm_f32_stream and erc_gemm_bf16a_stream (csrc/gemm_stream.hip) on exact products.

The cases, their operands and the float64 expectations are those of tests/gemm_forms_ref.py (read its header first): integer
operands whose products are exact in fp32 in any summation order, so a result is compared with torch.equal, never through a
tolerance; NaN wherever a call has no business reading or writing, so a stray access shows without faulting; and before every
launch the form query, on the real device pointers, has to report the form the table claims -- tests/test_gemm_forms_ref.py
holds the table to the complete list of forms.  The real-valued cases are held to the derived bound of the header and print
the fraction of it they reach."""
import pytest
import torch

from tests import gemm_forms_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def capi():
    from erc_amd import capi as c
    c.lib()
    return c


def _upload(o):
    dev = {k: v.to(DEV) for k, v in o.items() if isinstance(v, torch.Tensor) and not k.endswith("64") and k != "C_old"}
    return dev, (lambda name: dev[name].data_ptr())


def run_f32(capi, c):
    o = R.f32_operands(c)
    dev, addr = _upload(o)
    args = R.f32_args(c, o, addr)
    assert capi.gemm_f32_stream_form(*args) == R.f32_form(c), c
    capi.gemm_f32_stream(*args)
    return R.f32_check(c, o, dev["C"].cpu(), dev["bias_out"].cpu() if c["ones"] else None)


def run_bf(capi, c, o=None):
    o = R.bf_operands(c) if o is None else o
    dev, addr = _upload(o)
    X, ldx, idx, W, ldw, Cm, ldc, M, N, K, bias, act, wb = R.bf_args(c, o, addr)
    assert capi.gemm_bf16a_stream_form(X, ldx, idx, W, ldw, Cm, ldc, M, N, K, bias, act, wb) == R.bf_form(c), c
    capi._call("erc_gemm_bf16a_stream", X, ldx, idx, W, ldw, wb, Cm, ldc, M, N, K, bias, act)
    return R.bf_check(c, o, dev["C"].cpu())


# =============================================================================================== erc_gemm_f32_stream
def test_f32_every_form_once(capi):
    """all 43 instantiations at tile-edge sizes, gather indices out of order and repeating"""
    cases = R.f32_every_form()
    assert {R.f32_form(c) for c in cases} == R.F32_FORMS
    for c in cases:
        run_f32(capi, c)


@pytest.mark.parametrize("layout", R.SWEEP_LAYOUTS)
def test_f32_every_k(capi, layout):
    """every K of 1 .. 1100 at M = 17, N = 33: every per-wavefront remainder, the partial block on every wavefront, no partial
    block.  The operands are the leading K of one integer block at a fixed pitch; what lies past K is NaN at the time of the
    launch (the block is filled in one k per launch)."""
    a_k, b_k = R.LAYOUT[layout]
    M, N, Kmax, LD = R.SWEEP_M, R.SWEEP_N, R.SWEEP_K, R.SWEEP_LD
    A, B = R.f32_sweep_blocks()
    exp = R.prefix_products(A, B)
    # stored forms: K-contiguous [rows + 2, LD] (k along a row), K-major [Kmax + 2, rows + 3] (k down a column)
    srcA, srcB = (A.t() if a_k else A).contiguous().to(DEV), (B if b_k else B.t()).contiguous().to(DEV)
    wA = torch.full((Kmax + 2, M + 3) if a_k else (M + 2, LD), R.NAN, device=DEV)
    wB = torch.full((Kmax + 2, N + 3) if b_k else (N + 2, LD), R.NAN, device=DEV)
    lda, ldb = wA.shape[1], wB.shape[1]
    out = torch.full((Kmax, M + 2, N + 3), R.NAN, device=DEV)
    for K in range(1, Kmax + 1):
        if a_k:
            wA[K - 1, :M] = srcA[K - 1]
        else:
            wA[:M, K - 1] = srcA[:, K - 1]
        if b_k:
            wB[K - 1, :N] = srcB[K - 1]
        else:
            wB[:N, K - 1] = srcB[:, K - 1]
        args = (wA.data_ptr(), lda, a_k, None, wB.data_ptr(), ldb, b_k, None, out[K - 1].data_ptr(), N + 3, M, N, K)
        assert capi.gemm_f32_stream_form(*args) == R.f32_form(R.f32_sweep_case(layout, K)), K
        capi.gemm_f32_stream(*args)
    got = out.cpu()
    for K in range(1, Kmax + 1):      # per K, so that a failure names it
        R.check_written(got[K - 1], exp[K - 1], "f32 %s K=%d" % (layout, K))


def test_f32_other_forms_at_five_k_per_nw(capi):
    cases = R.f32_other_k()
    assert len(cases) == 33 * 5
    for c in cases:
        run_f32(capi, c)


@pytest.mark.parametrize("nw", [1, 4, 8])
@pytest.mark.parametrize("layout", list(R.LAYOUT))
def test_f32_tile_edges(capi, layout, nw):
    """M and N on, below and above every tile boundary, with and without the virtual ones column / row (which opens a tile of
    its own at N % 32 == 0 resp. M % 16 == 0)"""
    for c in R.f32_tile_edges(layout, nw):
        run_f32(capi, c)


def test_f32_split_k(capi):
    """every slab and bias slab is written in full (an empty last piece writes zeros) and equals its K range's exact product,
    so their sum is exact too"""
    cases = R.f32_split_cases()
    assert {R.f32_form(c)[2] for c in cases if R.has_empty_last_split(c)} == {1, 4, 8}
    for c in cases:
        run_f32(capi, c)


def test_f32_epilogues(capi):
    """bias, act 1 / 2 / 3 and accumulate, alone and combined, in every layout at every wavefront count.  act 3 alone runs on
    positive operands, so its non-zero set IS the keep mask; the mask is the restated erc_uniform >= drop_p on row N + col."""
    for c in R.f32_epilogue_cases():
        run_f32(capi, c)
        if c["act"] == 3 and c["positive"]:
            o = R.f32_operands(c)
            exp, _, _ = R.f32_expected(c, o)
            assert torch.equal(exp[0] != 0, R.keep_mask(c["M"], c["N"])) and 0.4 < float((exp[0] != 0).double().mean()) < 0.6


@pytest.mark.parametrize("i", range(5))
def test_f32_big_tile(capi, i):
    c = R.f32_big_cases()[i]
    assert R.f32_form(c) == (0, 0, 4, 0, 0, 1, 2, 4)
    run_f32(capi, c)


def test_f32_real_valued_within_the_derived_bound(capi):
    """randn operands, bias and accumulate, once per form: |got - ref64| <= (K + NW + 3) 2^-23 (|A| |B| + |bias| + |C_old|)"""
    for c in R.f32_every_form(real=True):
        frac = run_f32(capi, c)
        print("f32 form %s K=%d: %.2e of the bound" % (R.f32_form(c), c["K"], frac))


# ============================================================================================= erc_gemm_bf16a_stream
def test_bf16a_streaming_every_access_width(capi):
    """every (nw, W type, a_vec, b_vec): widths from the pitch (ld % 8, % 4, % 2, odd) and from a pointer one element off"""
    cases = R.bf_streaming_cases()
    assert {R.bf_form(c) for c in cases} == R.BF_FORMS - {(1, 8, 1, 6, 1, 1)}
    for c in cases:
        run_bf(capi, c)


@pytest.mark.parametrize("wb", [True, False])
def test_bf16a_every_k(capi, wb):
    """every K of 1 .. 600 at M = 33, N = 17; what lies past K is NaN at the time of the launch"""
    M, N, Kmax, LD = R.BF_SWEEP_M, R.BF_SWEEP_N, R.BF_SWEEP_K, R.BF_SWEEP_LD
    X, W = R.bf_sweep_blocks()
    exp = R.prefix_products(X, W.t())
    wdt = torch.bfloat16 if wb else torch.float32
    srcX, srcW = X.bfloat16().to(DEV), W.to(wdt).to(DEV)
    wX = torch.full((M + 2, LD), R.NAN, dtype=torch.bfloat16, device=DEV)
    wW = torch.full((N + 2, LD), R.NAN, dtype=wdt, device=DEV)
    out = torch.full((Kmax, M + 2, N + 3), R.NAN, device=DEV)
    for K in range(1, Kmax + 1):
        wX[:M, K - 1] = srcX[:, K - 1]
        wW[:N, K - 1] = srcW[:, K - 1]
        args = (wX.data_ptr(), LD, None, wW.data_ptr(), LD, out[K - 1].data_ptr(), N + 3, M, N, K)
        assert capi.gemm_bf16a_stream_form(*args, w_is_bf16=wb) == (0, R.bf_nw(K), int(wb), 6, 2, 2 if wb else 1), K
        capi._call("erc_gemm_bf16a_stream", *args[:5], int(wb), *args[5:], None, 0)
    got = out.cpu()
    for K in range(1, Kmax + 1):
        R.check_written(got[K - 1], exp[K - 1], "bf16a wb=%d K=%d" % (wb, K))


def test_bf16a_gather_bias_relu(capi):
    for c in R.bf_gather_cases():
        run_bf(capi, c)


@pytest.mark.parametrize("M", R.PERSIST_M)
def test_bf16a_persistent_kernel(capi, M):
    """the register-resident kernel: K with and without a shifted last block (K % 32), N through both column halves up to 128"""
    cases = R.bf_persist_cases(M)
    assert len(cases) == len(R.PERSIST_N) * len(R.PERSIST_K) and {R.bf_form(c) for c in cases} == {(1, 8, 1, 6, 1, 1)}
    for c in cases:
        run_bf(capi, c)


def test_bf16a_just_past_the_persistent_limits(capi):
    """K = 1540 and N = 129 at M = 1024 report the streaming kernel and are exact"""
    for c in R.bf_beyond_persist_cases():
        assert R.bf_form(c)[0] == 0
        run_bf(capi, c)


@pytest.mark.parametrize("b_sel", R.B_SEL[False])
def test_bf16a_fp32_weights_round_to_nearest_even(capi, b_sel):
    """W on and one fp32 ulp beside the bf16 rounding boundaries: a truncating or round-half-up conversion changes sums that
    are exact in fp32 (tests/test_gemm_forms_ref.py shows both do)"""
    c, o = R.rounding_case(b_sel)
    run_bf(capi, c, o)


def test_bf16a_real_valued_within_the_derived_bound(capi):
    for c in R.bf_streaming_cases(real=True) + [R.bf_persist_real_case()]:
        frac = run_bf(capi, c)
        print("bf16a form %s K=%d: %.2e of the bound" % (R.bf_form(c), c["K"], frac))
