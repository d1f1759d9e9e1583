"""Host tests of tests/encoder_kernels_ref.py: no GPU.

(1) The float64 restatements are tied to known references: torch.nn.functional.multi_head_attention_forward on identity
    projections (rounding switched off), float64 autograd of the forward restatement, torch.nn.functional.layer_norm.
(2) The bounds the GPU tests use have teeth: six known mutations (a dropped last key, the keys of sequence 0 read for
    sequence 1, a head shifted by one column, the last 4 of K dropped in the GEMM, the last column of a LayerNorm row
    skipped, rowsum(dP) for rowsum(P dP)) each violate their bound on the GPU tests' own inputs.
(3) The recorded float32 figures (what fp32 arithmetic alone uses of each bound; the GPU tests allow 4 x them) are
    re-measured from the float32 restatements and must reproduce."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import encoder_kernels_ref as R

TIE = 1e-12


def _inputs(B, T, D, seed, masked):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * T, 3 * D, generator=g) * 0.7).to(torch.bfloat16)
    dout = torch.randn(B * T, D, generator=g).to(torch.bfloat16)
    lengths = None
    if masked:
        lengths = torch.randint(1, T, (B,), generator=g, dtype=torch.int64)
        lengths[0] = T
    return qkv, dout, lengths


def _mha(qkv, B, T, D, heads, lengths):
    """torch's multi-head attention in float64 with identity projections: what is left is the attention itself"""
    q, k, v = (qkv.double()[:, i * D:(i + 1) * D].reshape(B, T, D).transpose(0, 1) for i in range(3))
    eye = torch.eye(D, dtype=torch.float64)
    pad = None if lengths is None else torch.arange(T)[None, :] >= lengths[:, None]
    out, _ = F.multi_head_attention_forward(
        q, k, v, D, heads, in_proj_weight=None, in_proj_bias=None, bias_k=None, bias_v=None, add_zero_attn=False, dropout_p=0.0,
        out_proj_weight=eye, out_proj_bias=torch.zeros(D, dtype=torch.float64), training=False, key_padding_mask=pad,
        need_weights=False, use_separate_proj_weight=True, q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye)
    return out.transpose(0, 1).reshape(B * T, D)


# ------------------------------------------------------------------------------------------------ (1) reference ties
@pytest.mark.parametrize("B,T,D,heads", [(2, 13, 24, 6), (2, 17, 712, 8)])
def test_attention_restatements_match_torch_mha(B, T, D, heads):
    qkv, _, lengths = _inputs(B, T, D, T + D, True)
    want = _mha(qkv, B, T, D, heads, None)
    assert float((R.attention(qkv, B, T, D, heads)[0] - want).abs().max()) <= TIE
    assert float((R.attention_train(qkv, B, T, D, heads, None, None, R.identity)[0] - want).abs().max()) <= TIE
    assert int(lengths.min()) < T
    want = _mha(qkv, B, T, D, heads, lengths)
    assert float((R.attention_train(qkv, B, T, D, heads, lengths, None, R.identity)[0] - want).abs().max()) <= TIE


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("B,T,D,heads", [(2, 13, 24, 6), (2, 17, 712, 8)])
def test_attention_backward_restatement_matches_autograd(B, T, D, heads, p, masked):
    qkv, dout, lengths = _inputs(B, T, D, T + D + 1, masked)
    keep = R.keep_mask((B, heads, T, T), p, R.RNG[1], R.RNG[0], R.ATTN_STREAM) if p > 0 else None
    x = qkv.double().requires_grad_(True)
    out, _ = R.attention_train(x, B, T, D, heads, lengths, keep, R.identity)
    out.backward(dout.double())
    got, _ = R.attention_train_bwd(qkv, dout, B, T, D, heads, lengths, keep, R.identity)
    assert float((got - x.grad).abs().max()) <= TIE
    if masked:          # keys behind the mask: exactly no gradient
        L = int(lengths[1])
        assert L < T and float(got[T + L:2 * T, D:].abs().max()) == 0.0


def test_rounding_is_applied_where_the_kernels_round():
    """with r in place, Pd and dS are bf16 values: the products' left operands survive a bf16 round trip unchanged"""
    c = R.attn_train_case(2, 17, 24, 6, 0.5, True)
    q, k, v = R._qkv(c["qkv"], 2, 17, 24, 6)
    Pd = R.r(R._probabilities(q, k, c["lengths"]) * c["keep"].double())
    assert torch.equal(R.r(Pd), Pd)
    assert float((R._rows(Pd @ v) - c["out"]).abs().max()) == 0.0
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=torch.float64)
    assert R.r(x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]                # ties to even, above a tie up
    assert R._bf16_np(x.float().numpy()).tolist() == R.r(x).tolist()


@pytest.mark.parametrize("rows,D", R.LN_CASES)
def test_add_layernorm_restatement_matches_torch(rows, D):
    c = R.ln_case(rows, D)
    want = F.layer_norm(c["a"].double() + c["b"].double(), (D,), c["gamma"].double(), c["beta"].double(), R.LN_EPS)
    assert float((c["ref"] - want).abs().max()) <= TIE


def test_gemm_restatement():
    g = torch.Generator().manual_seed(3)
    a, w, bias = torch.randn(5, 12, generator=g), torch.randn(3, 12, generator=g), torch.randn(3, generator=g)
    y, absdot = R.gemm(a, w, bias, relu=True)
    assert float((y - F.relu(F.linear(a.double(), w.double(), bias.double()))).abs().max()) <= TIE
    assert float((absdot - torch.einsum("mk,nk->mn", a.double().abs(), w.double().abs())).abs().max()) <= TIE


# --------------------------------------------------------------------------------------------- (2) the bounds have teeth
def _violates(got, ref, bound):
    return bool(((got - ref).abs() > bound).any())


def _lengths_without_last_key(c, B, T, seq):
    lengths = torch.full((B,), T, dtype=torch.int64) if c.get("lengths") is None else c["lengths"].clone()
    lengths[seq] -= 1
    return lengths


def _keys_of_sequence_0(qkv, T, D):
    m = qkv.clone()
    m[T:2 * T, D:2 * D] = qkv[:T, D:2 * D]
    return m


def _head_shifted(qkv, D, hd, head):
    """head `head` of q, k and v read one column late"""
    m = qkv.clone()
    for blk in range(3):
        c0 = blk * D + head * hd
        m[:, c0:c0 + hd] = torch.roll(qkv[:, c0:c0 + hd + 1] if c0 + hd < 3 * D else qkv[:, c0:c0 + hd], -1, 1)[:, :hd]
    return m


INFER_MUTATION_CASES = [n for n, c in R.ATTN_CASES.items() if c[0] > 1 and c[1] > 1]


@pytest.mark.parametrize("name", INFER_MUTATION_CASES)
def test_inference_attention_bound_rejects_mutations(name):
    c = R.attn_case(name)
    n_seq, S, D, heads = c["n_seq"], c["S"], c["D"], c["heads"]
    assert not _violates(R.f32_restatement_attention(c["qkv"], n_seq, S, D, heads).double(), c["ref"], c["bound"])
    # the last key of sequence 1 dropped
    got = R.attention_train(c["qkv"], n_seq, S, D, heads, _lengths_without_last_key({}, n_seq, S, 1), None, R.identity)[0]
    assert _violates(got, c["ref"], c["bound"]) and not _violates(got[:S], c["ref"][:S], c["bound"][:S])
    # sequence 1 reads the keys of sequence 0
    got = R.attention(_keys_of_sequence_0(c["qkv"], S, D), n_seq, S, D, heads)[0]
    assert _violates(got[S:2 * S], c["ref"][S:2 * S], c["bound"][S:2 * S])
    # the last head shifted by one column
    hd = D // heads
    got = R.attention(_head_shifted(c["qkv"], D, hd, heads - 1), n_seq, S, D, heads)[0]
    assert _violates(got[:, D - hd:], c["ref"][:, D - hd:], c["bound"][:, D - hd:])
    assert not _violates(got[:, :D - hd], c["ref"][:, :D - hd], c["bound"][:, :D - hd])


def _bwd_rowsum_of_dp(c):
    """attention_train_bwd with the softmax backward's row sum taken over dP instead of P dP"""
    B, T, D, heads = c["B"], c["T"], c["D"], c["heads"]
    q, k, v = R._qkv(c["qkv"], B, T, D, heads)
    do = R._heads(c["dout"].double(), B, T, heads)
    P = R._probabilities(q, k, c["lengths"])
    kp = 1.0 if c["keep"] is None else c["keep"].double()
    dP = (do @ v.transpose(-1, -2)) * kp
    dS = R.r(P * (dP - dP.sum(-1, keepdim=True)) / math.sqrt(D // heads))
    return torch.cat([R._rows(dS @ k), R._rows(dS.transpose(-1, -2) @ q)], 1)


TRAIN_MUTATION_CASES = [c for c in R.ATTN_TRAIN_CASES if c[0] > 1 and c[1] > 1]


@pytest.mark.parametrize("B,T,D,heads,p,masked", TRAIN_MUTATION_CASES)
def test_training_attention_bounds_reject_mutations(B, T, D, heads, p, masked):
    c = R.attn_train_case(B, T, D, heads, p, masked)
    rec = R.F32_SHARE[(B, T, D, heads, p, masked)]
    parts = [slice(0, D), slice(D, 2 * D), slice(2 * D, 3 * D)]

    def run(qkv, lengths):
        out = R.attention_train(qkv, B, T, D, heads, lengths, c["keep"])[0]
        return out, R.attention_train_bwd(qkv, c["dout"], B, T, D, heads, lengths, c["keep"])[0]

    def violated(out, grads):
        return [_violates(out, c["out"], c["out_bound"])] + [_violates(grads[:, s], c["grads"][:, s], c["grads_bound"][:, s])
                                                             for s in parts]
    assert violated(c["out"], c["grads"]) == [False] * 4
    # the last key of sequence 0 (full length) dropped: out, dQ, dK and dV all leave their element-wise bound, and the
    # mean tier as well wherever the damage is not confined to a few elements
    out, grads = run(c["qkv"], _lengths_without_last_key(c, B, T, 0))
    assert violated(out, grads) == [True] * 4
    assert R.share((out - c["out"]).abs(), c["out_bound"]) > R.SHARE_FACTOR * rec[0]
    # sequence 1 reads the keys of sequence 0
    out, grads = run(_keys_of_sequence_0(c["qkv"], T, D), c["lengths"])
    assert violated(out, grads) == [True] * 4
    # the last head one column late
    out, grads = run(_head_shifted(c["qkv"], D, D // heads, heads - 1), c["lengths"])
    assert violated(out, grads) == [True] * 4
    # rowsum(dP) in the softmax backward: dQ and dK
    m = _bwd_rowsum_of_dp(c)
    assert _violates(m[:, :D], c["grads"][:, :D], c["grads_bound"][:, :D])
    assert _violates(m[:, D:], c["grads"][:, D:2 * D], c["grads_bound"][:, D:2 * D])
    for i, s in enumerate(parts[:2]):
        assert R.share((m[:, i * D:(i + 1) * D] - c["grads"][:, s]).abs(), c["grads_bound"][:, s]) > R.SHARE_FACTOR * rec[1 + i]


@pytest.mark.parametrize("M,N,K", [(5, 3, 12), (129, 127, 68), (70, 712, 1380), (40, 24, 2048)])
def test_gemm_bounds_reject_a_dropped_k_tail(M, N, K):
    g = torch.Generator().manual_seed(K)
    # integer operands: exact means equal, and losing 4 of K products does not stay equal
    a = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16)
    w = torch.randint(-3, 4, (N, K), generator=g).to(torch.bfloat16)
    ref, absdot = R.gemm(a, w)
    assert float(absdot.max()) + 3 < 2 ** 24                         # every partial sum is an fp32-exact integer
    assert torch.equal(ref.float().double(), ref)
    assert not torch.equal(R.gemm(a[:, :K - 4], w[:, :K - 4])[0], ref)
    # random operands: the forward bound K 2^-24 absdot holds for a float32 product and not without the tail
    a, w = torch.randn(M, K, generator=g).to(torch.bfloat16), torch.randn(N, K, generator=g).to(torch.bfloat16)
    ref, absdot = R.gemm(a, w)
    bound = R.gemm_bound(K, absdot)
    assert not _violates((a.float() @ w.float().t()).double(), ref, bound)
    cut = R.gemm(a[:, :K - 4], w[:, :K - 4])[0]
    assert _violates(cut, ref, bound) and _violates(cut, ref, bound + 2.0 ** -8 * ref.abs())


@pytest.mark.parametrize("rows,D,offset", [c + (0.0,) for c in R.LN_CASES if c[1] > 1] + [R.LN_OFFSET_CASE + (100.0,)])
def test_layernorm_bounds_reject_a_skipped_column(rows, D, offset):
    c = R.ln_case(rows, D, offset)
    tol = R.SHARE_FACTOR * R.LN_OFFSET_F32_ERR if offset else 1e-4
    x = c["a"].double() + c["b"].double()
    mean = x[:, :-1].mean(-1, keepdim=True)
    var = ((x[:, :-1] - mean) ** 2).mean(-1, keepdim=True)
    got = (x - mean) / (var + R.LN_EPS).sqrt() * c["gamma"].double() + c["beta"].double()
    assert float((got - c["ref"]).abs().max()) > tol
    assert R.ln_f32_err(c) < tol


def test_offset_layernorm_tolerance_separates_one_pass_variance():
    c = R.ln_case(*R.LN_OFFSET_CASE, 100.0)
    x = c["a"] + c["b"]
    assert abs(float(x.mean()) - 100.0) < 0.1 and abs(float(x.std()) - 1.0) < 0.1
    mean = x.mean(-1, keepdim=True)
    var = (x * x).mean(-1, keepdim=True) - mean * mean                # float32, one pass
    got = (x - mean) / (var + R.LN_EPS).sqrt() * c["gamma"] + c["beta"]
    assert float((got.double() - c["ref"]).abs().max()) > R.SHARE_FACTOR * R.LN_OFFSET_F32_ERR


# ------------------------------------------------------------------------------------- (3) the recorded float32 figures
def _reproduces(got, recorded):
    return got == recorded if recorded == 0 else abs(got - recorded) <= 0.1 * recorded


@pytest.mark.parametrize("B,T,D,heads,p,masked", R.ATTN_TRAIN_CASES)
def test_recorded_training_attention_shares(B, T, D, heads, p, masked):
    got = R.attn_train_f32_share(R.attn_train_case(B, T, D, heads, p, masked))
    rec = R.F32_SHARE[(B, T, D, heads, p, masked)]
    print("f32 share (out, dQ, dK, dV)", got, "recorded", rec)
    assert all(_reproduces(g, w) for g, w in zip(got, rec))
    assert all(R.SHARE_FACTOR * w < 0.5 for w in rec)                 # the mean tier is well inside the element-wise bound


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_recorded_inference_attention_shares(name):
    got = R.attn_f32_share(R.attn_case(name))
    print("f32 share", got, "recorded", R.ATTN_F32_SHARE[name])
    assert _reproduces(got, R.ATTN_F32_SHARE[name])


def test_recorded_layernorm_figure():
    got = R.ln_f32_err(R.ln_case(*R.LN_OFFSET_CASE, 100.0))
    print("f32 max err", got, "recorded", R.LN_OFFSET_F32_ERR)
    assert _reproduces(got, R.LN_OFFSET_F32_ERR)
    assert all(R.ln_f32_err(R.ln_case(*c)) < 1e-5 for c in R.LN_CASES)  # the plain cases: far inside 1e-4


def test_ramp_cases_move_the_running_maximum():
    """`grow`: nearly every batch of 16 keys raises the running maximum of the online softmax; `shrink`: none does"""
    frac = {}
    for name in ("grow", "shrink"):
        c = R.attn_case(name)
        q, k, _ = R._qkv(c["qkv"], c["n_seq"], c["S"], c["D"], c["heads"])
        s = q @ k.transpose(-1, -2)
        bm = torch.stack([s[..., j:j + 16].max(-1).values for j in range(0, c["S"], 16)], -1)
        run = torch.cummax(bm, -1).values
        frac[name] = float((bm[..., 1:] > run[..., :-1]).float().mean())
    assert frac["grow"] > 0.9 and frac["shrink"] < 0.1
