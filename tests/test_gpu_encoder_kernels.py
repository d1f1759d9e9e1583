"""GPU: the Transformer-encoder kernels (csrc/encoder.hip, csrc/encoder_train.hip) one by one through the C ABI, in every
launch form, against the float64 restatements of tests/encoder_kernels_ref.py -- the operation's formula on exactly the
bf16 / fp32 values the kernel receives, rounded to bf16 where the kernel rounds.  The bounds, where each comes from and
what float32 arithmetic alone uses of them are stated in that module's docstring; tests/test_encoder_kernels_ref.py shows
on the CPU that a dropped key, a neighbour's keys, a shifted head, a dropped K tail, a skipped LayerNorm column and a wrong
softmax-backward row sum each violate them on the inputs used here.

  erc_enc_gemm_bf16 / _ex      integer operands: EXACT (fp32 output == float64, bf16 output == its rounding), every output /
                               bias / ReLU / epilogue form, tight and padded pitches (NaN in the operands' padding,
                               sentinels around C), the weight-gradient form; random operands: K 2^-24 |a| |w|^T
  erc_enc_attention            both kernels (pair loads, generic), 2^-8 |ref| + 2^-16 P |v| per element
  erc_enc_add_layernorm        1e-4 absolute; bf16 copy exact; mean-100 rows at 4 x the float32 restatement's error
  erc_enc_attention_train/_bwd 2^-8 (|left| |right| + |ref|) per element, mean(err / bound) <= 4 x the float32 restatement's
  EncoderBlock / EncoderTrain  the inference and the training host paths on the same weights against each other
The file takes a few seconds on an MI355X."""
import copy

import pytest
import torch

from tests import encoder_kernels_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 12288.0              # bf16-exact sentinel for memory the kernels must not write
BF, F32 = torch.bfloat16, torch.float32


def _capi():
    from erc_amd import capi
    return capi


def rng_state():
    return torch.tensor(R.RNG, dtype=torch.int64, device=DEV)


def _within(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    worst = float((err - bound).max())
    print("%s: max err %.3e, max (err - bound) %.3e, mean err / bound %.3e" % (what, float(err.max()), worst, R.share(err, bound)))
    assert bool((err <= bound).all()), (what, worst)
    return R.share(err, bound)


# ---------------------------------------------------------------------------------------------------------------- GEMM
def _pitched(t, ld, fill):
    """device copy of the 2-d tensor `t` with row pitch `ld`, the padding columns holding `fill`"""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf


def _launch_gemm(a, w, bias, lda, ldw, ldc, f32, bf16, relu=0, ex=False, **kw):
    """one launch; returns the fp32 and bf16 outputs [M, N] (None where not asked for) after checking the sentinels in
    C's padding columns and guard row"""
    capi = _capi()
    (M, K), N = a.shape, w.shape[0]
    A, W = _pitched(a, lda, float("nan")), _pitched(w, ldw, float("nan"))
    Cf = torch.full((M + 1, ldc), SENT, dtype=F32, device=DEV) if f32 else None
    Ch = torch.full((M + 1, ldc), SENT, dtype=BF, device=DEV) if bf16 else None
    b = None if bias is None else bias.to(DEV)
    if ex or kw:
        capi.enc_gemm_bf16_ex(A, lda, W, ldw, b, Cf, Ch, ldc, M, N, K, relu=relu, **kw)
    else:
        capi.enc_gemm_bf16(A, lda, W, ldw, b, Cf, Ch, ldc, M, N, K, relu=relu)
    outs = []
    for Cm in (Cf, Ch):
        if Cm is not None:
            assert bool((Cm[:M, N:] == SENT).all()) and bool((Cm[M] == SENT).all()), "wrote outside C"
            Cm = Cm[:M, :N].cpu()
        outs.append(Cm)
    return outs


def _int_operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-3, 4, (M, K), generator=g).to(BF)
    w = torch.randint(-3, 4, (N, K), generator=g).to(BF)
    bias = torch.randint(-3, 4, (N,), generator=g).to(F32)
    return a, w, bias


def _assert_exact(outs, ref, what):
    cf, ch = outs
    if cf is not None:
        assert torch.equal(cf.double(), ref), (what, "fp32")
    if ch is not None:
        assert torch.equal(ch, ref.to(BF)), (what, "bf16")


GEMM_SHAPES = [(1, 1, 8), (5, 3, 12), (128, 128, 64), (129, 127, 68), (130, 260, 132), (257, 1100, 24), (40, 24, 2048)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_exact_in_every_launch_form(M, N, K):
    a, w, bias = _int_operands(M, N, K, M + N + K)
    refs = {(hb, relu): R.gemm(a, w, bias if hb else None, bool(relu))[0] for hb in (0, 1) for relu in (0, 1)}
    assert float(R.gemm(a, w)[1].max()) + 3 < 2 ** 24
    for (hb, relu), ref in refs.items():
        for f32, bf16 in ((1, 0), (0, 1), (1, 1)):
            for ex in (False, True):
                outs = _launch_gemm(a, w, bias if hb else None, K, K, N, f32, bf16, relu, ex=ex)
                _assert_exact(outs, ref, (hb, relu, f32, bf16, ex))
    # epilogue 2: multiply by (mask != 0) * scale, the mask read at its own pitch
    g = torch.Generator().manual_seed(K)
    mask = torch.tensor([0.0, 1.0, -2.0])[torch.randint(0, 3, (M, N), generator=g)].to(BF)
    mask_dev = _pitched(mask, N + 8, 1.0)
    for hb in (0, 1):
        ref = refs[(hb, 0)] * 2.0 * (mask != 0)
        outs = _launch_gemm(a, w, bias if hb else None, K, K, N, 1, 1, 0, epilogue=2, mask_src=mask_dev, ld_mask=N + 8, scale=2.0)
        _assert_exact(outs, ref, ("epilogue 2", hb))


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_exact_with_padded_pitches(M, N, K):
    """lda = K + 4, ldw = K + 12, ldc = N + 3: NaN behind every operand row (a read past K poisons the result), sentinels
    in C's padding columns and in a guard row behind C"""
    a, w, bias = _int_operands(M, N, K, M + N + K + 1)
    for relu in (0, 1):
        ref = R.gemm(a, w, bias, bool(relu))[0]
        _assert_exact(_launch_gemm(a, w, bias, K + 4, K + 12, N + 3, 1, 1, relu), ref, ("pitched", relu))
    _assert_exact(_launch_gemm(a, w, None, K + 4, K + 12, N + 3, 1, 0), R.gemm(a, w)[0], "pitched, fp32 only, no bias")
    _assert_exact(_launch_gemm(a, w, None, K + 4, K + 12, N + 3, 0, 1), R.gemm(a, w)[0], "pitched, bf16 only, no bias")


@pytest.mark.parametrize("n_out,n_in", [(72, 24), (130, 36)])
def test_gemm_weight_gradient_form(n_out, n_in):
    """EncoderTrain._wgrad: wgrad[n_out, n_in] = dy^T x from the transposed operands [n_out, Mp] and [n_in, Mp], the token
    axis M = 13 zero-padded to Mp = 16, which is both K and the pitch"""
    capi = _capi()
    M, Mp = 13, 16
    g = torch.Generator().manual_seed(n_out)
    dy, x = torch.randint(-3, 4, (M, n_out), generator=g).to(BF), torch.randint(-3, 4, (M, n_in), generator=g).to(BF)
    tA, tB = torch.full((n_out, Mp), 3.0, dtype=BF, device=DEV), torch.full((n_in, Mp), 3.0, dtype=BF, device=DEV)
    capi.enc_transpose_bf16(dy.to(DEV), n_out, M, n_out, tA, Mp)
    capi.enc_transpose_bf16(x.to(DEV), n_in, M, n_in, tB, Mp)
    assert float(tA[:, M:].float().abs().max()) == 0.0 and torch.equal(tA[:, :M].cpu(), dy.t())
    wg = torch.full((n_out + 1, n_in), SENT, device=DEV)
    capi.enc_gemm_bf16(tA, Mp, tB, Mp, None, wg, None, n_in, n_out, n_in, Mp)
    assert torch.equal(wg[:n_out].cpu().double(), dy.double().t() @ x.double())
    assert bool((wg[n_out] == SENT).all())


def test_gemm_dropout_epilogue_keeps_what_the_generator_keeps():
    """epilogue 1 on a product that is 1 everywhere: kept elements equal `scale`, dropped ones 0, element (row, col)
    decided by the generator at index row * N + col"""
    M, N, K, p, stream = 129, 127, 68, 0.5, 0x102
    a, w = torch.zeros(M, K, dtype=BF), torch.zeros(N, K, dtype=BF)
    a[:, 0], w[:, 0] = 1.0, 1.0
    want = R.keep_mask((M, N), p, R.RNG[1], R.RNG[0], stream)
    assert 0.4 < float((want > 0).float().mean()) < 0.6 and set(want.unique().tolist()) == {0.0, 2.0}
    for relu in (0, 1):
        cf, ch = _launch_gemm(a, w, None, K, K, N, 1, 1, relu, epilogue=1, scale=1 / (1 - p), drop_p=p, rng_state=rng_state(),
                              rng_stream=stream)
        assert torch.equal(cf, want) and torch.equal(ch, want.to(BF))


@pytest.mark.parametrize("M,N,K", [(129, 127, 68), (70, 712, 1380)])
def test_gemm_random_values(M, N, K):
    g = torch.Generator().manual_seed(M + K)
    a, w = torch.randn(M, K, generator=g).to(BF), torch.randn(N, K, generator=g).to(BF)
    ref, absdot = R.gemm(a, w)
    bound = R.gemm_bound(K, absdot)
    cf, ch = _launch_gemm(a, w, None, K, K, N, 1, 1)
    _within(cf, ref, bound, "fp32 output")
    _within(ch, ref, bound + 2.0 ** -8 * ref.abs(), "bf16 output")
    assert torch.equal(ch, cf.to(BF))
    cf2, ch2 = _launch_gemm(a, w, None, K + 4, K + 12, N + 3, 1, 1)
    assert torch.equal(cf2, cf) and torch.equal(ch2, ch)           # the pitch changes no bit


def test_gemm_refusals():
    capi = _capi()
    h = lambda *s: torch.zeros(*s, dtype=BF, device=DEV)
    c = torch.zeros(8, 8, device=DEV)
    with pytest.raises(capi.ErcGraftError):                        # K = 4
        capi.enc_gemm_bf16(h(8, 4), 4, h(8, 4), 4, None, c, None, 8, 8, 8, 4)
    with pytest.raises(capi.ErcGraftError):                        # K % 4 != 0
        capi.enc_gemm_bf16(h(8, 12), 12, h(8, 12), 12, None, c, None, 8, 8, 8, 10)
    with pytest.raises(capi.ErcGraftError):                        # lda % 4 != 0
        capi.enc_gemm_bf16(h(8, 10), 10, h(8, 8), 8, None, c, None, 8, 8, 8, 8)
    for which in (0, 1):                                           # an operand one bf16 element off its 8-byte alignment
        ops = [h(8, 8), h(8, 8)]
        ops[which] = h(8 * 8 + 1)[1:]
        assert ops[which].data_ptr() % 8 == 2
        with pytest.raises(capi.ErcGraftError):
            capi.enc_gemm_bf16(ops[0], 8, ops[1], 8, None, c, None, 8, 8, 8, 8)
    with pytest.raises(capi.ErcGraftError):                        # epilogue 1 without a generator state
        capi.enc_gemm_bf16_ex(h(8, 8), 8, h(8, 8), 8, None, c, None, 8, 8, 8, 8, epilogue=1, scale=2.0, drop_p=0.5)
    with pytest.raises(capi.ErcGraftError):                        # epilogue 2 with a mask pitch below N
        capi.enc_gemm_bf16_ex(h(8, 8), 8, h(8, 8), 8, None, c, None, 8, 8, 8, 8, epilogue=2, mask_src=h(8, 8), ld_mask=4, scale=2.0)
    torch.cuda.synchronize()
    assert float(c.abs().max()) == 0.0                             # nothing was launched


# ------------------------------------------------------------------------------------------------ inference attention
def _run_attention(c, offset_view=False):
    capi = _capi()
    n_rows, D = c["n_seq"] * c["S"], c["D"]
    if offset_view:
        qkv = torch.zeros(n_rows * 3 * D + 1, dtype=BF, device=DEV)[1:].view(n_rows, 3 * D)
        qkv.copy_(c["qkv"])
        assert qkv.data_ptr() % 4 == 2
    else:
        qkv = c["qkv"].to(DEV)
    out = torch.full((n_rows + 1, D), SENT, dtype=BF, device=DEV)
    capi.enc_attention(qkv, c["n_seq"], c["S"], D, c["heads"], out)
    assert bool((out[n_rows] == SENT).all())
    return out[:n_rows].cpu()


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_inference_attention(name):
    c = R.attn_case(name)
    got = _run_attention(c)
    s = _within(got, c["ref"], c["bound"], name)
    assert s <= R.SHARE_FACTOR * R.ATTN_F32_SHARE[name]


def test_inference_attention_from_a_misaligned_view():
    """(3, 17, 24, 6) again, the data pointer one bf16 element off a 4-byte boundary: the pair loads would be misaligned,
    the launch falls back to the generic kernel -- same bound, and the same values as the aligned run up to the two
    kernels' different summation order"""
    c = R.attn_case("s17")
    got = _run_attention(c, offset_view=True)
    _within(got, c["ref"], c["bound"], "s17, offset view")


def test_inference_attention_refusals():
    capi = _capi()
    h = lambda *s: torch.zeros(*s, dtype=BF, device=DEV)
    with pytest.raises(capi.ErcGraftError):                        # head dim 257
        capi.enc_attention(h(4, 3 * 1542), 1, 4, 1542, 6, h(4, 1542))
    with pytest.raises(capi.ErcGraftError):                        # D % heads != 0
        capi.enc_attention(h(4, 3 * 25), 1, 4, 25, 6, h(4, 25))


# --------------------------------------------------------------------------------------------------- add + LayerNorm
def _run_layernorm(c, rows, D):
    capi = _capi()
    yf = torch.full((rows + 1, D), SENT, device=DEV)
    yh = torch.full((rows + 1, D), SENT, dtype=BF, device=DEV)
    capi.enc_add_layernorm(c["a"].to(DEV), c["b"].to(DEV), D, rows, c["gamma"].to(DEV), c["beta"].to(DEV), R.LN_EPS, yf, yh)
    assert bool((yf[rows] == SENT).all()) and bool((yh[rows] == SENT).all())
    assert torch.equal(yh[:rows], yf[:rows].to(BF))
    return yf[:rows].cpu()


@pytest.mark.parametrize("rows,D", R.LN_CASES)
def test_inference_add_layernorm(rows, D):
    c = R.ln_case(rows, D)
    err = float((_run_layernorm(c, rows, D).double() - c["ref"]).abs().max())
    print("max err %.3e" % err)
    assert err < 1e-4


def test_inference_add_layernorm_rows_of_mean_100():
    """two-pass variance: rows of mean 100 over unit spread stay within 4 x what the two-pass float32 restatement loses
    (a one-pass float32 variance loses 7.9e-3, 100 x this tolerance: tests/test_encoder_kernels_ref.py)"""
    rows, D = R.LN_OFFSET_CASE
    c = R.ln_case(rows, D, 100.0)
    err = float((_run_layernorm(c, rows, D).double() - c["ref"]).abs().max())
    print("max err %.3e (float32 restatement %.3e)" % (err, R.LN_OFFSET_F32_ERR))
    assert err <= R.SHARE_FACTOR * R.LN_OFFSET_F32_ERR


def test_inference_add_layernorm_refuses_wide_rows():
    capi = _capi()
    f = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(capi.ErcGraftError):
        capi.enc_add_layernorm(f(2, 2049), f(2, 2049), 2049, 2, f(2049), f(2049), 1e-5, f(2, 2049),
                               torch.zeros(2, 2049, dtype=BF, device=DEV))


# ------------------------------------------------------------------------------------------------- training attention
@pytest.mark.parametrize("B,T,D,heads,p,masked", R.ATTN_TRAIN_CASES)
def test_training_attention_forward_backward(B, T, D, heads, p, masked):
    capi = _capi()
    c = R.attn_train_case(B, T, D, heads, p, masked)
    rec = R.F32_SHARE[(B, T, D, heads, p, masked)]
    M = B * T
    qkv, dout = c["qkv"].to(DEV), c["dout"].to(DEV)
    lengths = c["lengths"].to(DEV) if masked else None
    rs = rng_state() if p > 0 else None
    out = torch.full((M + 1, D), SENT, dtype=BF, device=DEV)
    capi.enc_attention_train(qkv, B, T, D, heads, lengths, p, rs, R.ATTN_STREAM, out)
    assert bool((out[M] == SENT).all())
    s = _within(out[:M], c["out"], c["out_bound"], "out")
    assert s <= R.SHARE_FACTOR * rec[0], ("out", s, rec[0])
    dqkv = torch.full((M + 1, 3 * D), SENT, dtype=BF, device=DEV)
    capi.enc_attention_bwd(qkv, dout, B, T, D, heads, lengths, p, rs, R.ATTN_STREAM, dqkv)
    assert bool((dqkv[M] == SENT).all())
    for i, name in enumerate(("dq", "dk", "dv")):
        part = slice(i * D, (i + 1) * D)
        s = _within(dqkv[:M, part], c["grads"][:, part], c["grads_bound"][:, part], name)
        assert s <= R.SHARE_FACTOR * rec[1 + i], (name, s, rec[1 + i])
    if masked:
        behind = torch.arange(T)[None, :] >= c["lengths"][:, None]                  # [B, T]: keys behind the mask
        rows = behind.reshape(M).to(DEV)
        assert B == 1 or T == 1 or bool(rows.any())
        # they receive no gradient ...
        assert float(dqkv[:M][rows][:, D:].float().abs().sum()) == 0.0
        # ... and have no influence: 1e4 in their k and v rows changes no output bit
        qkv2 = qkv.clone()
        qkv2[rows, D:] = 1e4
        out2 = torch.full((M + 1, D), SENT, dtype=BF, device=DEV)
        capi.enc_attention_train(qkv2, B, T, D, heads, lengths, p, rs, R.ATTN_STREAM, out2)
        assert torch.equal(out2.view(torch.int16), out.view(torch.int16))


# -------------------------------------------------------------------------------------------------------- block level
@pytest.mark.parametrize("B,T,D", [(2, 17, 24), (2, 37, 712)])
def test_inference_and_training_host_paths_agree(B, T, D):
    """EncoderBlock.forward and EncoderTrain.forward(training=False, lengths=None) on the same weights and input, under
    the thresholds test_encoder_block_vs_reference_layers uses against the bf16-rounded oracle.  Both round the same values
    to bf16 at the same places and share the dense product; up to T = 128 EncoderBlock also runs the matrix-core attention,
    so what differs here is the add + LayerNorm kernel (inference form against training form with p = 0) and the host
    plumbing (workspaces, ping-pong buffers, weight shadows made by the transpose kernel against torch's rounding)."""
    from erc_amd.cogmen import COGMENModule
    from erc_amd.encoder import EncoderBlock
    torch.manual_seed(B + T + D)
    m = COGMENModule(D, 100, 17, 2, 6, chained_encoder=True)
    with torch.no_grad():
        for lyr in m.rnn[0].layers:
            lyr.norm1.weight.uniform_(0.5, 1.5), lyr.norm1.bias.uniform_(-0.3, 0.3)
            lyr.norm2.weight.uniform_(0.5, 1.5), lyr.norm2.bias.uniform_(-0.3, 0.3)
    blk = EncoderBlock(copy.deepcopy(m.rnn[0]), DEV)
    m.finalize(DEV)
    x = torch.randn(B, T, D).to(DEV)
    a = blk.forward(x).reshape(B * T, D).to(BF).float().cpu()       # the block's bf16 copy is its fp32 output rounded
    b = m.enc_train.forward(x, None, False, None).float().cpu()
    e = (a - b).abs().flatten()
    print("mean %.2e p99.9 %.2e max %.2e" % (float(e.mean()), float(e.quantile(0.999)), float(e.max())))
    assert float(b.abs().mean()) > 0.3
    assert float(e.mean()) < 1e-3 and float(e.quantile(0.999)) < 1.5e-2
