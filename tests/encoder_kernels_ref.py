"""Float64 restatements of the Transformer-encoder kernels (csrc/encoder.hip, csrc/encoder_train.hip), the bounds the GPU
tests hold the kernels to, and the inputs both the host tests (tests/test_encoder_kernels_ref.py) and the GPU tests
(tests/test_gpu_encoder_kernels.py) use.  torch on the CPU and numpy only: nothing here touches a GPU.

Every kernel of the family takes bf16 operands and accumulates in fp32.  The restatements take exactly the values the
kernel receives (bf16 / fp32 tensors, widened to float64 without loss) and round to bf16 where the kernel does, so what
separates a correct kernel from them is fp32 accumulation order, the library's expf and single-ulp flips of a bf16
rounding whose argument fp32 moved across a rounding boundary.

ROUNDING POINTS (r = float64 -> bfloat16 -> float64, round to nearest even)
  enc_gemm_kernel             none before the output; fp32 output unrounded, bf16 output r(fp32 value)
  enc_attn_kernel / _generic  probabilities stay fp32 in registers; the output is r(.)
  enc_attn_train_fwd_kernel   Pd = r(P * keep) when the probabilities go to LDS (store_rows); the output is r(Pd V)
  enc_attn_bwd_kernel         Pd = r(P * keep) (store_cols), dS = r(P (dP - rowsum(P dP)) scale) (store_cols / store_rows);
                              dQ, dK, dV are r(.) of their products.  dP = (dO V^T) keep stays fp32.
  enc_add_ln_kernel           none; the bf16 copy is r(fp32 output)

BOUNDS (element-wise unless stated; `absdot` = |left| @ |right| of the product that makes the element)
  GEMM, integer operands      operands in [-3, 3] are bf16-exact and with K <= 2048 every partial sum is an integer below
                              2^24: the fp32 result is exact in ANY order -> fp32 output == float64 bit for bit, bf16 output
                              == r(float64) bit for bit.
  GEMM, random operands       |fp32 - ref| <= K 2^-24 absdot (the standard forward bound of a length-K fp32 sum);
                              bf16 output: that + 2^-8 |ref|.
  inference attention         |got - ref| <= 2^-8 |ref| + 2^-16 pabs, pabs = P @ |v|: the output's bf16 rounding, and fp32
                              expf + accumulation over at most 128 keys.
  training attention          |got - ref| <= 2^-8 absdot + 2^-8 |ref| for out, dQ, dK, dV: every bf16-rounded left operand
                              (Pd or dS) one ulp off, plus the bf16 output.  Second tier: mean(err / bound) over ALL elements
                              <= 4 x the figure of the fp32 restatement below (F32_SHARE).
  add + LayerNorm             1e-4 absolute on O(1) outputs (the project's existing figure); bf16 copy == r(fp32 output);
                              rows of mean 100 over unit spread: 4 x the fp32 restatement's own error (LN_OFFSET_F32_ERR).

WHAT FP32 ALONE COSTS.  The f32_restatement_* twins repeat the non-exact operations in numpy float32 with the same rounding
points; mean(err / bound) of a twin against float64 on the GPU tests' inputs is the share of the bound that fp32
arithmetic uses up by itself.  Measured from the references alone (never from a kernel), recorded in F32_SHARE /
ATTN_F32_SHARE / LN_OFFSET_F32_ERR below and re-measured by tests/test_encoder_kernels_ref.py on every run (they must
reproduce to 10 %: the figures are dominated by the bf16 rounding of the output, which does not depend on the BLAS in use).
The factor 4 the GPU tests allow on top covers another accumulation order and the library's expf.

  training attention, mean(err / bound), case = (B, T, D, heads, p, masked)      out     dQ      dK      dV
      (3, 13, 24, 6, 0.0, masked)                                                 0.083   0.092   0.062   0.058
      (2, 37, 712, 8, 0.5, masked)                                                0.078   0.080   0.053   0.052
      (2, 110, 1380, 6, 0.5, masked)                                              0.052   0.057   0.038   0.034
      (2, 128, 96, 6, 0.0, unmasked)                                              0.031   0.037   0.038   0.029
      (1, 1, 24, 6, 0.0, masked)        one key, probability 1: exact             0       0       0       0
      (4, 33, 1380, 6, 0.3, masked)                                               0.068   0.073   0.058   0.052
      (2, 17, 24, 6, 0.5, masked)                                                 0.102   0.092   0.076   0.082
      (2, 97, 1164, 6, 0.0, masked)                                               0.042   0.049   0.031   0.026
  inference attention, mean(err / bound): 0.33 .. 0.36 in every case (0 for one key) -- the output's bf16 rounding alone
      uses a third of the bound, so 4 x the figure is above 1 and only the element-wise bound bites there
  add + LayerNorm, rows of mean 100, (rows, D) = (6, 712): max |err| 1.99e-5 (plain cases: at most 6.4e-7);
      a one-pass float32 variance on the same rows: 7.9e-3
The kernels on an MI355X measure the same mean(err / bound) figures to three digits (most of each figure is the output's
own bf16 rounding, which the kernel and the restatement share), and 1.47e-5 on the mean-100 rows.
"""
import functools
import math

import numpy as np
import torch

from tests.test_gpu_encoder_train import erc_uniform_np, keep_mask  # noqa: F401  (re-exported: one restatement of the generator)

RNG = (7, 12345)            # {offset, seed} the tests hand the kernels
ATTN_STREAM = 0x100         # generator stream of the attention dropout site


def r(t):
    """float64 -> bfloat16 -> float64"""
    return t.to(torch.bfloat16).to(torch.float64)


def identity(t):
    return t


def share(err, bound):
    """mean(err / bound) over all elements; an element whose bound is 0 must be exact (0 / 0 counts 0, x / 0 inf)"""
    err, bound = err.double().flatten(), bound.double().flatten()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.mean())


# ---------------------------------------------------------------------------------------------------------------- GEMM
def gemm(a, w, bias=None, relu=False):
    """(a @ w.T + bias [relu], |a| @ |w|.T) in float64"""
    a, w = a.double(), w.double()
    y = a @ w.t()
    if bias is not None:
        y = y + bias.double()
    if relu:
        y = y.clamp_min(0.0)
    return y, a.abs() @ w.abs().t()


def gemm_bound(K, absdot):
    return K * 2.0 ** -24 * absdot


# ----------------------------------------------------------------------------------------------------------- attention
def _heads(t, n_seq, S, heads):
    """[n_seq * S, heads * hd] -> [n_seq, heads, S, hd]"""
    return t.reshape(n_seq, S, heads, -1).permute(0, 2, 1, 3)


def _rows(t):
    """[n_seq, heads, S, hd] -> [n_seq * S, heads * hd]"""
    n_seq, heads, S, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(n_seq * S, heads * hd)


def _qkv(qkv, n_seq, S, D, heads):
    qkv = qkv.double()
    return tuple(_heads(qkv[:, i * D:(i + 1) * D], n_seq, S, heads) for i in range(3))


def _probabilities(q, k, lengths):
    S, hd = q.shape[2], q.shape[3]
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    if lengths is not None:
        pad = torch.arange(S)[None, :] >= lengths[:, None]
        s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    s = s - s.max(-1, keepdim=True).values
    e = s.exp()
    return e / e.sum(-1, keepdim=True)


def attention(qkv, n_seq, S, D, heads):
    """inference form: (softmax(q k^T / sqrt(hd)) v, P @ |v|) per (sequence, head) over all S positions, [n_seq * S, D]"""
    q, k, v = _qkv(qkv, n_seq, S, D, heads)
    P = _probabilities(q, k, None)
    return _rows(P @ v), _rows(P @ v.abs())


def attn_bound(ref, pabs):
    return 2.0 ** -8 * ref.abs() + 2.0 ** -16 * pabs


def attention_train(qkv, n_seq, S, D, heads, lengths=None, keep=None, rnd=r):
    """training form: Pd = rnd(P * keep), out = Pd V.  Returns (out, Pd @ |V|), both [n_seq * S, D]."""
    q, k, v = _qkv(qkv, n_seq, S, D, heads)
    P = _probabilities(q, k, lengths)
    Pd = rnd(P if keep is None else P * keep.double())
    return _rows(Pd @ v), _rows(Pd.abs() @ v.abs())


def attention_train_bwd(qkv, dout, n_seq, S, D, heads, lengths=None, keep=None, rnd=r):
    """(dqkv, absdot), both [n_seq * S, 3 D] (dq | dk | dv):
    Pd = rnd(P keep); dV = Pd^T dO; dP = (dO V^T) keep; dS = rnd(P (dP - rowsum(P dP)) scale); dK = dS^T Q; dQ = dS K"""
    q, k, v = _qkv(qkv, n_seq, S, D, heads)
    do = _heads(dout.double(), n_seq, S, heads)
    scale = 1.0 / math.sqrt(q.shape[3])
    P = _probabilities(q, k, lengths)
    kp = 1.0 if keep is None else keep.double()
    Pd = rnd(P * kp)
    dP = (do @ v.transpose(-1, -2)) * kp
    dS = rnd(P * (dP - (P * dP).sum(-1, keepdim=True)) * scale)
    PdT, dST = Pd.transpose(-1, -2), dS.transpose(-1, -2)
    grads = torch.cat([_rows(dS @ k), _rows(dST @ q), _rows(PdT @ do)], 1)
    absdot = torch.cat([_rows(dS.abs() @ k.abs()), _rows(dST.abs() @ q.abs()), _rows(PdT.abs() @ do.abs())], 1)
    return grads, absdot


def attn_train_bound(ref, absdot):
    return 2.0 ** -8 * absdot + 2.0 ** -8 * ref.abs()


# ----------------------------------------------------------------------------------------------------------- LayerNorm
def add_layernorm(a, b, gamma, beta, eps):
    x = a.double() + b.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)          # two passes
    return (x - mean) / (var + eps).sqrt() * gamma.double() + beta.double()


# ------------------------------------------------------------------------------------------------ float32 restatements
def _bf16_np(x):
    """numpy float32 -> nearest-even bf16, kept as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def _np32(t):
    return t.to(torch.float32).numpy()


def _probabilities_np(q, k, lengths):
    S, hd = q.shape[2], q.shape[3]
    s = np.matmul(q * np.float32(1.0 / math.sqrt(hd)), np.swapaxes(k, -1, -2))      # the kernels scale q / the scores in fp32
    if lengths is not None:
        pad = np.arange(S)[None, :] >= lengths.numpy()[:, None]
        s = np.where(pad[:, None, None, :], np.float32(-np.inf), s)
    e = np.exp(s - s.max(-1, keepdims=True), dtype=np.float32)
    return e / e.sum(-1, keepdims=True, dtype=np.float32)


def _qkv_np(qkv, n_seq, S, D, heads):
    return tuple(np.ascontiguousarray(_np32(_heads(qkv[:, i * D:(i + 1) * D], n_seq, S, heads))) for i in range(3))


def _rows_t(x):
    return _rows(torch.from_numpy(np.ascontiguousarray(x)))


def f32_restatement_attention(qkv, n_seq, S, D, heads):
    q, k, v = _qkv_np(qkv, n_seq, S, D, heads)
    return _rows_t(_bf16_np(np.matmul(_probabilities_np(q, k, None), v)))


def f32_restatement_attention_train(qkv, n_seq, S, D, heads, lengths=None, keep=None):
    q, k, v = _qkv_np(qkv, n_seq, S, D, heads)
    P = _probabilities_np(q, k, lengths)
    Pd = _bf16_np(P if keep is None else P * _np32(keep))
    return _rows_t(_bf16_np(np.matmul(Pd, v)))


def f32_restatement_attention_train_bwd(qkv, dout, n_seq, S, D, heads, lengths=None, keep=None):
    q, k, v = _qkv_np(qkv, n_seq, S, D, heads)
    do = np.ascontiguousarray(_np32(_heads(dout, n_seq, S, heads)))
    scale = np.float32(1.0 / math.sqrt(q.shape[3]))
    P = _probabilities_np(q, k, lengths)
    kp = np.float32(1.0) if keep is None else _np32(keep)
    Pd = _bf16_np(P * kp)
    dP = np.matmul(do, np.swapaxes(v, -1, -2)) * kp
    dS = _bf16_np(P * (dP - (P * dP).sum(-1, keepdims=True, dtype=np.float32)) * scale)
    PdT, dST = np.swapaxes(Pd, -1, -2), np.swapaxes(dS, -1, -2)
    return torch.cat([_rows_t(_bf16_np(np.matmul(dS, k))), _rows_t(_bf16_np(np.matmul(dST, q))),
                      _rows_t(_bf16_np(np.matmul(PdT, do)))], 1)


def f32_restatement_add_layernorm(a, b, gamma, beta, eps):
    x = _np32(a) + _np32(b)
    D = np.float32(x.shape[-1])
    mean = x.sum(-1, keepdims=True, dtype=np.float32) / D
    d = x - mean
    var = (d * d).sum(-1, keepdims=True, dtype=np.float32) / D
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps))
    return torch.from_numpy(d * rstd * _np32(gamma) + _np32(beta))


# ------------------------------------------------------------------------------------------------- the GPU tests' inputs
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(round(1000 * k)) for i, k in enumerate(key)) % (2 ** 31))


# (B, T, D, heads, p, masked): the existing test's list, + a dropout case two rows past one 16-row tile, + hd = 194 (its
# last 96-column chunk is partial)
ATTN_TRAIN_CASES = [(3, 13, 24, 6, 0.0, True), (2, 37, 712, 8, 0.5, True), (2, 110, 1380, 6, 0.5, True),
                    (2, 128, 96, 6, 0.0, False), (1, 1, 24, 6, 0.0, True), (4, 33, 1380, 6, 0.3, True),
                    (2, 17, 24, 6, 0.5, True), (2, 97, 1164, 6, 0.0, True)]


@functools.lru_cache(maxsize=None)
def attn_train_case(B, T, D, heads, p, masked):
    """inputs, float64 references and bounds of one training-attention case (computed once, shared, never modified)"""
    g = _gen(B, T, D, heads, p, masked)
    qkv = (torch.randn(B * T, 3 * D, generator=g) * 0.7).to(torch.bfloat16)
    dout = torch.randn(B * T, D, generator=g).to(torch.bfloat16)
    lengths = None
    if masked:
        lengths = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int64)
        lengths[0] = T
        if B > 1 and T > 1 and int(lengths[1:].min()) == T:
            lengths[1] = T // 2 + 1                      # at least one sequence with keys behind the mask
    keep = keep_mask((B, heads, T, T), p, RNG[1], RNG[0], ATTN_STREAM) if p > 0 else None
    out, out_abs = attention_train(qkv, B, T, D, heads, lengths, keep)
    grads, grads_abs = attention_train_bwd(qkv, dout, B, T, D, heads, lengths, keep)
    return dict(B=B, T=T, D=D, heads=heads, p=p, qkv=qkv, dout=dout, lengths=lengths, keep=keep, out=out,
                out_bound=attn_train_bound(out, out_abs), grads=grads, grads_bound=attn_train_bound(grads, grads_abs))


def attn_train_f32_share(case):
    """(out, dQ, dK, dV): mean(err / bound) of the float32 restatement against float64"""
    c, D = case, case["D"]
    a = (c["qkv"], c["B"], c["T"], D, c["heads"])
    o32 = f32_restatement_attention_train(*a, c["lengths"], c["keep"])
    g32 = f32_restatement_attention_train_bwd(c["qkv"], c["dout"], *a[1:], c["lengths"], c["keep"])
    ge, gb = (g32.double() - c["grads"]).abs(), c["grads_bound"]
    return (share((o32.double() - c["out"]).abs(), c["out_bound"]),) + tuple(
        share(ge[:, i * D:(i + 1) * D], gb[:, i * D:(i + 1) * D]) for i in range(3))


# inference attention: name -> (n_seq, S, D, heads, key scale per position or None)
ATTN_CASES = {
    "one": (1, 1, 24, 6, None), "s15": (3, 15, 24, 6, None), "s16": (3, 16, 24, 6, None), "s17": (3, 17, 24, 6, None),
    "hd89": (2, 37, 712, 8, None), "hd230": (2, 110, 1380, 6, None), "hd256": (1, 33, 1536, 6, None),
    "hd2": (5, 3, 12, 6, None), "grow": (2, 40, 96, 6, "grow"), "shrink": (2, 40, 96, 6, "shrink"),
}


@functools.lru_cache(maxsize=None)
def attn_case(name):
    n_seq, S, D, heads, ramp = ATTN_CASES[name]
    g = _gen(n_seq, S, D, heads, len(name))
    x = torch.randn(n_seq * S, 3 * D, generator=g) * 0.7
    if ramp is not None:
        # keys 4 x larger from one batch of 16 to the next (or smaller): the running maximum of the online softmax moves
        # (or stays) at every batch and the accumulated sums are rescaled by far more than an ulp
        step = torch.arange(S) // 16
        sc = 0.1 * 4.0 ** (step if ramp == "grow" else step.max() - step)
        x[:, D:2 * D] *= sc.repeat(n_seq)[:, None]
    qkv = x.to(torch.bfloat16)
    ref, pabs = attention(qkv, n_seq, S, D, heads)
    return dict(n_seq=n_seq, S=S, D=D, heads=heads, qkv=qkv, ref=ref, bound=attn_bound(ref, pabs))


def attn_f32_share(case):
    c = case
    got = f32_restatement_attention(c["qkv"], c["n_seq"], c["S"], c["D"], c["heads"])
    return share((got.double() - c["ref"]).abs(), c["bound"])


LN_CASES = [(1, 1), (5, 63), (5, 64), (5, 65), (9, 24), (6, 1380), (7, 2048)]
LN_OFFSET_CASE = (6, 712)
LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_case(rows, D, offset=0.0):
    g = _gen(rows, D, offset)
    a, b = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g) * 2
    if offset:
        a, b = torch.randn(rows, D, generator=g) * 0.6 + offset * 0.75, torch.randn(rows, D, generator=g) * 0.8 + offset * 0.25
    gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.3
    return dict(a=a, b=b, gamma=gamma, beta=beta, ref=add_layernorm(a, b, gamma, beta, LN_EPS))


def ln_f32_err(case):
    c = case
    return float((f32_restatement_add_layernorm(c["a"], c["b"], c["gamma"], c["beta"], LN_EPS).double() - c["ref"]).abs().max())


# ------------------------------------------------------------------------------------- measured float32 figures (see top)
# training attention: mean(err / bound) of (out, dQ, dK, dV).  About a tenth of the bound or less: most of it is the bf16
# rounding of the output itself (at most half of 2^-8 |ref|, against a bound that also carries 2^-8 absdot).
F32_SHARE = {
    (3, 13, 24, 6, 0.0, True): (8.293e-02, 9.199e-02, 6.151e-02, 5.846e-02),
    (2, 37, 712, 8, 0.5, True): (7.808e-02, 7.981e-02, 5.339e-02, 5.213e-02),
    (2, 110, 1380, 6, 0.5, True): (5.201e-02, 5.684e-02, 3.760e-02, 3.375e-02),
    (2, 128, 96, 6, 0.0, False): (3.086e-02, 3.748e-02, 3.778e-02, 2.921e-02),
    (1, 1, 24, 6, 0.0, True): (0.0, 0.0, 0.0, 0.0),
    (4, 33, 1380, 6, 0.3, True): (6.752e-02, 7.344e-02, 5.771e-02, 5.219e-02),
    (2, 17, 24, 6, 0.5, True): (1.024e-01, 9.187e-02, 7.601e-02, 8.152e-02),
    (2, 97, 1164, 6, 0.0, True): (4.191e-02, 4.911e-02, 3.107e-02, 2.615e-02),
}
# inference attention: mean(err / bound).  A third of the bound is the output's own bf16 rounding (nothing is rounded before
# it), so 4 x this figure is above 1 and the mean says nothing the element-wise bound does not: recorded for the record.
ATTN_F32_SHARE = {
    "one": 0.0, "s15": 3.471e-01, "s16": 3.520e-01, "s17": 3.319e-01, "hd89": 3.404e-01, "hd230": 3.301e-01,
    "hd256": 3.412e-01, "hd2": 3.618e-01, "grow": 3.364e-01, "shrink": 3.380e-01,
}
# add + LayerNorm on rows of mean 100 over unit spread, (rows, D) = LN_OFFSET_CASE: max |err| of the two-pass float32
# restatement (the row sum of 712 values near 100 carries it; the plain cases of LN_CASES reach 6.4e-7 at most).  A one-pass
# float32 variance E[x^2] - mean^2 cancels 1e4 against 1e4 to leave a variance of 1: 7.9e-3 on the output (measured).
LN_OFFSET_F32_ERR = 1.991e-05
SHARE_FACTOR = 4.0          # what the GPU tests allow on top: another accumulation order, the library's expf
