"""Float64 restatement of COGMEN's training head and BatchNorm kernels (csrc/head.hip: erc_head_fused, erc_head_fused_bn,
erc_bn_batch_stats, erc_bn_bwd_apply), its float32 twin, the inputs and the case table that both the host tests
(tests/test_head_ref.py) and the GPU tests (tests/test_gpu_head.py) use, and the checker both apply to what a launch wrote
(`check_outputs`: the host tests feed it the float32 twin with one deliberate error).  numpy, and torch on the CPU for the bf16
rounding: nothing here touches a GPU.

THE CHAIN (track_mm/cogmen.py:67-73,116-122,185-188), per row of H2 [N, F], saved = mean | rstd of the batch:
    xhat = (H2 - mean) rstd          y = xhat gamma + beta           H3 = y > 0 ? y : slope y
    Z = relu(H3 W0^T + b0) keep      logits = Z W3^T + b3            keep = 0 or 1 / (1 - p): the inverted-dropout mask
    loss = sum_i w_i (lse_i - logit_i[y_i]) / sum_i w_i              w_i = weight[y_i] (1 without class weights)
    dlogits = w_i / sum w (softmax - onehot)      dZ = Z > 0 ? (dlogits W3) keep : 0      dY = (dZ W0) (y > 0 ? 1 : slope)
    dbeta = sum_rows dY     dgamma = sum_rows dY xhat     bn_bwd = dbeta / N | dgamma / N
    stats = {loss, #rows whose FIRST maximal logit is the label (torch.argmax), sum w}
    dH2 = gamma rstd (dY - bn_bwd[c] - xhat bn_bwd[F + c])           (erc_bn_bwd_apply)
At y == 0 and at a zero pre-activation both torch and the kernel take the `else` side (slope, and 0): so does this file.

WORKGROUP RECORDS.  The head leaves one record of PART = 228 floats per workgroup: [0, 112) sum dY, [112, 224) sum dY xhat (columns
>= F zero), [224] sum w_i (lse_i - logit_i[y_i]) (not normalised), [225] hits, [226] sum w (the same in every record), over the
rows of that workgroup: rows [g rpw, (g + 1) rpw) for head_fused_kernel (`row_groups`), the row tiles 4 b + w + 4 G k of workgroup
b for the throughput form above 8192 rows (`rows_kernel_groups`, G = min(ceil(tiles / 4), 512) workgroups).

BOUNDS the GPU tests hold the kernels to (never taken from a kernel's output):
  exact inputs   (`exact_inputs`) every ReLU / LeakyReLU / argmax decision and H3, Z, logits are exact in fp32 in any summation
                 order: those are compared bit for bit, ties in the maximal logit included.
  random inputs  (`random_inputs`) err / scale per output group against float64, scale = the group's largest reference entry, must
                 stay below BOUND[group] = 4 x the float32 twin's worst figure over CASES (F32_WORST), one significant digit up.
                 Rows whose decisions fp32 may legitimately flip (`fragile_rows`) are left out of dZ and dY only; at most 1 % of
                 the rows may be fragile, and at most 1 % may have a top-two logit margin below 1e-4 (left out of #correct).
  column sums    link 1: the kernel's records / bn_bwd / dgamma / dbeta against float64 sums of the kernel's OWN dY and the
                 reference xhat, |err| <= 32 2^-24 sum |terms| per record (fp32 sums of a few rounding levels; the last arriver
                 adds the records in float64).  Link 2: dY against the reference off the fragile rows.

F32_WORST was measured from the two restatements alone (tests/test_head_ref.py re-measures it on every run: every case must stay
inside BOUND and the worst figure within 0.5 .. 1.5 x the recorded one); BOUND = 4 x, one significant digit up:
    group             H3       Z        logits   dlogits  dZ       dY       bn       loss
    random, worst     1.30e-7  5.31e-7  5.41e-7  1.78e-7  2.32e-7  2.97e-7  3.51e-6  9.49e-8
    random, BOUND     6e-7     3e-6     3e-6     8e-7     1e-6     2e-6     2e-5     4e-7
    exact, worst      0        0        0        3.46e-7  8.84e-6  1.29e-5  1.64e-5  4.00e-7
    exact, BOUND      bit for bit                2e-6     4e-5     6e-5     7e-5     2e-6
(the exact inputs' larger figures come from their one-row cases: with a single row and two classes sharing a W3 row, dZ = dlogits W3
cancels to a small fraction of its terms, and the scale is the group's largest entry.)  `bn` of the random inputs is the float32
twin's column sum over up to 32 801 rows; the kernels add their records in float64 and are held to link 1 instead.
"""
import functools
import math

import numpy as np
import torch

from tests.test_gpu_encoder_train import erc_uniform_np  # one restatement of the generator (csrc/erc_common.h erc_uniform)

PART = 228            # floats per workgroup record (erc_head_fused_part_floats())
RNG = (7, 12345)      # {offset, seed} of every dropout draw in these tests
EPS, MOMENTUM = 1e-5, 0.1
FRAGILE = 2.0 ** -16  # relative margin below which an fp32 kernel may take the other side of a ReLU / LeakyReLU decision
MARGIN = 1e-4         # top-two logit margin below which a row is left out of #correct
U = 2.0 ** -24        # half a unit in the last place of a float
NAN16 = 0x7FC0        # the bf16 NaN the bf16 outputs are prefilled with
GROUPS = ("H3", "Z", "logits", "dlogits", "dZ", "dY", "bn", "loss")


# ------------------------------------------------------------------------------------------------- BatchNorm statistics
def _finish_stats(mean, var, N, eps, momentum, running_mean, running_var, unbiased_rstd=False):
    unbiased = var * N / (N - 1) if N > 1 else var
    rstd = 1.0 / np.sqrt((unbiased if unbiased_rstd else var) + np.float64(np.float32(eps)))
    mom = np.float64(np.float32(momentum))          # the kernels hold momentum and eps as floats
    keep_old = np.float64(np.float32(1.0) - np.float32(momentum))
    rm = keep_old * np.asarray(running_mean, np.float64) + mom * mean
    rv = keep_old * np.asarray(running_var, np.float64) + mom * unbiased
    return dict(saved=np.concatenate([mean, rstd]), running_mean=rm, running_var=rv, mean=mean, var=var,
                scale_mean=np.abs(keep_old * np.asarray(running_mean, np.float64)) + np.abs(mom * mean))


def bn_stats(x, eps, momentum, running_mean, running_var, unbiased_rstd=False):
    """two-pass column mean and biased variance of x [N, F] (nn.BatchNorm1d in training mode): saved = mean | rstd, running
    statistics updated with the unbiased variance (at N = 1 the variance unchanged).  ``unbiased_rstd`` is mutation 8."""
    x = np.asarray(x, np.float64)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return _finish_stats(mean, var, x.shape[0], eps, momentum, running_mean, running_var, unbiased_rstd)


def bn_finalize(bn_part_f32, N, eps, momentum, running_mean, running_var, unbiased_rstd=False):
    """the contract of erc_head_fused_bn: the float32 per-tile records [tiles][2F] = sum x | sum x^2 added in float64,
    var = max(0, sxx / N - m^2).  ``unbiased_rstd`` is mutation 8."""
    part = np.asarray(bn_part_f32)
    assert part.dtype == np.float32
    s = part.astype(np.float64).sum(0)
    F = s.shape[0] // 2
    mean = s[:F] / N
    var = np.maximum(0.0, s[F:] / N - mean * mean)
    return _finish_stats(mean, var, N, eps, momentum, running_mean, running_var, unbiased_rstd)


def bn_tile_sums(H2, n_tiles=None):
    """float32 [tiles][2F] = sum x | sum x^2 of 16 rows each, computed in float64 and rounded once -- what erc_cogmen_fwd_tile
    (bn_fused = 2) leaves; tiles at or beyond ceil(N / 16) hold zeros (their rows put zeros into the sums)"""
    x = np.asarray(H2, np.float64)
    N, F = x.shape
    tiles = -(-N // 16)
    out = np.zeros((n_tiles or tiles, 2 * F), np.float32)
    for t in range(tiles):
        blk = x[16 * t:16 * t + 16]
        out[t, :F], out[t, F:] = blk.sum(0), (blk * blk).sum(0)
    return out


# ------------------------------------------------------------------------------------------------- dropout mask
def keep(seed, offset, N, F, p):
    """the inverted-dropout mask head.hip draws: element index row * F + col, no stream folded into the seed; 0 or 1 / (1 - p)"""
    if p == 0:
        return np.ones((N, F))
    idx = np.arange(N * F, dtype=np.uint64)
    u = erc_uniform_np(np.uint64(seed), offset, idx).reshape(N, F)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return (u >= np.float32(p)).astype(np.float64) * np.float64(scale)


# ------------------------------------------------------------------------------------------------- the chain
def _chain(dt, H2, saved, gamma, beta, slope, W0, b0, W3, b3, labels, weight, keep, mutation=None):
    """the chain above in dtype ``dt`` with plain ``@``.  ``mutation`` (tests/test_head_ref.py only): one deliberate error"""
    c = lambda a: np.asarray(a, dtype=dt)
    H2, saved, gamma, beta, W0, b0, W3, b3, keep = (c(a) for a in (H2, saved, gamma, beta, W0, b0, W3, b3, keep))
    slope = dt(slope)
    labels = np.asarray(labels, np.int64)
    N, F = H2.shape
    C = W3.shape[0]
    mean, rstd = saved[:F], saved[F:]
    xhat = (H2 - mean) * rstd
    y = xhat * gamma + beta
    H3 = np.where(y > 0, y, y * slope)
    pre = H3 @ W0.T + b0
    Z = np.maximum(pre, 0) * keep
    logits = Z @ W3.T + b3
    mx = logits.max(1, keepdims=True)
    lse = mx + np.log(np.exp(logits - mx).sum(1, keepdims=True))
    w = c(np.asarray(weight)[labels]) if weight is not None else np.ones(N, dt)
    wsum = float(np.asarray(w, np.float64).sum()) if weight is not None else float(N)      # the kernels add the weights in fp64
    norm = float(N) if mutation == "loss_norm_n" else wsum
    onehot = (np.arange(C)[None, :] == labels[:, None]).astype(dt)
    row_loss = w * (lse[:, 0] - logits[np.arange(N), labels])
    coef = (np.ones(N, dt) if mutation == "unweighted_dlogits" else w) * dt(1.0 / norm)
    dlogits = coef[:, None] * (np.exp(logits - lse) - onehot)
    dZ = np.where(Z > 0, (dlogits @ W3) * keep, 0).astype(dt)
    dH3 = dZ @ W0
    side = (H3 * gamma > 0) if mutation == "lrelu_sign" else (y > 0)
    dY = (dH3 * np.where(side, dt(1), slope)).astype(dt)
    if mutation == "dead_last_columns":
        dY[:, 96:] = 0
    pred = (C - 1 - logits[:, ::-1].argmax(1)) if mutation == "argmax_last" else logits.argmax(1)
    hit = pred == labels
    sdy, sdyx = dY.sum(0, dtype=dt), (dY * xhat).sum(0, dtype=dt)
    return dict(xhat=xhat, y=y, H3=H3, pre=pre, Z=Z, logits=logits, dlogits=dlogits, dZ=dZ, dY=dY, row_loss=row_loss, hit=hit,
                w=w, wsum=wsum, sum_dY=sdy, sum_dYx=sdyx, bn_bwd=np.concatenate([sdy, sdyx]) / dt(N), dgamma=sdyx, dbeta=sdy,
                stats=np.array([float(row_loss.sum(dtype=dt)) / norm, float(hit.sum()), wsum]), N=N, F=F, C=C)


def head(H2, saved, gamma, beta, slope, W0, b0, W3, b3, labels, weight, keep):
    """float64: H3, Z, logits, dlogits, dZ, dY, sum_dY, sum_dYx, bn_bwd, dgamma, dbeta, stats = {loss, #correct, sum w}"""
    return _chain(np.float64, H2, saved, gamma, beta, slope, W0, b0, W3, b3, labels, weight, keep)


def head_f32(H2, saved, gamma, beta, slope, W0, b0, W3, b3, labels, weight, keep, mutation=None):
    """the same formulas, float32 throughout: the yardstick of the bounds"""
    return _chain(np.float32, H2, saved, gamma, beta, slope, W0, b0, W3, b3, labels, weight, keep, mutation)


def bn_bwd_apply(x, saved, gamma, bn_bwd, dY, dt=np.float64):
    c = lambda a: np.asarray(a, dtype=dt)
    x, saved, gamma, bn_bwd, dY = (c(a) for a in (x, saved, gamma, bn_bwd, dY))
    F = x.shape[1]
    xhat = (x - saved[:F]) * saved[F:]
    return gamma * saved[F:] * (dY - bn_bwd[:F] - xhat * bn_bwd[F:])


# ------------------------------------------------------------------------------------------------- workgroup records
def row_groups(N, rows_per_workgroup):
    return [np.arange(r, min(N, r + rows_per_workgroup)) for r in range(0, N, rows_per_workgroup)]


def rows_kernel_groups(n_cap, n):
    """throughput form (more than 8192 rows): workgroup b of G = min(ceil(tiles / 4), 512) takes the row tiles 4 b + w + 4 G k;
    the grid is sized for the capacity n_cap, the rows end at n"""
    G = min(-(-(-(-n_cap // 16)) // 4), 512)
    tiles = -(-n // 16)
    out = []
    for b in range(G):
        ts = [t for w in range(4) for t in range(4 * b + w, tiles, 4 * G)]
        out.append(np.concatenate([np.arange(16 * t, min(n, 16 * t + 16)) for t in ts]) if ts else np.arange(0))
    return out


def records(out, groups, dY=None, stale=None):
    """float64 [len(groups)][PART] records of a chain result ``out`` (``dY``: another dY, e.g. a kernel's own, in its place;
    ``stale``: mutation 9, records of an earlier launch left behind the live ones)"""
    F = out["F"]
    dY = np.asarray(out["dY"] if dY is None else dY, np.float64)
    xhat = np.asarray(out["xhat"], np.float64)
    rec = np.zeros((len(groups), PART))
    for g, rows in enumerate(groups):
        rec[g, :F] = dY[rows].sum(0)
        rec[g, 112:112 + F] = (dY[rows] * xhat[rows]).sum(0)
        rec[g, 224] = np.asarray(out["row_loss"], np.float64)[rows].sum()
        rec[g, 225] = out["hit"][rows].sum()
        rec[g, 226] = out["wsum"]
    return rec if stale is None else np.concatenate([rec, stale])


def record_abs(out, groups, dY):
    """sum |terms| of the two column sums of every record (the scale of link 1's bound)"""
    F = out["F"]
    dY, xhat = np.abs(np.asarray(dY, np.float64)), np.abs(np.asarray(out["xhat"], np.float64))
    rec = np.zeros((len(groups), PART))
    for g, rows in enumerate(groups):
        rec[g, :F] = dY[rows].sum(0)
        rec[g, 112:112 + F] = (dY[rows] * xhat[rows]).sum(0)
    return rec


# ------------------------------------------------------------------------------------------------- decisions fp32 may flip
def fragile_rows(out, W0, b0, gamma, beta):
    """rows with a pre-activation |H3 W0^T + b0| < 2^-16 (|H3| |W0|^T + |b0|), or a BatchNorm output within the same relative
    margin of 0, in the float64 result ``out``"""
    W0, b0 = np.asarray(W0, np.float64), np.asarray(b0, np.float64)
    m1 = np.abs(out["pre"]) < FRAGILE * (np.abs(out["H3"]) @ np.abs(W0).T + np.abs(b0))
    m2 = np.abs(out["y"]) < FRAGILE * (np.abs(out["xhat"] * np.asarray(gamma, np.float64)) + np.abs(np.asarray(beta, np.float64)))
    return m1.any(1) | m2.any(1)


def close_rows(out):
    """rows whose float64 top-two logit margin is below MARGIN (none when there is one class)"""
    lg = out["logits"]
    if lg.shape[1] < 2:
        return np.zeros(lg.shape[0], bool)
    top = np.sort(lg, 1)[:, -2:]
    return (top[:, 1] - top[:, 0]) < MARGIN


# ------------------------------------------------------------------------------------------------- inputs
def _labels_weight(r, N, C, weighted):
    labels = r.randint(0, C, N).astype(np.int64)
    weight = (0.5 + r.rand(C)).astype(np.float32) if weighted else None
    return labels, weight


def random_inputs(N, F, C, weighted, seed):
    r = np.random.RandomState(seed)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    b = 1.0 / math.sqrt(F)
    P = dict(H2=f(0.3 + 1.5 * r.randn(N, F)), gamma=f(0.5 + r.rand(F)), beta=f(0.3 * r.randn(F)), slope=0.01,
             W0=f(r.uniform(-b, b, (F, F))), b0=f(r.uniform(-b, b, F)), W3=f(r.uniform(-b, b, (C, F))), b3=f(r.uniform(-b, b, C)))
    P["labels"], P["weight"] = _labels_weight(r, N, C, weighted)
    x = P["H2"].astype(np.float64)
    var = x.var(0) if N > 1 else np.ones(F)
    P["saved"] = f(np.concatenate([x.mean(0), 1.0 / np.sqrt(var + EPS)]))
    return P


def exact_inputs(N, F, C, weighted, seed):
    """every product and partial sum up to the logits is exact in fp32 in any order (asserted on the float64 result by
    `assert_exact`); classes 0 and 1 share their W3 row and bias, so every row in which they are maximal ties"""
    r = np.random.RandomState(seed)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    ri = lambda lo, hi, *s: r.randint(lo, hi + 1, s)
    P = dict(H2=f(ri(-4, 4, N, F)), gamma=f(r.choice([-2, -1, 1, 2], F)), beta=f(ri(-2, 2, F)), slope=0.25,
             W0=f(ri(-2, 2, F, F)), b0=f(ri(-3, 3, F)), W3=f(ri(-3, 3, C, F) * 2.0 ** -10), b3=f(ri(-8, 8, C) * 2.0 ** -4),
             saved=f(np.concatenate([ri(-2, 2, F), r.choice([0.5, 1.0, 2.0], F)])))
    if C > 1:      # (non-negative weights on Z >= 0: the shared score is the maximum of most rows)
        P["W3"][0], P["b3"][0] = np.abs(P["W3"][0]), P["b3"].max()
        P["W3"][1], P["b3"][1] = P["W3"][0], P["b3"][0]
    P["labels"], P["weight"] = _labels_weight(r, N, C, weighted)
    if weighted:
        P["weight"] = f(r.choice([0.5, 1.0, 2.0, 4.0], C))
    return P


EXACT_EPS = 0.25      # exact inputs through erc_head_fused_bn: var + eps in {4, 1, 0.25} gives rstd in {0.5, 1, 2}


def exact_bn_part(saved, n, n_tiles):
    """float32 tile sums that finalise (eps = EXACT_EPS) to exactly ``saved`` = integer mean | rstd in {0.5, 1, 2}: tile t of r_t
    rows holds r_t mean | r_t (var + mean^2), var = 1 / rstd^2 - eps.  Every entry and every partial sum is a multiple of
    0.25 below 2^24, so the float64 sums, sx / n and sxx / n are exact"""
    F = saved.shape[0] // 2
    mean, rstd = saved[:F].astype(np.float64), saved[F:].astype(np.float64)
    var = 1.0 / (rstd * rstd) - EXACT_EPS
    out = np.zeros((n_tiles, 2 * F), np.float32)
    for t in range(-(-n // 16)):
        rows = min(16, n - 16 * t)
        out[t, :F], out[t, F:] = rows * mean, rows * (var + mean * mean)
    return out


def place_ties(P, out):
    """give tied rows the lower index (a hit) and the higher index (a miss) as label, two to one, and then make sure that taking
    the LAST maximal index would count differently; needs the float64 result.  Returns the number of tied rows"""
    lg = out["logits"]
    if lg.shape[1] < 2:
        return 0
    tied = np.flatnonzero((lg[:, 0] == lg[:, 1]) & (lg[:, 0] == lg.max(1)))
    for k, row in enumerate(tied[:3]):
        P["labels"][row] = (0, 1, 0)[k]
    for row in tied[3:]:      # first-index hits are the tied rows labelled 0, last-index hits those labelled 1
        if (P["labels"][tied] == 0).sum() != (P["labels"][tied] == 1).sum():
            break
        P["labels"][row] = 0
    assert len(tied) < 3 or (P["labels"][tied] == 0).sum() != (P["labels"][tied] == 1).sum()
    return len(tied)


def assert_exact(P, out):
    """the precondition of the bit-for-bit comparisons: sum |terms| of every product, in units of its smallest bit, is below 2^24"""
    a = lambda k: np.abs(np.asarray(P[k], np.float64))
    assert float((np.abs(out["H3"]) @ a("W0").T + a("b0")).max()) / 0.125 < 2 ** 24
    assert float((np.abs(out["Z"]) @ a("W3").T + a("b3")).max()) / 2.0 ** -13 < 2 ** 24
    for k in ("H3", "Z", "logits"):
        assert np.array_equal(out[k].astype(np.float32).astype(np.float64), out[k]), k


# ------------------------------------------------------------------------------------------------- the case table
def _c(name, form, N, F, C, pad, w, p, out, ldb16, lddl, lr, nd, env=None):
    return dict(name=name, form=form, N=N, F=F, C=C, ldh=F + pad, weighted=bool(w), p=p, out=out, ldb16=ldb16, lddl=lddl,
                label_rows=bool(lr), n_dev=nd, env=env)


# form: A head_fused <false,1> | B head_fused rows kernel | C head_fused_bn <true,1> | D head_fused_bn <true,2> | E head_fused
# <false,2> (a child process with env).  n_dev: None, or the count on the device.  out: fp32 only | both | bf16 only.
CASES = [
    _c("A-n1", "A", 1, 100, 6, 0, 0, 0.0, "f32", 0, 0, 0, None),
    _c("A-n15", "A", 15, 96, 7, 12, 1, 0.5, "both", 104, 8, 1, None),
    _c("A-n16-nd16", "A", 16, 36, 8, 0, 1, 0.0, "bf16", 112, 0, 0, 16),
    _c("A-n17-nd16", "A", 17, 4, 1, 12, 0, 0.5, "both", 112, 8, 1, 16),
    _c("A-n17-nd1", "A", 17, 96, 6, 0, 1, 0.0, "f32", 0, 0, 0, 1),
    _c("A-n33-nd15", "A", 33, 100, 8, 0, 1, 0.0, "f32", 0, 0, 0, 15),
    _c("A-n37-nd36", "A", 37, 36, 6, 12, 0, 0.5, "bf16", 104, 8, 1, 36),
    _c("A-n1025", "A", 1025, 100, 7, 0, 1, 0.5, "both", 112, 0, 0, None),
    _c("B-n8193", "B", 8193, 100, 6, 0, 1, 0.5, "f32", 0, 0, 0, None),
    _c("B-n8209-nd8193", "B", 8209, 96, 7, 12, 0, 0.0, "both", 104, 8, 1, 8193),
    _c("B-n8209-nd8208", "B", 8209, 36, 1, 0, 1, 0.5, "bf16", 112, 0, 0, 8208),
    _c("B-n8193-nd1", "B", 8193, 4, 8, 12, 0, 0.0, "f32", 0, 8, 1, 1),
    _c("B-n32801-nd32801", "B", 32801, 100, 8, 0, 1, 0.5, "both", 112, 0, 0, 32801),
    _c("C-n1", "C", 1, 36, 1, 0, 0, 0.0, "f32", 0, 0, 0, None),
    _c("C-n17-nd17", "C", 17, 100, 7, 12, 1, 0.5, "both", 104, 8, 1, 17),
    _c("C-n33-nd32", "C", 33, 96, 6, 0, 0, 0.0, "bf16", 112, 0, 0, 32),
    _c("C-n37-nd15", "C", 37, 4, 8, 12, 1, 0.5, "f32", 0, 8, 1, 15),
    _c("C-n1025-nd1", "C", 1025, 100, 6, 0, 1, 0.5, "both", 112, 0, 0, 1),
    _c("D-n8193", "D", 8193, 100, 7, 12, 1, 0.5, "both", 104, 8, 1, None),
    _c("D-n8209-nd8200", "D", 8209, 96, 6, 0, 0, 0.0, "f32", 0, 0, 0, 8200),
    _c("D-n8209-nd8208", "D", 8209, 36, 8, 0, 1, 0.0, "bf16", 112, 0, 0, 8208),
    _c("D-n8193-nd1", "D", 8193, 4, 1, 12, 0, 0.5, "f32", 0, 8, 1, 1),
    _c("D-n8193-nd8193", "D", 8193, 100, 6, 0, 1, 0.5, "f32", 0, 0, 0, 8193),
    _c("E-rows32-n17", "E", 17, 36, 7, 12, 1, 0.5, "both", 104, 8, 1, None, env=("ERC_HEAD_ROWS", "32")),
    _c("E-rows32-n33-nd17", "E", 33, 100, 8, 0, 0, 0.0, "bf16", 112, 0, 0, 17, env=("ERC_HEAD_ROWS", "32")),
    _c("E-rows32-n15-nd15", "E", 15, 4, 1, 0, 1, 0.5, "f32", 0, 0, 0, 15, env=("ERC_HEAD_ROWS", "32")),
    _c("E-wave0-n8209-nd8208", "E", 8209, 100, 6, 12, 1, 0.5, "both", 112, 8, 1, 8208, env=("ERC_HEAD_WAVE", "0")),
    _c("E-wave0-n8193-nd1", "E", 8193, 96, 7, 0, 0, 0.0, "f32", 0, 0, 0, 1, env=("ERC_HEAD_WAVE", "0")),
]
CASE = {c["name"]: c for c in CASES}


def case_rows(c):
    """the number of rows a case's launch works on"""
    return c["N"] if c["n_dev"] is None else max(1, min(c["n_dev"], c["N"]))


def case_seed(c):
    return 1000 + CASES.index(c)


@functools.lru_cache(maxsize=None)
def case_reference(name, kind):
    """inputs (float32), the dropout mask and the float64 result of a case on its live rows; computed once, never changed.
    kind = 'exact' | 'random'.  Forms C and D take ``saved`` from bn_finalize of the tile sums (random) or from tile sums built
    to finalise to it (exact), so the same reference serves every form."""
    c = CASE[name]
    n, F, C = case_rows(c), c["F"], c["C"]
    P = (exact_inputs if kind == "exact" else random_inputs)(n, F, C, c["weighted"], case_seed(c))
    rm0 = np.zeros(F, np.float32) + np.float32(0.05)
    rv0 = np.ones(F, np.float32)
    P["rm0"], P["rv0"] = rm0, rv0
    tiles_cap = -(-c["N"] // 16)
    if c["form"] in "CD":
        if kind == "exact":
            P["eps"] = EXACT_EPS
            P["bn_part"] = exact_bn_part(P["saved"], n, tiles_cap)
        else:
            P["eps"] = EPS
            P["bn_part"] = bn_tile_sums(P["H2"], tiles_cap)
        P["bn"] = bn_finalize(P["bn_part"], n, P["eps"], MOMENTUM, rm0, rv0)
        P["saved"] = P["bn"]["saved"].astype(np.float32)
    k = keep(RNG[1], RNG[0], n, F, c["p"])
    args = lambda: (P["H2"], P["saved"], P["gamma"], P["beta"], P["slope"], P["W0"], P["b0"], P["W3"], P["b3"], P["labels"], P["weight"], k)
    out = head(*args())
    ties = 0
    if kind == "exact":
        ties = place_ties(P, out)
        out = head(*args())
        assert_exact(P, out)
        assert ties >= 3 or n < 3 or C < 2, (name, ties)
    return dict(P=P, keep=k, out=out, args=args(), ties=ties)


def f32_figures(name, kind="random"):
    """err / scale of the float32 twin against float64 per output group (fragile rows left out of dZ and dY)"""
    ref = case_reference(name, kind)
    P, out = ref["P"], ref["out"]
    tw = head_f32(*ref["args"])
    ok = ~fragile_rows(out, P["W0"], P["b0"], P["gamma"], P["beta"]) if kind == "random" else np.ones(out["N"], bool)
    return figures(tw, out, ok)


def figures(got, out, ok):
    """{group: max |got - ref| / max |ref|}; ``got`` holds arrays of any float dtype under the reference's keys"""
    fig = {}
    for k in ("H3", "Z", "logits", "dlogits", "dZ", "dY"):
        rows = ok if k in ("dZ", "dY") else slice(None)
        fig[k] = _rel(np.asarray(got[k], np.float64)[rows], out[k][rows])
    if "bn_bwd" in got:
        fig["bn"] = max(_rel(got[k], out[k]) for k in ("bn_bwd", "dgamma", "dbeta"))
    if "stats" in got:
        fig["loss"] = abs(float(got["stats"][0]) - out["stats"][0]) / max(abs(out["stats"][0]), 1e-30)
    return fig


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if b.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))


# worst err / scale of the float32 twin over CASES per kind of input, measured from the restatements alone
F32_WORST = dict(
    random=dict(H3=1.30e-7, Z=5.31e-7, logits=5.41e-7, dlogits=1.78e-7, dZ=2.32e-7, dY=2.97e-7, bn=3.51e-6, loss=9.49e-8),
    exact=dict(H3=0.0, Z=0.0, logits=0.0, dlogits=3.46e-7, dZ=8.84e-6, dY=1.29e-5, bn=1.64e-5, loss=4.00e-7))


def _one_digit_up(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


BOUND = {kind: {k: (_one_digit_up(4 * v) if v > 0 else 0.0) for k, v in w.items()} for kind, w in F32_WORST.items()}


# ------------------------------------------------------------------------------------------------- what a launch is held to
def bf16_bits(a):
    """round-to-nearest-even bf16 of a float32 array, as int16 bit patterns"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).view(torch.int16).numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def untouched(a):
    """every element still holds its prefill (NaN for float32, 0x7FC0 for the bf16 bit patterns)"""
    return bool(np.isnan(a).all()) if a.dtype == np.float32 else bool((a == NAN16).all())


def uses_rows_kernel(c, n_rows, bn):
    return (not bn) and n_rows > 8192 and c["env"] != ("ERC_HEAD_WAVE", "0")


def rows_per_workgroup(c, n_rows):
    if c["env"] == ("ERC_HEAD_ROWS", "32"):
        return 32
    return 16 if n_rows <= 8192 else 32


def groups_of(c, n_rows, n, bn):
    """the rows of every workgroup record of the launch: (list of row index arrays, one per workgroup of the grid)"""
    if uses_rows_kernel(c, n_rows, bn):
        return rows_kernel_groups(n_rows, n)
    rpw = rows_per_workgroup(c, n_rows)
    g = row_groups(n, rpw)
    return g + [np.arange(0)] * (-(-n_rows // rpw) - len(g))


def check_outputs(c, kind, ref, got, n_rows, n, out_mode, defer):
    """everything one launch wrote against the float64 result ``ref`` of its n live rows"""
    P, out, F, C = ref["P"], ref["out"], c["F"], c["C"]
    tag = (c["name"], kind, out_mode, defer)
    bn = c["form"] in "CD"
    f32o = out_mode != "bf16"
    # ---- the prefill: rows at or beyond the count, pad columns
    for k in ("H3", "Z", "dZ", "dlogits", "logits", "dY", "H3b", "Zb", "dZb", "dlb"):
        if k not in got:
            continue
        live = f32o or k in ("logits", "dY", "H3b", "Zb", "dZb", "dlb")
        width = dict(dlogits=C, logits=C, dlb=C).get(k, F)
        assert untouched(got[k][n:]), (tag, k, "rows beyond the count")
        assert untouched(got[k][:, width:]), (tag, k, "pad columns")
        if live:
            a = got[k][:n, :width]
            assert not (np.isnan(a).any() if a.dtype == np.float32 else (a == NAN16).any()), (tag, k, "unwritten or NaN")
        else:
            assert untouched(got[k]), (tag, k, "fp32 output written although its pointer was NULL")
    assert np.isnan(got["stats"][3])
    # ---- bf16 copies: bit for bit the rounding of the fp32 outputs of the same launch
    if out_mode == "both":
        for k16, k32, width in (("H3b", "H3", F), ("Zb", "Z", F), ("dZb", "dZ", F), ("dlb", "dlogits", C)):
            assert same_bits(got[k16][:n, :width], bf16_bits(got[k32][:n, :width])), (tag, k16)
    # ---- BatchNorm statistics finalised in the launch (forms C, D)
    if bn:
        want = P["bn"]
        assert np.all(np.abs(got["saved"] - want["saved"]) <= 2 * U * np.abs(want["saved"])), (tag, "saved")
        assert np.all(np.abs(got["rm"] - want["running_mean"]) <= 2 * U * want["scale_mean"]), (tag, "running_mean")
        assert np.all(np.abs(got["rv"] - want["running_var"]) <= 2 * U * np.abs(want["running_var"])), (tag, "running_var")
        if kind == "exact":
            assert same_bits(got["saved"], P["saved"]), (tag, "saved")
    # ---- the records: one per workgroup, over that workgroup's rows; link 1 on the kernel's own dY
    groups = groups_of(c, n_rows, n, bn)
    G = len(groups)
    rec = got["ws"][:G * PART].reshape(G, PART).astype(np.float64)
    dY_own = got["dY"][:n, :F]
    want = records(out, groups, dY=dY_own)
    lim = 32 * U * record_abs(out, groups, dY_own)
    err = np.abs(rec[:, :224] - want[:, :224])
    assert np.all(err <= lim[:, :224]), (tag, "record sums", float((err / np.maximum(lim[:, :224], 1e-300)).max()))
    rec_ratio = float((err / np.maximum(lim[:, :224], 1e-300)).max())
    assert np.all(np.abs(rec[:, 226] - out["wsum"]) <= 2 * U * out["wsum"]), (tag, "record weight sum")
    assert np.all(rec[:, 227] == 0), (tag, "record pad")
    ref_rec = records(out, groups)
    close = close_rows(out) if kind == "random" else np.zeros(n, bool)
    close_per = np.array([int(close[g].sum()) for g in groups])
    assert np.all(np.abs(rec[:, 225] - ref_rec[:, 225]) <= close_per), (tag, "record hits")
    loss_rec = rec[:, 224].sum() / out["wsum"]
    bound = BOUND[kind]
    fig = dict(loss=abs(loss_rec - out["stats"][0]) / max(abs(out["stats"][0]), 1e-30))
    # ---- element-wise outputs
    ok = np.ones(n, bool)
    if kind == "random":
        ok = ~fragile_rows(out, P["W0"], P["b0"], P["gamma"], P["beta"])
    g = {k: got[k][:n, :(C if k in ("logits", "dlogits") else F)] for k in ("H3", "Z", "logits", "dlogits", "dZ", "dY") if f32o or k in ("logits", "dY")}
    for k in g:
        rows = ok if k in ("dZ", "dY") else slice(None)
        fig[k] = _rel(g[k][rows], out[k][rows])
    if kind == "exact":
        for k in ("H3", "Z", "logits"):
            if k in g:
                assert same_bits(g[k] + np.float32(0), (out[k] + 0.0).astype(np.float32)), (tag, k, "not bit-equal to float64")
    if "Z" in g:      # the dropout mask, wherever the float64 pre-activation is safely positive
        sure = (out["pre"] > 0) & ok[:, None]
        assert np.array_equal((g["Z"] != 0)[sure], (ref["keep"] != 0)[sure]), (tag, "dropout mask")
    # ---- reduced outputs
    if defer:
        for k in ("bn_bwd", "dgamma", "dbeta"):
            assert untouched(got[k]), (tag, k, "written by a deferred launch")
        assert untouched(got["stats"]), (tag, "stats written by a deferred launch")
    else:
        lim_sum = lim[:, :224].sum(0)
        for k, lo, half in (("dbeta", 0, 0), ("dgamma", 112, F)):      # record slots [lo, lo + F), bn_bwd[half, half + F)
            w_ = want[:, lo:lo + F].sum(0)
            tol = lim_sum[lo:lo + F] + 2 * U * np.abs(w_)
            assert np.all(np.abs(got[k] - w_) <= tol), (tag, k)
            assert np.all(np.abs(got["bn_bwd"][half:half + F] - w_ / n) <= tol / n), (tag, "bn_bwd")
        st = got["stats"].astype(np.float64)
        assert abs(st[0] - loss_rec) <= 2 * U * abs(loss_rec), (tag, "stats[0] is not the records' loss")
        assert st[1] == rec[:, 225].sum() and abs(st[1] - out["stats"][1]) <= int(close.sum()), (tag, "#correct", st[1], out["stats"][1])
        assert abs(st[2] - out["wsum"]) <= 2 * U * out["wsum"], (tag, "stats[2]")
        if kind == "exact":      # the sums end to end: no decision can differ
            assert st[1] == out["stats"][1], (tag, "#correct, ties included")
            fig["bn"] = max(_rel(got[k], out[k]) for k in ("bn_bwd", "dgamma", "dbeta"))
    print("head %-22s %-6s %-4s defer=%d rows=%d fragile=%.4f close=%.4f record/limit=%.3f " % (c["name"], kind, out_mode, defer, n, 1 - ok.mean(), close.mean(), rec_ratio)
          + " ".join("%s=%.2e" % (k, fig[k]) for k in GROUPS if k in fig))
    for k, v in fig.items():
        assert v <= bound[k], (tag, k, v, bound[k])
    return rec
