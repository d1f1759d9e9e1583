"""MMGCN's small operators (csrc/mmgcn_ops.hip) called directly, each against float64 on the CPU: the adjacency's forward and
backward as the module chains them, the cross-modal entries, the node tables, the speaker-embedding gradient, and the
elementwise / dropout kernels.

Bounds.  Forward adjacency: the golden test's (atol 2e-5, rtol 1e-4).  Everything else that is a sum of fp32 products is held to
rel_err <= max(4 x the rel_err of the SAME computation run in float32 on the CPU, FLOOR): d sim / d cos = 0.99999 / (pi sqrt(1 -
t^2)) at t = 0.99999 cos close to 1 (every diagonal entry; duplicate rows) amplifies the fp32 rounding of the cosine by 1 / (1 - t^2)
~ 5e4 in ANY fp32 implementation, so only another fp32 implementation says what fp32 can deliver there.  FLOOR restates the bound of
test_gpu_ops.py's exact-fp32 GEMM comparisons (atol 2e-4 sqrt(K / 100) on results of rms sqrt(K): 2e-5 of the result's rms for
every K) on rel_err's scale, the reference's largest entry >= its rms.  Elementwise kernels are exact or within a rounding."""
import math

import numpy as np
import pytest
import torch

from tests.util_cases import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FD, MAXP, SHRINK = 200, 128, 0.99999
FLOOR = 2e-5
BIG = 2048 * 256 + 3          # one past the elementwise grid cap (2048 workgroups of 256): the grid-stride loop runs


@pytest.fixture(scope="module")
def capi():
    from erc_amd import capi as c
    c.lib()
    return c


def _tables(lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    dlg = np.concatenate([np.full(L, b, dtype=np.int32) for b, L in enumerate(lens)])
    return torch.from_numpy(off), torch.from_numpy(dlg)


# ----------------------------------------------------------------------------- adjacency
ADJ_CASES = {"one": (1,), "stride": (1, 5, 64, 65), "maxp": (128, 3), "hard": (7, 7)}


def _adj_inputs(name, M):
    lens = ADJ_CASES[name]
    N = sum(lens)
    g = torch.Generator().manual_seed(100 * M + len(lens) + N)
    X = torch.randn(M * N, FD, generator=g) * (0.5 + 1.5 * torch.rand(M * N, 1, generator=g))
    if name == "hard":
        X[1] = X[0]                                                         # duplicate row in (modality 0, dialogue 0): cos = 1
        X[3] = X[2] * (1 + 1e-2 * torch.randn(FD, generator=g))             # near duplicate
        X[5] = -X[4]                                                        # antiparallel: cos = -1, sim = 0.0014 > 0
        X[N + 7 + 2] = X[7 + 2]                                             # utterance 2 of dialogue 1: modalities 0 and 1 alike
    T = max(lens)
    P = (T + 3) // 4 * 4
    B = len(lens)
    dADJ, dCR = torch.randn(B * M, P, P, generator=g), torch.randn(B, M * M, P, generator=g)
    valid = torch.zeros(B, P, dtype=torch.bool)
    for b, L in enumerate(lens):
        valid[b, :L] = True
    vb = valid.repeat_interleave(M, 0)
    vadj = vb[:, :, None] & vb[:, None, :]
    vcr = valid[:, None, :] & ~torch.eye(M, dtype=torch.bool).reshape(1, M * M, 1)
    dX0 = torch.randn(M * N, FD, generator=g)
    return dict(lens=lens, M=M, N=N, B=B, T=T, P=P, X=X, dADJ=dADJ * vadj, dCR=dCR * vcr, vadj=vadj, vcr=vcr, dX0=dX0)


def _adj_restated(c, dtype):
    """row normalisation -> cosine blocks -> arccos similarity -> degrees -> D^-1/2 . D^-1/2, on the kernels' block layout, with
    autograd on sum(ADJ dADJ) + sum(CR dCR): DEG, G = dCOS + dCOS^T, GC (both directions of a pair summed), dX."""
    lens, M, N, P, B = c["lens"], c["M"], c["N"], c["P"], c["B"]
    x = c["X"].to(dtype).clone().requires_grad_()
    xh = x / torch.sqrt((x * x).sum(1, keepdim=True))
    COS, CCOS = [], []
    off = 0
    for L in lens:
        rows = [xh[m * N + off:m * N + off + L] for m in range(M)]
        for m in range(M):
            COS.append(torch.nn.functional.pad(rows[m] @ rows[m].t(), (0, P - L, 0, P - L)))
            for n in range(M):
                CCOS.append(torch.nn.functional.pad((rows[m] * rows[n]).sum(1), (0, P - L)))
        off += L
    COS, CCOS = torch.stack(COS), torch.stack(CCOS).reshape(B, M * M, P)
    COS.retain_grad(), CCOS.retain_grad()
    sim = lambda t: 1 - torch.acos(t * SHRINK) / math.pi
    S = sim(COS) * c["vadj"].to(dtype)
    SC = sim(CCOS) * c["vcr"].to(dtype)
    deg = S.sum(2).reshape(B, M, P) + SC.reshape(B, M, M, P).sum(2)           # [B, M, P]; 0 on the pads
    deg.retain_grad()
    u = torch.where(deg > 0, deg, torch.ones_like(deg)) ** -0.5
    ub = u.reshape(B * M, P)
    ADJ = S * ub[:, :, None] * ub[:, None, :]
    CR = SC * (u[:, :, None, :] * u[:, None, :, :]).reshape(B, M * M, P)
    ((ADJ * c["dADJ"].to(dtype)).sum() + (CR * c["dCR"].to(dtype)).sum()).backward()
    gc = CCOS.grad.reshape(B, M, M, P)
    DEG = torch.zeros(M * N, dtype=dtype)
    off = 0
    for b, L in enumerate(lens):
        for m in range(M):
            DEG[m * N + off:m * N + off + L] = deg.detach()[b, m, :L]
        off += L
    return dict(ADJ=ADJ.detach(), CR=CR.detach(), DEG=DEG, G=COS.grad + COS.grad.transpose(1, 2),
                GC=(gc + gc.transpose(1, 2)).reshape(B, M * M, P), dX=x.grad + c["dX0"].to(dtype))


def _adj_oracle(c):
    """the stated reference: tests.mmgcn_chain_ref.build_adjacency (oracle.mmgcn.big_adjacency) in float64, autograd"""
    from tests.mmgcn_chain_ref import build_adjacency
    M, N = c["M"], c["N"]
    x = c["X"].double().requires_grad_()
    off, _ = _tables(c["lens"])
    ADJ, CR = build_adjacency([x[m * N:(m + 1) * N] for m in range(M)], off, c["P"])
    ((ADJ * c["dADJ"].double()).sum() + (CR * c["dCR"].double()).sum()).backward()
    return ADJ.detach(), CR.detach(), x.grad + c["dX0"].double()


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("name", list(ADJ_CASES))
def test_adjacency_forward_and_backward_match_float64(capi, name, M):
    """mm_row_normalize -> gemm_grouped(1) -> mm_adj_finish, and mm_adj_finish_bwd -> gemm_grouped(0) -> mm_cross_apply ->
    mm_row_normalize_bwd into a pre-filled dX, on: one single-utterance dialogue; lengths around the 64-lane stride under P = 68;
    P = 128; duplicate, near-duplicate and antiparallel rows and an utterance whose modalities coincide.  The pads of COS, dADJ and
    dCR hold NaN during the backward: nothing the module reads afterwards may depend on them.
    Measured (MI355X), rel_err | float32 CPU yardstick: DEG <= 1.7e-06 | 4e-07 .. 8.5e-06; G <= 1.1e-06 (hard: 9.3e-05) | 3.5e-03 ..
    1.1e-02; GC <= 7.2e-07 (hard: 7.5e-06) | 6e-07 .. 5.4e-03; dX <= 3.3e-07 | 3e-08 .. 8e-08 (its bound is FLOOR); ADJ, CR <= 1.1e-06
    absolute.  With `1.0f - t * t` in dsim_dc and cosines taken as the GEMM and the dot product left them (|xhat|^2 = 1 +- 5e-7),
    GC of the hard M = 3 case was 5.3e-03 against a bound of 2.7e-03, G up to 2.5e-02 (bound 2.6e-02), DEG up to 2.2e-05 (bound
    2.5e-05): csrc/mmgcn_ops.hip now renormalises the cosines by their own norms and forms 1 - t^2 without cancellation."""
    c = _adj_inputs(name, M)
    lens, N, B, T, P = c["lens"], c["N"], c["B"], c["T"], c["P"]
    assert N <= 330 and P <= MAXP
    want = _adj_restated(c, torch.float64)
    o_adj, o_cr, o_dx = _adj_oracle(c)
    for k, o in (("ADJ", o_adj), ("CR", o_cr), ("dX", o_dx)):                   # the restatement IS the oracle's adjacency
        assert bool(torch.isfinite(o).all()) and rel_err(want[k], o, floor=0) < 1e-9, k
    assert bool(torch.isfinite(want["G"]).all()) and float(want["DEG"].min()) > 0
    yard = _adj_restated(c, torch.float32)

    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    R3 = M * N
    off, dlg = _tables(lens)
    off, dlg = off.to(DEV), dlg.to(DEV)
    X, XH, INV = c["X"].to(DEV), f32(R3, FD), f32(R3)
    COS, ADJ, CR, CCOS, DEG = f32(B * M, P, P), f32(B * M, P, P), f32(B, M * M, P), f32(B, M * M, P), f32(R3)
    capi.mm_row_normalize(X, R3, XH, INV)
    capi.gemm_grouped(1, XH, FD, XH, FD, COS, P, FD, off, B, M, N, T, P)
    capi.mm_adj_finish(COS, XH, off, B, M, N, P, ADJ, CR, CCOS, DEG)
    vadj, vcr = c["vadj"].to(DEV), c["vcr"].to(DEV)
    nan = torch.tensor(float("nan"), device=DEV)
    COS = torch.where(vadj, COS, nan)
    dADJ, dCR = torch.where(vadj, c["dADJ"].to(DEV), nan), torch.where(vcr, c["dCR"].to(DEV), nan)
    Gb, GC, DDEG, dXH, dX = f32(B * M, P, P), f32(B, M * M, P), f32(R3), f32(R3, FD), c["dX0"].to(DEV).clone()
    capi.mm_adj_finish_bwd(COS, CCOS, DEG, dADJ, dCR, off, B, M, N, P, Gb, GC, DDEG)
    capi.gemm_grouped(0, Gb, P, XH, FD, dXH, FD, FD, off, B, M, N, T, P)
    capi.mm_cross_apply(GC, XH, FD, dlg, off, M, N, P, dXH, FD)
    capi.mm_row_normalize_bwd(XH, INV, dXH, R3, dX)
    torch.cuda.synchronize()

    got = dict(ADJ=ADJ.cpu() * c["vadj"], CR=CR.cpu() * c["vcr"], DEG=DEG.cpu(), G=Gb.cpu(), GC=GC.cpu(), dX=dX.cpu())
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    assert bool(torch.isfinite(DDEG).all()) and bool(torch.isfinite(dXH).all())
    assert float(Gb.cpu()[~c["vadj"]].abs().max() if (~c["vadj"]).any() else 0.0) == 0.0, "G written outside the dialogue"
    np.testing.assert_allclose(got["ADJ"].numpy(), o_adj.numpy(), atol=2e-5, rtol=1e-4)
    np.testing.assert_allclose(got["CR"].numpy(), o_cr.numpy(), atol=2e-5, rtol=1e-4)
    line, bad = [], []
    for k in ("DEG", "G", "GC", "dX"):
        ref = o_dx if k == "dX" else want[k]
        e, y = rel_err(got[k], ref), rel_err(yard[k], ref)
        bound = max(4 * y, FLOOR)
        line.append("%s=%.2e (float32 cpu %.2e, bound %.2e)" % (k, e, y, bound))
        if not e <= bound:
            bad.append(k)
    print("mmgcn-ops adjacency %s M=%d ADJ=%.2e CR=%.2e %s" % (name, M, float((got["ADJ"] - o_adj).abs().max()),
                                                                float((got["CR"] - o_cr).abs().max()), " ".join(line)))
    assert not bad, (bad, line)


@pytest.mark.parametrize("which", ["M1", "M4", "P132"])
def test_adj_finish_rejects_unsupported_sizes(capi, which):
    """M outside 2..3 and P above 128 raise before any launch"""
    M, P = dict(M1=(1, 8), M4=(4, 8), P132=(3, 132))[which]
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    off = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    blk, cr, row = z(4, 132, 132), z(1, 16, 132), z(4 * 5, FD)
    with pytest.raises(capi.ErcGraftError, match="mm_adj_finish"):
        capi.mm_adj_finish(blk, row, off, 1, M, 5, P, z(4, 132, 132), z(1, 16, 132), z(1, 16, 132), z(20))
    with pytest.raises(capi.ErcGraftError, match="mm_adj_finish_bwd"):
        capi.mm_adj_finish_bwd(blk, cr, z(20), blk, cr, off, 1, M, 5, P, z(4, 132, 132), z(1, 16, 132), z(20))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- cross-modal entries
@pytest.mark.parametrize("layout", ["planes_apart", "planes_in_row"])
@pytest.mark.parametrize("planes", [1, 5, 64])
@pytest.mark.parametrize("M", [2, 3])
def test_cross_grad_matches_float64(capi, M, planes, layout):
    """dCR[b][m M + n][p] += sum over planes of dhi[(m, p)] . h[(n, p)]: 1, 5 and 64 planes (the 4-plane unroll with its clamped
    tail), plane stride R3 * 200 at pitch 200 (per-layer form) and plane stride 200 at pitch 64 * 200 (chain form); added to a
    non-zero dCR, whose pads and m == n rows stay as they were"""
    lens = (9, 1, 23)
    N, B, P = sum(lens), len(lens), 24
    R3 = M * N
    g = torch.Generator().manual_seed(planes + 10 * M)
    if layout == "planes_apart":
        d, h = torch.randn(planes, R3, FD, generator=g), torch.randn(planes, R3, FD, generator=g)
        ld, plane = FD, R3 * FD
        dv, hv = d, h
    else:
        d, h = torch.randn(R3, 64 * FD, generator=g), torch.randn(R3, 64 * FD, generator=g)
        ld, plane = 64 * FD, FD
        dv, hv = (t.reshape(R3, 64, FD)[:, :planes].permute(1, 0, 2) for t in (d, h))
    dCR0 = torch.randn(B, M * M, P, generator=g)
    want = dCR0.double().clone()
    prod = torch.einsum("lmic,lnic->mni", dv.double().reshape(planes, M, N, FD), hv.double().reshape(planes, M, N, FD))
    o = 0
    for b, L in enumerate(lens):
        for m in range(M):
            for n in range(M):
                if n != m:
                    want[b, m * M + n, :L] += prod[m, n, o:o + L]
        o += L
    off, dlg = _tables(lens)
    dCR = dCR0.to(DEV)
    capi.mm_cross_grad(d.to(DEV), ld, h.to(DEV), ld, dlg.to(DEV), off.to(DEV), M, N, P, dCR, planes=planes, d_plane=plane,
                       h_plane=plane)
    got = dCR.cpu()
    same = want == dCR0.double()
    assert torch.equal(got[same], dCR0[same])
    e = rel_err(got, want)
    print("mmgcn-ops cross_grad M=%d planes=%d %s rel_err=%.2e (bound %.0e)" % (M, planes, layout, e, FLOOR))
    assert e <= FLOOR


@pytest.mark.parametrize("M", [2, 3])
def test_cross_apply_accumulates_at_wide_pitches(capi, M):
    """out[(m, p), :200] += sum_{n != m} CR[b][m M + n][p] h[(n, p), :200] with ldh = 208, ldo = 256 into a non-zero out; the
    columns past 200 stay"""
    lens = (9, 1, 23)
    N, B, P, ldh, ldo = sum(lens), len(lens), 24, 208, 256
    g = torch.Generator().manual_seed(7 + M)
    CR, h, out0 = torch.randn(B, M * M, P, generator=g), torch.randn(M * N, ldh, generator=g), torch.randn(M * N, ldo, generator=g)
    want = out0.double().clone()
    o = 0
    for b, L in enumerate(lens):
        for m in range(M):
            for n in range(M):
                if n != m:
                    want[m * N + o:m * N + o + L, :FD] += CR[b, m * M + n, :L, None].double() * h[n * N + o:n * N + o + L, :FD].double()
        o += L
    off, dlg = _tables(lens)
    out = out0.to(DEV)
    capi.mm_cross_apply(CR.to(DEV), h.to(DEV), ldh, dlg.to(DEV), off.to(DEV), M, N, P, out, ldo)
    got = out.cpu()
    assert torch.equal(got[:, FD:], out0[:, FD:])
    e = rel_err(got[:, :FD], want[:, :FD])
    print("mmgcn-ops cross_apply M=%d rel_err=%.2e (bound %.0e)" % (M, e, FLOOR))
    assert e <= FLOOR


# ----------------------------------------------------------------------------- node tables, flatten, embedding gradient
@pytest.mark.parametrize("S", [2, 9])
@pytest.mark.parametrize("B", [1, 5, 32])
def test_meta_tables_match_a_python_loop(capi, B, S):
    g = torch.Generator().manual_seed(B * 10 + S)
    T = 12
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    big = torch.rand(T, B + 2, S + 3, generator=g).to(DEV)
    qmask = big[:, 1:B + 1, 2:2 + S]                                      # a slice: strides (B + 2)(S + 3), S + 3, 1
    assert not qmask.is_contiguous() and qmask.stride(2) == 1
    N = int(lens.sum())
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=DEV)
    off, row, dlg, spk = i32(B + 1), i32(N + 1), i32(N + 1), i32(N + 1)
    capi.mm_meta(lens.to(DEV), qmask, qmask.stride(0), qmask.stride(1), S, B, off, row, dlg, spk)
    q = qmask.cpu()
    w_off, w_row, w_dlg, w_spk = [0], [], [], []
    for b in range(B):
        for t in range(int(lens[b])):
            w_row.append(t * B + b), w_dlg.append(b), w_spk.append(int(torch.argmax(q[t, b])))
        w_off.append(len(w_row))
    assert off.cpu().tolist() == w_off and int(off[B]) == N
    assert row.cpu().tolist() == w_row + [-7] and dlg.cpu().tolist() == w_dlg + [-7] and spk.cpu().tolist() == w_spk + [-7]


@pytest.mark.parametrize("with_emb", [False, True])
def test_flatten_gathers_rows_and_adds_the_speaker_embedding(capi, with_emb):
    g = torch.Generator().manual_seed(3)
    N, rows, lds, ldd, S = 33, 50, 208, 256, 9
    src, emb = torch.randn(rows, lds, generator=g), torch.randn(S, FD, generator=g)
    row_map = torch.randperm(rows, generator=g)[:N].to(torch.int32)
    spk = torch.randint(0, S, (N,), generator=g).to(torch.int32)
    dst0 = torch.randn(N + 1, ldd, generator=g)
    dst = dst0.to(DEV)
    capi.mm_flatten(src.to(DEV), lds, row_map.to(DEV), emb.to(DEV) if with_emb else None, spk.to(DEV) if with_emb else None, N,
                    dst, ldd)
    want = src[row_map.long(), :FD] + (emb[spk.long()] if with_emb else 0)
    got = dst.cpu()
    assert torch.equal(got[:N, :FD], want)
    assert torch.equal(got[:N, FD:], dst0[:N, FD:]) and torch.equal(got[N], dst0[N])


@pytest.mark.parametrize("N", [1, 33, 257])
def test_emb_grad_matches_index_add_and_is_deterministic(capi, N):
    g = torch.Generator().manual_seed(N)
    S, ld = 9, 208
    dl = torch.randn(N, ld, generator=g)
    spk = torch.randint(0, S - 1, (N,), generator=g).to(torch.int32)
    spk[spk == 4] = 5                                                      # speakers 4 and 8 have no rows
    want = torch.zeros(S, FD, dtype=torch.float64).index_add_(0, spk.long(), dl[:, :FD].double())
    outs = []
    for _ in range(2):
        demb = torch.full((S + 1, FD), 7.0, device=DEV)
        ws = torch.full((capi.mm_emb_grad_ws_floats(S),), float("nan"), device=DEV)
        capi.mm_emb_grad(dl.to(DEV), ld, spk.to(DEV), N, S, demb, ws)
        outs.append(demb.cpu())
    got = outs[0]
    assert torch.equal(outs[0], outs[1])
    assert float(got[4].abs().max()) == 0.0 and float(got[8].abs().max()) == 0.0 and bool((got[S] == 7.0).all())
    scale = float(want.abs().max())
    assert float((got[:S].double() - want).abs().max()) <= 1e-6 * scale


# ----------------------------------------------------------------------------- elementwise and dropout
def _rng(seed=123, offset=7):
    return torch.tensor([offset, seed], dtype=torch.int64, device=DEV)


def _kept_is_scaled(y, x, keep, p):
    """y = x * ks where kept: the fp32 keep scale 1 / (1 - p) and the product round once each (2^-22 covers both)"""
    want = x.double()[keep] / (1.0 - p)
    assert bool(((y.double()[keep] - want).abs() <= 2.0 ** -22 * want.abs()).all())


@pytest.mark.parametrize("n", [1, 255, BIG])
def test_dropout_fwd_masks(capi, n):
    p = 0.4
    g = torch.Generator().manual_seed(n % 1000)
    x = torch.randn(n, generator=g).abs() + 0.5
    xd = x.to(DEV)

    def run(rng, stream):
        y = torch.full((n + 5,), 9.0, device=DEV)
        capi.dropout_fwd(xd, n, p, rng, stream, y)
        assert bool((y[n:] == 9.0).all())
        return y[:n].cpu()
    y = run(_rng(), 1000)
    keep = y != 0
    _kept_is_scaled(y, x, keep, p)
    assert torch.equal(y, run(_rng(), 1000)), "same state, same stream: same mask"
    if n == BIG:
        assert abs(1.0 - float(keep.double().mean()) - p) < 0.01
        for other in (run(_rng(), 1001) != 0, run(_rng(offset=8), 1000) != 0, run(_rng(seed=124), 1000) != 0):
            assert abs(float((other == keep).double().mean()) - (p * p + (1 - p) * (1 - p))) < 0.01


@pytest.mark.parametrize("M,N", [(2, 1), (3, 1), (3, 437)])
def test_regroup_forward_and_backward(capi, M, N):
    """FE[i, m 400 + c] = relu(dropout(cat[xd, h][(m, i), c])); p = 0: relu(cat) exactly; the backward routes dFE * ks exactly where
    FE > 0 and writes 0 elsewhere.  M N 400 = 524 400 at (3, 437) passes the grid cap of 524 288 elements."""
    p, ks = 0.4, 1.0 / (1.0 - 0.4)
    g = torch.Generator().manual_seed(N + M)
    xd, h = torch.randn(M * N, FD, generator=g), torch.randn(M * N, FD, generator=g)
    cat = torch.cat([xd, h], 1)
    cat = torch.cat([cat[N * m:N * (m + 1)] for m in range(M)], 1)            # [N, M 400]
    total = N * M * 2 * FD
    assert (N == 1) or total > 2048 * 256
    FE = torch.full((total + 5,), 9.0, device=DEV)
    capi.mm_regroup_fwd(xd.to(DEV), h.to(DEV), M, N, 0.0, None, 0, FE)
    assert torch.equal(FE[:total].cpu().view(N, -1), torch.relu(cat)) and bool((FE[total:] == 9.0).all())
    outs = []
    for stream in (3000, 3000, 3001):
        capi.mm_regroup_fwd(xd.to(DEV), h.to(DEV), M, N, p, _rng(), stream, FE)
        outs.append(FE[:total].cpu().view(N, -1))
    fe = outs[0]
    assert torch.equal(fe, outs[1]) and bool((FE[total:] == 9.0).all())
    pos = cat > 0
    keep = fe != 0
    assert not bool(keep[~pos].any())
    _kept_is_scaled(fe, cat, keep, p)
    if N > 1:
        assert abs(1.0 - float(keep[pos].double().mean()) - p) < 0.01
        assert abs(float(((outs[2] != 0) == keep)[pos].double().mean()) - (p * p + (1 - p) * (1 - p))) < 0.01
    dFE = torch.randn(N, M * 2 * FD, generator=g)
    d_xd, d_h = torch.full((M * N, FD), 9.0, device=DEV), torch.full((M * N, FD), 9.0, device=DEV)
    capi.mm_regroup_bwd(dFE.to(DEV), fe.to(DEV), M, N, ks, d_xd, d_h)
    want = torch.where(fe > 0, dFE * torch.tensor(ks, dtype=torch.float32), torch.zeros(()))
    want = torch.cat([want[:, 2 * FD * m:2 * FD * (m + 1)] for m in range(M)], 0)       # back to node rows [M N, 400]
    assert torch.equal(d_xd.cpu(), want[:, :FD]) and torch.equal(d_h.cpu(), want[:, FD:])


@pytest.mark.parametrize("n", [1, 255, BIG])
def test_gcnii_combine_forward_and_backward(capi, n):
    """out = theta G + (1 - theta)((1 - alpha) hi + alpha h0), hd = dropout(relu(out)); plain (the input layer): hd = relu(G).
    Backward: dout = d_hd [hd > 0] ks; dG = theta dout, dhi = (1 - theta)(1 - alpha) dout, dh0 += (1 - theta) alpha dout at row pitch
    ld_d (200, and 208 > F); plain: dG = dout."""
    theta, alpha, p = math.log(0.5 / 3 + 1), 0.1, 0.4
    ks = 1.0 / (1.0 - p)
    g = torch.Generator().manual_seed(n % 997)
    G, hi, h0, d_hd = (torch.randn(n, generator=g) for _ in range(4))
    out64 = theta * G.double() + (1 - theta) * ((1 - alpha) * hi.double() + alpha * h0.double())
    hd = torch.full((n + 3,), 9.0, device=DEV)
    capi.gcnii_combine_fwd(G.to(DEV), hi.to(DEV), h0.to(DEV), n, theta, alpha, 0.0, None, 0, hd)
    tol = 8 * 2.0 ** -24 * float(G.abs().max() + hi.abs().max() + h0.abs().max())      # eight roundings of values this size
    assert float((hd[:n].cpu().double() - torch.relu(out64)).abs().max()) <= tol and bool((hd[n:] == 9.0).all())
    capi.gcnii_combine_fwd(G.to(DEV), None, None, n, theta, alpha, 0.0, None, 0, hd)
    assert torch.equal(hd[:n].cpu(), torch.relu(G))
    outs = []
    for stream in (2003, 2003, 2004):
        capi.gcnii_combine_fwd(G.to(DEV), hi.to(DEV), h0.to(DEV), n, theta, alpha, p, _rng(), stream, hd)
        outs.append(hd[:n].cpu())
    hdp = outs[0]
    assert torch.equal(hdp, outs[1])
    clear = out64 > 1e-3
    keep = hdp != 0
    assert not bool(keep[out64 < -1e-3].any())
    assert float((hdp.double()[keep] - out64[keep] * ks).abs().max() if keep.any() else 0.0) <= 2 * tol
    if n == BIG:
        assert abs(1.0 - float(keep[clear].double().mean()) - p) < 0.01
        assert abs(float(((outs[2] != 0) == keep)[clear].double().mean()) - (p * p + (1 - p) * (1 - p))) < 0.01
    # backward
    gate = (hdp > 0).double()
    dout = d_hd.double() * gate * ks
    dG = torch.full((n + 3,), 9.0, device=DEV)
    capi.gcnii_combine_bwd(d_hd.to(DEV), hdp.to(DEV), n, 0.0, 0.0, ks, 1, dG, None, None)
    assert float((dG[:n].cpu().double() - dout).abs().max()) <= 1e-6 * float(dout.abs().max() + 1) and bool((dG[n:] == 9.0).all())
    rows = (n + FD - 1) // FD
    idx = torch.arange(n)
    for ld_d in (FD, 208):
        j = (idx // FD) * ld_d + idx % FD
        dhi0, dh00 = torch.randn(rows * ld_d, generator=g), torch.randn(rows * ld_d, generator=g)
        dhi, dh0 = dhi0.to(DEV), dh00.to(DEV)
        capi.gcnii_combine_bwd(d_hd.to(DEV), hdp.to(DEV), n, theta, alpha, ks, 0, dG, dhi, dh0, F=FD, ld_d=ld_d)
        w_hi, w_h0 = dhi0.double().clone(), dh00.double().clone()
        w_hi[j] = (1 - theta) * (1 - alpha) * dout
        w_h0[j] += (1 - theta) * alpha * dout
        tol = 1e-6 * float(dout.abs().max() + 1)
        assert float((dG[:n].cpu().double() - theta * dout).abs().max()) <= tol
        assert float((dhi.cpu().double() - w_hi).abs().max()) <= tol and float((dh0.cpu().double() - w_h0).abs().max()) <= tol
        untouched = torch.ones(rows * ld_d, dtype=torch.bool)
        untouched[j] = False
        assert torch.equal(dhi.cpu()[untouched], dhi0[untouched]) and torch.equal(dh0.cpu()[untouched], dh00[untouched])


@pytest.mark.parametrize("n", [1, 255, BIG])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("masked", [False, True])
def test_axpy_mask(capi, n, accumulate, masked):
    """y (+)= x * scale where mask != 0 (everywhere without a mask); a masked-out entry contributes 0, and with accumulate = 0
    overwrites"""
    g = torch.Generator().manual_seed(n % 991 + accumulate)
    x, y0 = torch.randn(n, generator=g), torch.randn(n + 3, generator=g)
    mask = torch.randn(n, generator=g) * (torch.rand(n, generator=g) < 0.6)
    scale = 1.0 / 0.6
    y = y0.to(DEV)
    capi.axpy_mask(x.to(DEV), mask.to(DEV) if masked else None, n, scale, accumulate, y)
    v = x * torch.tensor(scale, dtype=torch.float32)
    if masked:
        v = torch.where(mask != 0, v, torch.zeros(()))
    want = y0[:n] + v if accumulate else v
    got = y.cpu()
    if accumulate:      # the product and the sum may be one fused multiply-add: within a rounding of the two-step result
        assert bool(((got[:n] - want).abs() <= 2.0 ** -23 * (y0[:n].abs() + v.abs())).all())
    else:
        assert torch.equal(got[:n], want)
    assert torch.equal(got[n:], y0[n:])
