"""DialogueGCN's graph kernels (csrc/dgcn_ops.hip) called one by one, in every launch form -- separate basis-space kernels, the three
fp32 matrix-core tile launches, the relation-space kernels, EdgeAtt forward / backward with the fold-ins of erc_edge_att_bwd_fused --
each against the float64 restatement tests/dgcn_ops_ref.py (pinned to oracle.dgcn and the reference fixtures by
tests/test_dgcn_ops_ref.py).  A kernel is fed the REFERENCE's operands rounded to fp32, never another kernel's output: errors do
not compound and a failure names one kernel.  Output buffers start as NaN, pad columns of the inputs hold NaN, LDS is poisoned in
front of the tile launches, comparisons are done on the host.

Bounds.  norm: the golden test's (atol 2e-6, rtol 2e-5), as a ratio |got - want| / (atol + rtol |want|) <= 1.  Everything that is a
sum of fp32 products: rel_err against float64 <= max(4 x the rel_err of the SAME restatement run in float32 on the CPU, FLOOR) --
the rule of tests/test_gpu_mmgcn_ops.py; the yardstick is computed here, per case and per quantity.  Copies and rows that are
mathematically empty: torch.equal.  The relation sums d att are also held against the float64 sum of the very TT they summed.
On the `hot` cases (scores up to 180, almost half of the edges below 1e-30) no fp32 implementation holds the norm bound: the float32
CPU run of the restatement has ratio 1.7 (ragged graph) and 2.8 (wide graph), the kernel 1.2 and 2.2 -- so there the bound is 4 x
the float32 run's ratio (6.8 and 11), as for the sums.

Measured on an MI355X, largest rel_err over the cases | the float32 yardstick of the same case and quantity (`hot` cases apart: their
yardsticks are 1e-5 .. 7e-4, the kernels stay where they are on the others).  No comparison came closer to its bound than 0.2 of
it (norm, hot-wide); everything that is a sum stays below 0.05 of FLOOR but EdgeAtt's dx on hot-wide (0.13 of its bound).
  EdgeAtt         norm ratio 0.018 | 0.019 (hot 2.2 | 2.8); dscore 1.1e-7 | 3.3e-7; DATT 3.5e-7 | 5.0e-7; dx 4.5e-7 | 4.2e-7 (hot 3.7e-4
                  | 6.9e-4: dx_j = sum_e dscore_e ATT[dst_e] cancels there); d att riding along 3.3e-7 | 4.0e-7
  basis separate  Z 3.9e-7 | 3.0e-7; dnorm 1.2e-7 | 4.3e-7; TT 1.6e-7 | 3.6e-7; datt 4.8e-7 | 4.2e-7; U 5.6e-7 | 4.2e-7
  tile            Z 3.9e-7 | 3.0e-7; out 3.0e-7 | 3.6e-7; dx 5.3e-8 | 5.3e-8; dnorm 2.3e-7 | 4.3e-7; TT 2.9e-7 | 3.3e-7; datt 5.5e-7 | 4.2e-7
  relation space  Wr 2.3e-7 | 2.3e-7; Z_rel 1.9e-7 | 2.4e-7; dnorm 1.0e-7 | 4.3e-7; U_rel 2.2e-7 | 4.1e-7; dbasis 1.0e-7 | 2.7e-7;
                  dcomp 2.2e-7 | 7.4e-7
  relation sums   overflow-real: datt 9.0e-7 | 1.9e-6, against the float64 sum of its own TT 9.0e-7 | 4.4e-6; at the list capacity
                  5.8e-7 | 2.1e-6 (2048 matches), 7.0e-7 | 1.5e-6 (2049)
  other widths    <= 2.3e-7 everywhere (norm ratio 0.011); csr_sum 2.9e-7 | 2.9e-7; gather_rows, transpose_batched and WrT identical
"""
import functools
import types

import numpy as np
import pytest
import torch

from tests import dgcn_ops_ref as ref
from tests.util_cases import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NB = ref.NB
FLOOR = 2e-5
RS_CAP = 2048          # csrc/dgcn_ops.hip RS_CAP: matching edges a wavefront of rel_sum_body keeps before the scan-and-add fallback
NAN = float("nan")
PROFILE = (-3.0, -8.0, -20.0, -45.0, -75.0, -110.0, -150.0, -200.0)        # hot: score offsets below a dialogue's best target

WIDE = (110, 3, 65, 64, 66)        # degree = dialogue length: one full pass (64), one edge in the second (65); nodes 112 | 113 have 3 | 65
RAGGED = (1, 5, 17, 16, 2)         # N = 41
CASES = {
    "one": dict(lengths=(1,), S=2, win=(10, 10)),
    "ragged": dict(lengths=RAGGED, S=2, win=(10, 10)),
    "s9": dict(lengths=(33, 1, 20), S=9, win=(10, 10)),
    "asym-past": dict(lengths=(40, 7), S=3, win=(-1, 2)),
    "asym-future": dict(lengths=(40, 7), S=3, win=(3, -1)),
    "wide-s2": dict(lengths=WIDE, S=2, win=(-1, -1)),
    "wide-s9": dict(lengths=WIDE, S=9, win=(-1, -1)),
    "three-pass": dict(lengths=(130,), S=2, win=(-1, -1)),
    "hot-ragged": dict(lengths=RAGGED, S=2, win=(10, 10), hot=True),
    "hot-wide": dict(lengths=WIDE, S=2, win=(-1, -1), hot=True),
    "overflow-real": dict(lengths=(110, 110), S=1, win=(-1, -1)),
}
EVERY = [n for n in CASES if n != "overflow-real"]
FOLD = ["ragged", "wide-s2", "wide-s9"]
WIDTHS = [(1, 1), (64, 64), (65, 65), (256, 128)]


@pytest.fixture(scope="module")
def capi():
    from erc_amd import capi as c
    c.lib()
    return c


def _hot_features(W, lengths, gen):
    """Rows s (P + t_k w) + noise per dialogue: score(j -> k) = const(j) + PROFILE-like offsets(k), the same ranking for every source.
    The two middle utterances of a dialogue are its best targets, 0.3 apart (inside every +-10 window of dialogues up to 21 long),
    the others fall off by PROFILE; in the first dialogue of two or more the two are the SAME row: every source there has a tie."""
    Fd, Wd, rows, tie, off = W.shape[0], W.double(), [], None, 0
    for L in lengths:
        cand = torch.randn(8, Fd, generator=gen).double()
        q = ((cand @ Wd) * cand).sum(1)
        P, pwp = cand[int(q.argmax())], float(q.max())
        w = Wd.t() @ P
        w = w / w.norm() * Fd ** 0.5
        s2 = 170.0 / pwp                                   # score(k -> k) ~ s^2 P W P = 170
        prof = torch.tensor([PROFILE[k % len(PROFILE)] for k in range(L)], dtype=torch.float64)
        a = (L - 1) // 2
        if L >= 2:
            prof[a], prof[a + 1] = 0.0, -0.3
        t = prof / (s2 * float(P @ Wd @ w))
        xd = (s2 ** 0.5 * (P[None] + t[:, None] * w[None]) + 0.01 * torch.randn(L, Fd, generator=gen).double()).float()
        if L >= 2 and tie is None:
            xd[a + 1], tie = xd[a], (off + a, off + a + 1)
        rows.append(xd)
        off += L
    return torch.cat(rows, 0), tie


@functools.lru_cache(maxsize=None)
def _case(name, Fd=200, O=100):
    """graph (device builder, checked against the host's), seeded operands, the float64 reference and the float32 yardstick: built once"""
    from erc_amd.cogmen import build_graph_tensors
    spec = CASES[name]
    lengths, S, (wp, wf) = spec["lengths"], spec["S"], spec["win"]
    R, B, T = 2 * S * S, len(lengths), max(lengths)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 7 * Fd + O)
    spk = torch.randint(0, S, (B, T), generator=gen)
    g, ei, et = build_graph_tensors(torch.tensor(lengths, device=DEV), spk.to(DEV), wp, wf, S)
    N, E = g["counts"].cpu().tolist()
    ei, et = ei[:, :E].cpu(), et[:E].cpu()
    hei, het = ref.host_graph(lengths, spk, wp, wf, S)
    assert N == sum(lengths) and torch.equal(ei, hei) and torch.equal(et, het)
    assert torch.equal(g["node_row"][:N].cpu(), torch.cat([b * T + torch.arange(L) for b, L in enumerate(lengths)]).int())
    W = torch.randn(Fd, Fd, generator=gen) / Fd            # scores of order 1 from N(0, 1) rows
    x, tie = torch.randn(N, Fd, generator=gen), None
    if spec.get("hot"):
        x, tie = _hot_features(W, lengths, gen)
    rn = lambda scale, *s: torch.randn(*s, generator=gen) * scale
    comp, basis, root, bias, gout = rn(0.3, R, NB), rn(0.1, NB, Fd, O), rn(0.1, Fd, O), rn(0.1, O), rn(0.1, N, O)
    c = types.SimpleNamespace(name=name if (Fd, O) == (200, 100) else "%s-%dx%d" % (name, Fd, O), hot=bool(spec.get("hot")), F=Fd, O=O,
                              S=S, R=R, N=N, E=E, B=B, T=T, g=g, ei=ei, et=et, x=x, W=W, comp=comp, basis=basis, root=root, bias=bias,
                              gout=gout, tie=tie, XW=Fd + O, LA=Fd + 4, LH=O + 4, LDX=Fd + 5, LDA=Fd + 3,
                              dx0=rn(1.0, N, Fd + 5), da0=rn(1.0, N, Fd + 3), dxw0=rn(1.0, N, Fd + O),
                              u6=torch.rand(6, E, generator=gen, dtype=torch.float64) + 0.1, v6=torch.rand(6, N, 1, generator=gen, dtype=torch.float64) + 0.1)
    c.r64 = ref.restate(ei, et, R, x, W, comp, basis, root, bias, gout)
    c.r32 = ref.restate(ei, et, R, x, W, comp, basis, root, bias, gout, dtype=torch.float32)
    c.occupied = torch.zeros(R, dtype=torch.bool).index_fill(0, et, True)
    if c.hot:
        _assert_hot(c)
    return c


def _assert_hot(c):
    score, norm, src = c.r64["score"], c.r64["norm"], c.ei[0]
    assert float(score.max()) > 150                                         # expf overflows without the max-subtraction
    assert float((norm < 1e-30).double().mean()) >= 0.10
    deg = torch.bincount(src, minlength=c.N)
    keep = torch.zeros(c.N, dtype=torch.long).index_add(0, src, (norm > 1e-6).long())
    assert int(keep[deg >= 2].min()) >= 2                                   # (a source with one out-edge has one: norm = 1)
    a, b = c.tie
    assert torch.equal(c.x[a], c.x[b])
    eid = {(int(s), int(d)): i for i, (s, d) in enumerate(zip(c.ei[0].tolist(), c.ei[1].tolist()))}
    ties = [(eid[(j, a)], eid[(j, b)]) for j in range(c.N) if (j, a) in eid and (j, b) in eid]
    assert ties and all(float(score[p]) == float(score[q]) for p, q in ties)


def _dev(t, pitch=None):
    """fp32 copy on the device; with ``pitch``: rows that far apart, the pad columns NaN"""
    t = t.to(torch.float32)
    if pitch is None:
        return t.contiguous().to(DEV)
    buf = torch.full((t.shape[0], pitch), NAN)
    buf[:, :t.shape[1]] = t
    return buf.to(DEV)


def _nan(*s):
    return torch.full(s, NAN, device=DEV)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class _Check:
    """prints every figure, collects the misses; done() asserts there is none"""

    def __init__(self, group, c):
        self.group, self.c, self.bad = group, c, []

    def close(self, what, got, want, yard):
        got, e, y = got.cpu(), None, rel_err(yard, want)
        ok = bool(torch.isfinite(got).all()) and got.shape == want.shape
        e = rel_err(got, want) if ok else float("inf")
        b = max(4 * y, FLOOR)
        print("MEASURED %-8s %-18s %-12s rel_err %.3g yardstick %.3g bound %.3g" % (self.group, self.c.name, what, e, y, b))
        if not e <= b:
            self.bad.append((what, e, b))

    def key(self, what, got, k):
        self.close(what, got, self.c.r64[k], self.c.r32[k])

    def norm(self, got):
        want = self.c.r64["norm"]
        ratio = lambda t: float(((t.double() - want).abs() / (2e-6 + 2e-5 * want.abs())).max())
        e, y = ratio(got.cpu()), ratio(self.c.r32["norm"])
        b = max(1.0, 4 * y) if self.c.hot else 1.0
        print("MEASURED %-8s %-18s %-12s ratio %.3g yardstick %.3g bound %.3g" % (self.group, self.c.name, "norm", e, y, b))
        if not e <= b:              # (NaN misses)
            self.bad.append(("norm", e, b))

    def same(self, what, got, want):
        if not _bits(got.cpu(), want.cpu() if torch.is_tensor(want) else want):
            self.bad.append((what, "not identical"))

    def datt(self, what, got, TT):
        """d att against the restatement's, against the float64 sum of the TT it summed, and exactly 0 where no edge has the type"""
        c, TT = self.c, TT.cpu()
        self.key(what, got, "dcomp")
        self.close(what + "|TT", got, ref.relation_sums(TT.double(), c.et, c.R), ref.relation_sums(TT, c.et, c.R))
        self.same(what + " empty", got.cpu()[~c.occupied], torch.zeros(int((~c.occupied).sum()), NB))

    def done(self):
        assert not self.bad, (self.group, self.c.name, self.bad)


# ----------------------------------------------------------------------------- the launches, each into fresh NaN-filled buffers
def _operands(c):
    r = c.r64
    return types.SimpleNamespace(xw=_dev(c.x, c.XW), att=_dev(r["ATT"], c.LA), nrm=_dev(r["norm"]), dn=_dev(r["dnorm"]), gw=_dev(c.gout, c.LH),
                                 comp=_dev(c.comp), basis=_dev(c.basis), root=_dev(c.root), bias=_dev(c.bias))


def _run_edge_att(capi, c):
    o, out = _operands(c), {}
    norm = _nan(c.E)
    capi.edge_att_fwd(o.xw, c.XW, o.att, c.LA, c.F, c.N, c.g, norm)
    out["norm"] = norm
    for acc in (0, 1):
        dx, DATT, dscore = c.dx0.to(DEV), c.da0.to(DEV), _nan(c.E)
        capi.edge_att_bwd(o.xw, c.XW, o.att, c.LA, c.F, c.N, c.g, o.nrm, o.dn, dx, c.LDX, acc, DATT, c.LDA, dscore)
        out["dx%d" % acc], out["DATT%d" % acc], out["dscore%d" % acc] = dx, DATT, dscore
    return out


def _fold_operands(c):
    """d norm as six partial vectors E + 7 apart, dx_rgcn as six slabs N F + 8 apart (NaN in the gaps), both split with positive weights"""
    parts = (c.r64["dnorm"][None] * (c.u6 / c.u6.sum(0))).float()
    dnbuf = torch.full((6, c.E + 7), NAN)
    dnbuf[:, :c.E] = parts
    slabs = (c.r64["dx_rgcn"][None] * (c.v6 / c.v6.sum(0))).float()
    slbuf = torch.full((6, c.N * c.F + 8), NAN)
    slbuf[:, :c.N * c.F] = slabs.reshape(6, -1)
    return dnbuf.to(DEV), slbuf.to(DEV)


def _run_edge_att_folds(capi, c, g=None, TT=None, R=None):
    o, out = _operands(c), {}
    dnbuf, slbuf = _fold_operands(c)
    dx, DATT, dscore = c.dx0.to(DEV), c.da0.to(DEV), _nan(c.E)
    capi.edge_att_bwd(o.xw, c.XW, o.att, c.LA, c.F, c.N, c.g, o.nrm, dnbuf, dx, c.LDX, 0, DATT, c.LDA, dscore, dn_parts=6, dn_stride=c.E + 7)
    out["p_dx"], out["p_DATT"], out["p_dscore"] = dx, DATT, dscore
    TT = _dev(c.r64["TT"]) if TT is None else TT
    R = c.R if R is None else R
    dx, DATT, dscore, datt = c.dx0.to(DEV), c.da0.to(DEV), _nan(c.E), _nan(R, NB)
    capi.edge_att_bwd_fused(o.xw, c.XW, o.att, c.LA, c.F, c.N, c.g if g is None else g, o.nrm, dnbuf, dx, c.LDX, 1, DATT, c.LDA, dscore,
                            dn_parts=6, dn_stride=c.E + 7, dx_slabs=slbuf, n_dx_slabs=6, dx_slab_stride=c.N * c.F + 8, rs_TT=TT,
                            rs_datt=datt, rs_R=R)
    out["f_dx"], out["f_DATT"], out["f_dscore"], out["f_datt"], out["f_TT"] = dx, DATT, dscore, datt, TT
    return out


def _run_basis_separate(capi, c):
    o = _operands(c)
    Z, dnorm, TT, datt, U = _nan(c.N, NB * c.F), _nan(c.E), _nan(c.E, NB), _nan(c.R, NB), _nan(c.N, NB * c.O)
    capi.brgcn_agg_fwd(o.xw, c.XW, c.F, c.N, c.g, o.nrm, o.comp, NB, Z)
    capi.brgcn_bwd_edges(o.xw, c.XW, c.F, c.N, c.R, c.g, o.nrm, o.comp, NB, _dev(c.r64["dZ"]), dnorm, TT, datt)
    capi.brgcn_bwd_source(o.gw, c.LH, c.O, c.N, c.g, o.nrm, o.comp, NB, U)
    return dict(Z=Z, dnorm=dnorm, TT=TT, datt=datt, U=U)


def _run_tile(capi, c):
    o, Sg, st = _operands(c), capi.brgcn_fwd_tile_slabs(), c.E + 3
    Z, slabs, out = _nan(c.N, NB * c.F), _nan(Sg, c.N, c.O), _nan(c.N, c.O)
    capi.poison_lds()
    capi.brgcn_fwd_tile(o.xw, c.XW, c.F, c.O, c.N, c.g, o.nrm, o.comp, NB, o.basis, o.root, Z, slabs)
    capi.slab_reduce(slabs, Sg, c.N * c.O, o.bias, c.O, 0, out, c.N * c.O)
    dsl, dx = _nan(Sg, c.N, c.F), c.dxw0.to(DEV)
    capi.poison_lds()
    capi.brgcn_bwd_source_tile(o.gw, c.LH, c.F, c.O, c.N, c.g, o.nrm, o.comp, NB, o.basis, o.root, dsl)
    capi.slab_reduce(dsl, Sg, c.N * c.F, None, c.F, 4, dx, c.N * c.F, ld_out=c.XW)
    dnsl, TT, datt, dn = _nan(Sg, st), _nan(c.E, NB), _nan(c.R, NB), _nan(c.E)
    capi.poison_lds()
    capi.brgcn_bwd_edges_tile(o.xw, c.XW, c.F, c.O, c.N, c.R, c.g, o.nrm, o.comp, NB, o.basis, o.gw, c.LH, TT, dnsl, st, datt)
    capi.slab_reduce(dnsl, Sg, st, None, 0, 0, dn, c.E)
    return dict(Z=Z, slabs=slabs, out=out, dsl=dsl, dx=dx, dnsl=dnsl, TT=TT, datt=datt, dnorm=dn)


def _run_relation(capi, c):
    o, R = _operands(c), c.R
    Wr, WrT, Zr, dn, Ur = _nan(R, c.F, c.O), _nan(R, c.O, c.F), _nan(c.N, R * c.F), _nan(c.E), _nan(c.N, R * c.O)
    dbasis, dcomp = _nan(NB, c.F, c.O), _nan(R, NB)
    capi.basis_compose(o.comp, o.basis, R, NB, c.F, c.O, Wr, WrT)
    capi.rrgcn_agg_fwd(o.xw, c.XW, c.F, c.N, R, c.g, o.nrm, Zr)
    capi.rrgcn_bwd_edges(o.xw, c.XW, c.F, c.N, R, c.g, _dev(c.r64["dZ_rel"]), dn)
    capi.rrgcn_bwd_source(o.gw, c.LH, c.O, c.N, R, c.g, o.nrm, Ur)
    capi.basis_decompose(o.comp, o.basis, _dev(c.r64["dWr"]), R, NB, c.F * c.O, dbasis, dcomp)
    return dict(Wr=Wr, WrT=WrT, Z_rel=Zr, dnorm=dn, U_rel=Ur, dbasis=dbasis, dcomp=dcomp)


def _run_csr(capi, c):
    o, out = _operands(c), {}
    for side, ptr, idx in (("in", "in_ptr", "in_src"), ("out", "out_ptr", "out_dst")):
        for acc in (0, 1):
            y = c.dx0.to(DEV)
            capi.csr_sum(o.xw, c.XW, c.F, c.N, c.g[ptr], c.g[idx], y, c.LDX, acc)
            out["%s%d" % (side, acc)] = y
    return out


# ----------------------------------------------------------------------------- the comparisons
def _check_edge_att(k, c, got):
    r64, r32, F = c.r64, c.r32, c.F
    k.norm(got["norm"])
    for acc in (0, 1):
        dx, DATT, ds = got["dx%d" % acc].cpu(), got["DATT%d" % acc].cpu(), got["dscore%d" % acc]
        k.key("dscore", ds, "dscore")
        k.key("DATT", DATT[:, :F], "DATT")
        k.close("dx acc=%d" % acc, dx[:, :F], r64["dx_att"] + acc * c.dx0[:, :F].double(), r32["dx_att"] + acc * c.dx0[:, :F])
        k.same("dx pad", dx[:, F:], c.dx0[:, F:])
        k.same("DATT pad", DATT[:, F:], c.da0[:, F:])
    if c.E == 1:
        k.same("dscore of a one-edge softmax", got["dscore0"], torch.zeros(1))


def _check_folds(k, c, got):
    r64, r32, F = c.r64, c.r32, c.F
    for p in ("p_", "f_"):
        dx, DATT = got[p + "dx"].cpu(), got[p + "DATT"].cpu()
        k.key(p + "dscore", got[p + "dscore"], "dscore")
        k.key(p + "DATT", DATT[:, :F], "DATT")
        k.same(p + "dx pad", dx[:, F:], c.dx0[:, F:])
        k.same(p + "DATT pad", DATT[:, F:], c.da0[:, F:])
    k.key("p_dx", got["p_dx"].cpu()[:, :F], "dx_att")
    k.close("f_dx", got["f_dx"].cpu()[:, :F], c.dx0[:, :F].double() + r64["dx_att"] + r64["dx_rgcn"], c.dx0[:, :F] + r32["dx_att"] + r32["dx_rgcn"])
    k.datt("f_datt", got["f_datt"], got["f_TT"])


def _check_basis_separate(k, c, got):
    for q in ("Z", "dnorm", "TT", "U"):
        k.key(q, got[q], q)
    k.datt("datt", got["datt"], got["TT"])


def _check_tile(k, c, got):
    F = c.F
    for q in ("Z", "out", "dnorm", "TT"):
        k.key(q, got[q], q)
    k.datt("datt", got["datt"], got["TT"])
    dx = got["dx"].cpu()
    k.close("dx", dx[:, :F], c.dxw0[:, :F].double() + c.r64["dx_rgcn"], c.dxw0[:, :F] + c.r32["dx_rgcn"])
    k.same("dx pad", dx[:, F:], c.dxw0[:, F:])


def _check_relation(k, c, got):
    for q in ("Wr", "Z_rel", "dnorm", "U_rel", "dbasis", "dcomp"):
        k.key(q, got[q], q)
    k.same("WrT", got["WrT"], got["Wr"].transpose(1, 2).contiguous())


def _check_csr(k, c, got):
    src, dst = c.ei
    for side, (a, b) in (("in", (dst, src)), ("out", (src, dst))):
        s64 = torch.zeros(c.N, c.F, dtype=torch.float64).index_add(0, a, c.x.double()[b])
        s32 = torch.zeros(c.N, c.F).index_add(0, a, c.x[b])
        for acc in (0, 1):
            y = got["%s%d" % (side, acc)].cpu()
            k.close("csr %s acc=%d" % (side, acc), y[:, :c.F], s64 + acc * c.dx0[:, :c.F].double(), s32 + acc * c.dx0[:, :c.F])
            k.same("csr pad", y[:, c.F:], c.dx0[:, c.F:])


# ----------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", ["hot-ragged", "hot-wide"])
def test_hot_features_meet_their_conditions_on_the_reference(name):
    """largest score > 150, >= 10 % of the edges below 1e-30, every source with two or more out-edges keeps two above 1e-6 (the one
    utterance dialogue of the ragged graph has a single edge, norm = 1), one pair of identical rows whose scores tie exactly"""
    _assert_hot(_case(name))


@pytest.mark.parametrize("name", EVERY)
def test_edge_att_forward_and_backward_match_float64(capi, name):
    """edge_att_fwd -> norm; edge_att_bwd -> dscore, DATT, dx into a wider pre-filled buffer, accumulate_dx 0 and 1"""
    c = _case(name)
    k = _Check("edgeatt", c)
    _check_edge_att(k, c, _run_edge_att(capi, c))
    k.done()


@pytest.mark.parametrize("name", FOLD)
def test_edge_att_backward_fold_ins_match_float64(capi, name):
    """dn_parts = 6 (partial d norm vectors E + 7 apart), and erc_edge_att_bwd_fused with six dx slabs and the relation sums riding along"""
    c = _case(name)
    k = _Check("edgeatt", c)
    _check_folds(k, c, _run_edge_att_folds(capi, c))
    k.done()


@pytest.mark.parametrize("name", EVERY)
def test_basis_space_separate_kernels_match_float64(capi, name):
    """brgcn_agg_fwd -> Z; brgcn_bwd_edges -> dnorm, TT, datt; brgcn_bwd_source -> U"""
    c = _case(name)
    k = _Check("basis", c)
    _check_basis_separate(k, c, _run_basis_separate(capi, c))
    k.done()


@pytest.mark.parametrize("name", EVERY)
def test_basis_space_tile_launches_match_float64(capi, name):
    """brgcn_fwd_tile -> Z, out; brgcn_bwd_source_tile -> dx (epilogue 4, ld_out = F + O); brgcn_bwd_edges_tile -> TT, dnorm, datt"""
    c = _case(name)
    k = _Check("tile", c)
    _check_tile(k, c, _run_tile(capi, c))
    k.done()


@pytest.mark.parametrize("name", [n for n in EVERY if 2 * CASES[n]["S"] ** 2 <= 8])
def test_relation_space_kernels_match_float64(capi, name):
    """basis_compose, rrgcn_agg_fwd, rrgcn_bwd_edges, rrgcn_bwd_source, basis_decompose; R <= rrgcn_max_relations() is their contract"""
    c = _case(name)
    assert c.R <= capi.rrgcn_max_relations() == 8
    k = _Check("relation", c)
    _check_relation(k, c, _run_relation(capi, c))
    k.done()


@pytest.mark.parametrize("Fd,O", WIDTHS)
def test_generic_kernels_at_other_widths_match_float64(capi, Fd, O):
    """the lane masks of the F <= 256 / O <= 128 kernels at one channel, a full chunk, a chunk and one, and the widest rows"""
    c = _case("ragged", Fd, O)
    k = _Check("widths", c)
    _check_edge_att(k, c, _run_edge_att(capi, c))
    _check_basis_separate(k, c, _run_basis_separate(capi, c))
    _check_relation(k, c, _run_relation(capi, c))
    _check_csr(k, c, _run_csr(capi, c))
    k.done()


def test_csr_sum_gather_rows_and_transpose(capi):
    c = _case("wide-s2")
    k = _Check("small", c)
    _check_csr(k, c, _run_csr(capi, c))
    gen = torch.Generator().manual_seed(3)
    rows, Fd = c.B * c.T, c.F
    src, back = torch.randn(rows, Fd + 2, generator=gen), torch.randn(rows, Fd + 1, generator=gen)
    node_row = c.g["node_row"][:c.N].cpu().long()
    x = _nan(c.N, Fd + 3)
    capi.gather_rows(src.to(DEV), Fd + 2, c.g["node_row"], c.N, Fd, x, Fd + 3)
    k.same("gather", x.cpu()[:, :Fd], src[node_row, :Fd])
    y, want = back.to(DEV), back.clone()
    capi.gather_rows(x, Fd + 3, c.g["node_row"], c.N, Fd, y, Fd + 1, scatter=1)
    want[node_row, :Fd] = src[node_row, :Fd]
    k.same("scatter", y, want)
    nb, rws, cols = 3, 419, 419                        # 526 683 elements: past the grid cap of 2048 workgroups x 256
    assert nb * rws * cols > 2048 * 256
    t = torch.randn(nb, rws, cols, generator=gen)
    tt = _nan(nb, cols, rws)
    capi.transpose_batched(t.to(DEV), nb, rws, cols, tt)
    k.same("transpose", tt, t.transpose(1, 2).contiguous())
    k.done()


def test_relation_sums_take_the_fallback_on_two_long_dialogues(capi):
    """Two dialogues of 110 utterances, one speaker, unbounded window: 24 200 edges of two relations, more than RS_CAP of one relation
    in a wavefront's quarter of the edge list -- rel_sum_body's scan-and-add fallback, from all three launches that sum d att."""
    c = _case("overflow-real")
    per = (c.E + 3) // 4
    quarter = [[int((c.et[w * per:min(c.E, (w + 1) * per)] == r).sum()) for r in range(c.R)] for w in range(4)]
    assert c.E == 24200 and c.R == 2 and max(max(q) for q in quarter) > RS_CAP, quarter
    k = _Check("relsum", c)
    sep, tile, fold = _run_basis_separate(capi, c), _run_tile(capi, c), _run_edge_att_folds(capi, c)
    k.key("TT", sep["TT"], "TT")
    k.key("TT tile", tile["TT"], "TT")
    k.datt("datt", sep["datt"], sep["TT"])
    k.datt("datt tile", tile["datt"], tile["TT"])
    k.datt("datt fused", fold["f_datt"], fold["f_TT"])
    k.done()


@pytest.mark.parametrize("zeros", [RS_CAP, RS_CAP + 1], ids=["list-full", "one-over"])
def test_relation_sums_at_the_list_capacity(capi, zeros):
    """Crafted edge types riding along in erc_edge_att_bwd_fused: E = 8203 (quarters of 2051: no multiple of 4 or 512), relation 0
    exactly RS_CAP times in wavefront 0's quarter (list full, no fallback), then once more (fallback); relation 2 never."""
    c = _case("ragged")
    E, R, per = 8203, 3, 2051
    typ = (torch.arange(E) % 2).int()
    typ[:per] = 0
    ones = [5, 700, per - 1][:per - zeros]
    typ[ones] = 1
    assert int((typ[:per] == 0).sum()) == zeros and all(int((typ[w * per:(w + 1) * per] == r).sum()) <= RS_CAP for w in (1, 2, 3) for r in (0, 1))
    TT = torch.randn(E, NB, generator=torch.Generator().manual_seed(zeros))
    g = dict(c.g, in_typ=typ.to(DEV), counts=torch.tensor([c.N, E], dtype=torch.int32, device=DEV))
    got = _run_edge_att_folds(capi, c, g=g, TT=TT.to(DEV), R=R)["f_datt"].cpu()
    k = _Check("relsum", c)
    k.close("datt %d" % zeros, got, ref.relation_sums(TT.double(), typ.long(), R), ref.relation_sums(TT, typ.long(), R))
    k.same("empty relation", got[2], torch.zeros(NB))
    k.done()


def test_relation_sums_of_one_edge(capi):
    c = _case("ragged")
    TT = torch.randn(1, NB, generator=torch.Generator().manual_seed(1))
    g = dict(c.g, in_typ=torch.tensor([1], dtype=torch.int32, device=DEV), counts=torch.tensor([c.N, 1], dtype=torch.int32, device=DEV))
    got = _run_edge_att_folds(capi, c, g=g, TT=TT.to(DEV), R=3)["f_datt"].cpu()
    assert _bits(got, torch.cat([torch.zeros(1, NB), TT, torch.zeros(1, NB)]))


@pytest.mark.parametrize("name", ["wide-s2", "wide-s9"])
def test_every_launch_repeats_its_bits(capi, name):
    """a second run of every launch, buffers and LDS poisoned again, gives the same bits"""
    c = _case(name)
    runs = [_run_edge_att, _run_edge_att_folds, _run_basis_separate, _run_tile, _run_csr] + ([_run_relation] if c.R <= 8 else [])
    for run in runs:
        a, b = run(capi, c), run(capi, c)
        for q in a:
            assert _bits(a[q].cpu(), b[q].cpu()), (run.__name__, q)
