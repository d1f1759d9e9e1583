"""Float64 restatements of the three per-dialogue attention kernel families, their float32 twins, the inputs and the case tables
that both the host tests (tests/test_att_kernels_ref.py) and the GPU tests (tests/test_gpu_att_kernels.py) use.  numpy only:
nothing here touches a GPU.

CIM (csrc/cim_attn.hip: erc_cim_attn_fwd / _bwd), per dialogue of L rows and ordered pair (x, y) of av va ta tv at vt, with
x, y the dense blocks merged[:, 600 + 100 m) (m = a, v, t) and g = dmerged[:, 100 p .. 100 p + 100):
    S = x y^T      P = softmax_rows(S)  (saved: Pbuf)      h = P y      out = h * x
    dh = g * x     Q = P * (dh y^T)     dS = Q - P rowsum(Q)
    dx += g * h + dS y                  dy += P^T dh + dS^T x          added to dmerged[:, 600:900) on top of what is there
    dmerged[:, 600:900) = dense > 0 ? dmerged[:, 600:900) mask_scale : 0                 (drop1 and ReLU's backward)

MATCHING ATTENTION 'general2' (csrc/match_att.hip: erc_match_att_fwd / _bwd / _bwd_cap), per dialogue:
    th = tanh(Q E^T)       p = exp(th) / rowsum(exp(th))      A = p E                               (saved: P, TH)
    dp = dA E^T            dz = p (dp - rowsum(p dp)) (1 - th^2)                                     (saved: DZ)
    dQ = dz E              dE = p^T dA + dz^T Q

POSITIONAL EDGE ATTENTION (csrc/dgcnv2_att.hip: erc_dgcnv2_edge_att_fwd / _bwd), per dialogue b and source j < L over the
T padded, time-major rows, win(j) = [max(0, j - wp), min(L, j + wf + 1)) (a negative wp / wf: unbounded on that side):
    u_t = exp(S[t, j] - max_{t < T} S[t, j])      den = sum_{t in win} u_t + 1e-10 sum_{t < T, t not in win} u_t
    norm(j -> i) = u_i / den       n_t = u_t / den       dot = sum_{i in win} dn_i n_i
    dS[t, j] = n_t (dn_t - dot) inside the window,  -1e-10 n_t dot outside it (padded rows included);  columns j >= L: 0
The edges (`edge_lists`) are built here from the lengths and the window, in-CSR order for the edge ids and out-CSR order for
what the kernels walk; 1e-10 is the float32 value the reference's mask holds (`LEAK`).

INPUTS.  CIM's dense values look like ReLU + dropout left them: half are exactly 0, the rest lie in (0, 0.65], and the second
non-empty dialogue of a case has an all-zero v block.  The matching attention runs at two scales: 'small' is 0.1 randn for E
and Q (|q . e| < 1: tanh nearly linear), 'sat' keeps E and solves Q = S* pinv(E)^T per dialogue for scores S* drawn uniformly
from [-3.75, 3.75]: a fifth of the pairs have |q . e| > 3, max |th| = tanh(3.75) = 0.9989, and min (1 - th^2) = 2.2e-3 stays
above 1e-3 -- a Gaussian scale with the same fifth would reach |s| = 10 somewhere in 110 x 110 pairs, where 1 - th^2 = 8e-9.
L <= 110 < F, so E has full row rank and Q E^T = S* up to the rounding of Q to float32.

BOUNDS the GPU tests hold the kernels to (never taken from a kernel's output): err / scale = max |got - ref| / max |ref| per
output group and case against float64 (where a group's reference is 0 identically -- DZ and dQ of a case of one-row
dialogues -- over the largest of the terms that cancel in it); BOUND[family][group] = 4 x the float32 twin's worst figure over
that family's cases (F32_WORST), one significant digit up.  The factor 4 covers the device's expf / tanhf, a few ulp off numpy's, and another
summation order.  tests/test_att_kernels_ref.py re-measures the figures on every run: every case must stay inside BOUND and
the worst figure within 0.5 .. 1.5 x the recorded one.  Measured from the restatements alone:
    CIM              out      P        ddense
      worst          3.66e-7  9.19e-7  1.11e-7
      BOUND          2e-6     4e-6     5e-7
    matching, small  A        P        TH       DZ       dQ       dE
      worst          7.62e-8  4.81e-8  6.48e-7  2.54e-7  3.35e-7  9.90e-8
      BOUND          4e-7     2e-7     3e-6     2e-6     2e-6     4e-7
    matching, sat    A        P        TH       DZ       dQ       dE
      worst          1.08e-7  4.15e-8  1.77e-6  3.60e-7  4.15e-7  9.86e-8
      BOUND          5e-7     2e-7     8e-6     2e-6     2e-6     4e-7
    edge attention   norm     dS
      worst          8.95e-7  1.38e-5
      BOUND          4e-6     6e-5
Quantities without arithmetic are compared bit for bit: the zero arm of CIM's mask, the zeroed capacity rows, the zero dS
columns of absent sources, every prefill.
"""
import functools
import math

import numpy as np

PAIR_X = (0, 1, 2, 2, 0, 1)      # av va ta tv at vt over the dense blocks a = 0, v = 1, t = 2
PAIR_Y = (1, 0, 0, 1, 2, 2)
LEAK = float(np.float32(1e-10))  # the out-of-window mask value, as the float32 the reference holds
NSCAL = 110                      # columns of S / dS the edge attention owns


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def rel(a, b, terms=None):
    """max |a - b| / max |b|; where b vanishes identically, over max |terms| (the terms that cancel in b) if given"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if b.size == 0:
        return 0.0
    scale = float(np.abs(b).max())
    if scale == 0 and terms is not None:
        scale = float(np.abs(terms).max())
    return float(np.abs(a - b).max() / max(scale, 1e-30))


def blocks(d):
    """the [L, L] blocks of a {key: block} save, one flat vector in key order"""
    return np.concatenate([np.asarray(d[k], np.float64).ravel() for k in sorted(d)]) if d else np.zeros(0)


# ===================================================================================================== CIM
def _cim(dt, dense, lens, G, Gd, mask_scale):
    dense, G = np.asarray(dense, dt), np.asarray(G, dt)
    dd = np.array(Gd, dt)                      # the classifier's gradient is there first; the pairs add to it in order
    out = np.zeros((dense.shape[0], 600), dt)
    P, off = {}, offsets(lens)
    for b, L in enumerate(lens):
        r = slice(off[b], off[b] + L)
        for p in range(6 if L else 0):
            cx, cy = 100 * PAIR_X[p], 100 * PAIR_Y[p]
            x, y, g = dense[r, cx:cx + 100], dense[r, cy:cy + 100], G[r, 100 * p:100 * p + 100]
            s = x @ y.T
            e = np.exp(s - s.max(1, keepdims=True))
            pm = e / e.sum(1, keepdims=True)
            h = pm @ y
            out[r, 100 * p:100 * p + 100] = h * x
            dh = g * x
            q = pm * (dh @ y.T)
            ds = q - pm * q.sum(1, keepdims=True)
            dd[r, cx:cx + 100] += g * h + ds @ y
            dd[r, cy:cy + 100] += pm.T @ dh + ds.T @ x
            P[p, b] = pm
    masked = np.where(dense > 0, dd * dt(mask_scale), dt(0))
    return dict(out=out, P=P, ddense_unmasked=dd, ddense=masked)


def cim(dense, lens, G, Gd, mask_scale):
    """float64.  dense [N, 300] = a | v | t, G [N, 600] the gradient of the six outputs, Gd [N, 300] what dmerged[:, 600:900)
    holds before the launch -> out [N, 600], P {(pair, slot): [L, L]}, ddense_unmasked, ddense [N, 300]"""
    return _cim(np.float64, dense, lens, G, Gd, mask_scale)


def cim_f32(dense, lens, G, Gd, mask_scale):
    return _cim(np.float32, dense, lens, G, Gd, mask_scale)


def _cc(name, lens, T, mask_scale, dead=0, exact=None):
    return dict(name=name, lens=list(lens), T=T, mask_scale=float(np.float32(mask_scale)), dead=dead, exact=exact)


# lens: one entry per dialogue SLOT (0 = an empty slot of a capacity launch); T: the launch's T (Pbuf and LDS pitch);
# dead: rows between N and n_cap; exact: the case holding the same dialogues as an exact launch
CIM_CASES = [
    _cc("L1", [1], 1, 1.0),
    _cc("L64-65", [64, 65], 65, 1.0 / (1.0 - 0.3)),
    _cc("L118", [118], 118, 2.0),
    _cc("L110-2-17", [110, 2, 17], 110, 1.0 / (1.0 - 0.3)),
    _cc("L7-65", [7, 65], 65, 2.0),
    _cc("cap-5x118", [0, 7, 0, 65, 0], 118, 2.0, dead=5, exact="L7-65"),
    _cc("L3-40", [3, 40], 40, 1.0 / (1.0 - 0.3)),
    _cc("cap-T118-3-40", [3, 0, 40], 118, 1.0 / (1.0 - 0.3), dead=3, exact="L3-40"),
]
CIM_CASE = {c["name"]: c for c in CIM_CASES}


def _dialogue_seed(c, CASE):
    """a capacity case shares the inputs of its exact twin: the seed is the twin's"""
    base = CASE[c["exact"]] if c.get("exact") else c
    return base["name"]


@functools.lru_cache(maxsize=None)
def cim_reference(name):
    """inputs (float32) and the float64 result of a case; computed once, never changed"""
    c = CIM_CASE[name]
    seed = 100 + [k["name"] for k in CIM_CASES].index(_dialogue_seed(c, CIM_CASE))
    r = np.random.RandomState(seed)
    live = [L for L in c["lens"] if L]
    N = sum(live)
    dense = (0.65 * (1.0 - r.rand(N, 300))).astype(np.float32)
    dense[r.rand(N, 300) < 0.5] = 0.0
    if len(live) > 1:                            # the second non-empty dialogue: nothing of v survived
        dense[live[0]:live[0] + live[1], 100:200] = 0.0
    G = r.randn(N, 600).astype(np.float32)
    Gd = r.randn(N, 300).astype(np.float32)
    return dict(c=c, N=N, dense=dense, G=G, Gd=Gd, out=cim(dense, c["lens"], G, Gd, c["mask_scale"]))


def cim_figures(got, ref):
    return dict(out=rel(got["out"], ref["out"]), P=rel(blocks(got["P"]), blocks(ref["P"])), ddense=rel(got["ddense"], ref["ddense"]))


def cim_f32_figures(name):
    R = cim_reference(name)
    return cim_figures(cim_f32(R["dense"], R["c"]["lens"], R["G"], R["Gd"], R["c"]["mask_scale"]), R["out"])


# ===================================================================================================== matching attention
def _match(dt, E, Q, dA, lens):
    E, Q, dA = np.asarray(E, dt), np.asarray(Q, dt), np.asarray(dA, dt)
    A, dQ, dE = np.zeros_like(E), np.zeros_like(E), np.zeros_like(E)
    dQ_terms = np.zeros_like(E)
    P, TH, DZ, DZ_terms, off = {}, {}, {}, {}, offsets(lens)
    for b, L in enumerate(lens):
        if L == 0:
            continue
        r = slice(off[b], off[b] + L)
        e, q, g = E[r], Q[r], dA[r]
        th = np.tanh(q @ e.T)
        x = np.exp(th)
        p = x / x.sum(1, keepdims=True)
        A[r] = p @ e
        dp = g @ e.T
        dz = p * (dp - (p * dp).sum(1, keepdims=True)) * (1 - th * th)
        dQ[r] = dz @ e
        dE[r] = p.T @ g + dz.T @ q
        P[b], TH[b], DZ[b] = p, th, dz
        DZ_terms[b] = p * np.abs(dp) * (1 - th * th)
        dQ_terms[r] = DZ_terms[b] @ np.abs(e)
    return dict(A=A, dQ=dQ, dE=dE, P=P, TH=TH, DZ=DZ, DZ_terms=DZ_terms, dQ_terms=dQ_terms)


def match(E, Q, dA, lens):
    """float64.  E, Q, dA [N, F] compact -> A, dQ, dE [N, F] and P, TH, DZ {slot: [L, L]}.  DZ_terms = p |dp| (1 - th^2) and
    dQ_terms = DZ_terms |E| are the terms that cancel in DZ and dQ: the scale of those two groups where the reference is 0
    identically (a case of one-row dialogues: a softmax over one key passes no gradient to the scores)"""
    return _match(np.float64, E, Q, dA, lens)


def match_f32(E, Q, dA, lens):
    return _match(np.float32, E, Q, dA, lens)


MATCH_LENS = [110, 1, 37, 64, 65, 16, 17, 2]
SAT_RANGE = 3.75
MATCH_GROUPS = ("A", "P", "TH", "DZ", "dQ", "dE")


def _mc(name, F, lens, T, tail=None, exact=None, scale="small"):
    return dict(name="%s-%s" % (name, scale), F=F, lens=list(lens), T=T, scale=scale, tail=tail,
                exact=None if exact is None else "%s-%s" % (exact, scale))


# tail: None = erc_match_att_bwd; k >= 0 = erc_match_att_bwd_cap with n_cap = N + k.  Pitches: `match_pitches`.
MATCH_CASES = [_mc(*a, scale=s) for s in ("small", "sat") for a in (
    ("F200-ragged", 200, MATCH_LENS, 110),
    ("F300-ragged", 300, MATCH_LENS, 110),
    ("F200-one", 200, [1], 1),
    ("F300-one", 300, [1], 1),
    ("F200-16-65-1", 200, [16, 65, 1], 65),
    ("F200-cap-tail37", 200, [0, 16, 0, 65, 1, 0], 110, 37, "F200-16-65-1"),
    ("F200-cap-tail0", 200, [0, 16, 0, 65, 1, 0], 110, 0, "F200-16-65-1"),
    ("F200-cap-tail1", 200, [0, 16, 0, 65, 1, 0], 110, 1, "F200-16-65-1"),
)]
MATCH_CASE = {c["name"]: c for c in MATCH_CASES}


def match_pitches(F):
    """all different, all above F, all multiples of 4"""
    return dict(lde=F + 4, ldq=F + 8, lda=F + 12, ldda=F + 16, lddq=F + 20, ldde=F + 24)


@functools.lru_cache(maxsize=None)
def match_reference(name):
    c = MATCH_CASE[name]
    base = MATCH_CASE[c["exact"]] if c["exact"] else c
    r = np.random.RandomState(200 + [k["name"] for k in MATCH_CASES].index(base["name"]))
    live = [L for L in c["lens"] if L]
    N, F = sum(live), c["F"]
    E = (0.1 * r.randn(N, F)).astype(np.float32)
    Q = (0.1 * r.randn(N, F)).astype(np.float32)
    dA = r.randn(N, F).astype(np.float32)
    if c["scale"] == "sat":
        off = offsets(live)
        for b, L in enumerate(live):
            want = r.uniform(-SAT_RANGE, SAT_RANGE, (L, L))
            Q[off[b]:off[b] + L] = (want @ np.linalg.pinv(E[off[b]:off[b] + L].astype(np.float64)).T).astype(np.float32)
    return dict(c=c, N=N, E=E, Q=Q, dA=dA, out=match(E, Q, dA, c["lens"]))


def match_figures(got, ref):
    fig = {k: rel(got[k], ref[k], ref["dQ_terms"] if k == "dQ" else None) for k in ("A", "dQ", "dE") if k in got}
    fig.update({k: rel(blocks(got[k]), blocks(ref[k]), blocks(ref["DZ_terms"]) if k == "DZ" else None) for k in ("P", "TH", "DZ") if k in got})
    return fig


def match_f32_figures(name):
    R = match_reference(name)
    return match_figures(match_f32(R["E"], R["Q"], R["dA"], R["c"]["lens"]), R["out"])


# ===================================================================================================== edge attention
def window(j, L, wp, wf):
    return (0 if wp < 0 else max(0, j - wp)), (L if wf < 0 else min(L, j + wf + 1))


def edge_lists(lens, wp, wf):
    """the window graph of compact nodes (slot b, position t -> node offsets[b] + t): src, dst [E] in in-CSR order (by
    destination, then source: an edge's id is its index here), and the out-CSR the kernels walk: out_ptr [N + 1], out_dst,
    out_eid [E] (by source, then destination)"""
    off = offsets(lens)
    pairs = []
    for b, L in enumerate(lens):
        for j in range(L):
            lo, hi = window(j, L, wp, wf)
            pairs += [(off[b] + j, off[b] + i) for i in range(lo, hi)]
    N = int(off[-1])
    if not pairs:
        z = np.zeros(0, np.int32)
        return dict(src=z, dst=z, out_ptr=np.zeros(N + 1, np.int32), out_dst=z, out_eid=z, n_nodes=N)
    pairs = np.array(pairs, np.int64)
    by_dst = np.lexsort((pairs[:, 0], pairs[:, 1]))
    src, dst = pairs[by_dst, 0], pairs[by_dst, 1]
    by_src = np.lexsort((dst, src))
    out_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))])
    return dict(src=src.astype(np.int32), dst=dst.astype(np.int32), out_ptr=out_ptr.astype(np.int32),
                out_dst=dst[by_src].astype(np.int32), out_eid=by_src.astype(np.int32), n_nodes=N)


def _edge(dt, S, lens, T, wp, wf, g, dn):
    """S [T, B, >= 110]; dn [E] by edge id -> norm [E], dS [T, B, 110]"""
    S, dn = np.asarray(S, dt), np.asarray(dn, dt)
    B = S.shape[1]
    norm, dS = np.zeros(len(g["src"]), dt), np.zeros((T, B, NSCAL), dt)
    off, leak = offsets(lens), dt(LEAK)
    t = np.arange(T)
    for b, L in enumerate(lens):
        for j in range(L):
            col = S[:T, b, j]
            u = np.exp(col - col.max())
            lo, hi = window(j, L, wp, wf)
            inw = (t >= lo) & (t < hi)
            den = u[inw].sum() + leak * u[~inw].sum()
            n = u / den
            k = slice(g["out_ptr"][off[b] + j], g["out_ptr"][off[b] + j + 1])
            i, eid = g["out_dst"][k] - off[b], g["out_eid"][k]
            norm[eid] = n[i]
            d = np.zeros(T, dt)
            d[i] = dn[eid]
            dot = (d * n)[inw].sum()
            dS[:, b, j] = np.where(inw, n * (d - dot), -leak * n * dot)
    return dict(norm=norm, dS=dS)


def edge(S, lens, T, wp, wf, g, dn):
    return _edge(np.float64, S, lens, T, wp, wf, g, dn)


def edge_f32(S, lens, T, wp, wf, g, dn):
    return _edge(np.float32, S, lens, T, wp, wf, g, dn)


WINDOWS = [(10, 10), (-1, -1), (0, 0), (-1, 3), (2, -1), (40, 40)]
EDGE_LENS = [("ragged", [110, 1, 65, 64, 13], 110), ("one", [1], 1), ("slots", [0, 9, 0, 70], 110)]
_FORMS = [(110, 1), (112, 3), (110, 3), (112, 1)]      # (ldS, dn_parts), every combination in turn
EDGE_CASES = [dict(name="%s-w%d_%d" % (ln, wp, wf), lens=lens, T=T, wp=wp, wf=wf, ldS=_FORMS[(3 * wi + li) % 4][0],
                   dn_parts=_FORMS[(3 * wi + li) % 4][1])
              for wi, (wp, wf) in enumerate(WINDOWS) for li, (ln, lens, T) in enumerate(EDGE_LENS)]
EDGE_CASE = {c["name"]: c for c in EDGE_CASES}


@functools.lru_cache(maxsize=None)
def edge_reference(name):
    """S [T, B, ldS] float32 (pad columns NaN), the edges, dnorm as dn_parts float32 vectors dn_stride apart (NaN behind the
    edges) and the float64 result of their sum"""
    c = EDGE_CASE[name]
    r = np.random.RandomState(300 + [k["name"] for k in EDGE_CASES].index(name))
    lens, T, B = c["lens"], c["T"], len(c["lens"])
    S = np.full((T, B, c["ldS"]), np.nan, np.float32)
    S[:, :, :NSCAL] = r.randn(T, B, NSCAL)
    for b, L in enumerate(lens):
        S[L:, b, :NSCAL] += 25.0                 # padded positions: exp(25) * 1e-10 is not negligible
    b0 = int(np.argmax(np.array(lens) > 0))      # out of source 0's window, inside the dialogue
    if c["wf"] >= 0:
        S[c["wf"] + 1:lens[b0], b0, 0] += 24.0
    g = edge_lists(lens, c["wp"], c["wf"])
    n_e = len(g["src"])
    stride = n_e + 5
    parts = np.full((c["dn_parts"], stride), np.nan, np.float32)
    parts[:, :n_e] = r.randn(c["dn_parts"], n_e)
    dn = parts[:, :n_e].astype(np.float64).sum(0)
    return dict(c=c, S=S, g=g, n_e=n_e, parts=parts, stride=stride, dn=dn, out=edge(S[:, :, :NSCAL], lens, T, c["wp"], c["wf"], g, dn))


def edge_figures(got, ref):
    return {k: rel(got[k], ref[k]) for k in ("norm", "dS") if k in got}


def edge_f32_figures(name):
    R = edge_reference(name)
    c = R["c"]
    dn32 = np.zeros(R["n_e"], np.float32)
    for q in range(c["dn_parts"]):               # the kernel's own order of adding the parts
        dn32 = dn32 + R["parts"][q, :R["n_e"]]
    return edge_figures(edge_f32(R["S"][:, :, :NSCAL], c["lens"], c["T"], c["wp"], c["wf"], R["g"], dn32), R["out"])


# ===================================================================================================== erc_dgcnv2_meta
def dgcnv2_meta(onehot, lengths, B, T, n_cap):
    """spk int64 [T * B]: the first index whose entry equals 1, 0 if none; node_row {index: t * B + b} of the first n_cap nodes,
    every length clamped to [0, T]"""
    oh = np.asarray(onehot).reshape(T * B, -1)
    spk = np.where((oh == 1).any(1), (oh == 1).argmax(1), 0).astype(np.int64)
    rows = [t * B + b for b in range(B) for t in range(int(min(max(int(lengths[b]), 0), T)))]
    return spk, np.array(rows[:n_cap], np.int32), len(rows)


# ===================================================================================================== bounds
# worst err / scale of the float32 twins over each family's cases, measured from the restatements alone
F32_WORST = dict(
    cim=dict(out=3.66e-7, P=9.19e-7, ddense=1.11e-7),
    match_small=dict(A=7.62e-8, P=4.81e-8, TH=6.48e-7, DZ=2.54e-7, dQ=3.35e-7, dE=9.90e-8),
    match_sat=dict(A=1.08e-7, P=4.15e-8, TH=1.77e-6, DZ=3.60e-7, dQ=4.15e-7, dE=9.86e-8),
    edge=dict(norm=8.95e-7, dS=1.38e-5))


def _one_digit_up(x):
    e = math.floor(math.log10(x))
    return float("%de%d" % (math.ceil(x / 10 ** e - 1e-9), e))


BOUND = {fam: {k: (_one_digit_up(4 * v) if v > 0 else 0.0) for k, v in w.items()} for fam, w in F32_WORST.items()}


def measure():
    """{family: {group: worst figure of the float32 twin over the family's cases}}"""
    def worst(figs):
        return {k: max(f[k] for f in figs) for k in figs[0]}
    return dict(cim=worst([cim_f32_figures(c["name"]) for c in CIM_CASES]),
                match_small=worst([match_f32_figures(c["name"]) for c in MATCH_CASES if c["scale"] == "small"]),
                match_sat=worst([match_f32_figures(c["name"]) for c in MATCH_CASES if c["scale"] == "sat"]),
                edge=worst([edge_f32_figures(c["name"]) for c in EDGE_CASES]))


if __name__ == "__main__":
    for fam, w in measure().items():
        print(fam, " ".join("%s=%.2e" % kv for kv in w.items()))
