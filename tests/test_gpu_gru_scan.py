"""GPU: erc_gru_scan_fwd / _bwd / _bwd_cap (csrc/gru.hip: the CIM encoders, hidden 200, three modalities x both directions
in one launch, compact rows) through the C ABI against the float64 chain of tests/rnn_scan_ref.py: different weights and GX
per modality, with and without the dropped copy, an empty slot, a launch with T shorter than a dialogue, more dialogues than
one wave of workgroups.  Every buffer has rows = N + 7 (the modality stride) and is NaN beforehand; every tensor of the
contract is compared (Hout, Hdrop, gates, ghn, Hprev, dGX, dGH, and per modality and direction the products dW_ih = dGX^T X,
db_ih, dW_hh = dGH^T Hprev, db_hh formed from the kernel's own gate gradients and Hprev).

TOLERANCES (TOL below; tests/test_rnn_scan_ref.py recomputes the table without a GPU).  Yardstick: the reference in float32
on the CPU (one thread; float32 sums and activations in the machine-independent form of rnn_scan_ref.ops) against itself in
float64, per case and class as max|x32 - x64| / max|x64| of the worst tensor and modality of the class; the bound is 4 x that,
rounded up to one significant digit.  Classes: forward outputs and saves | gate gradients | weight-gradient products.
Yardsticks:
    gru_ragged  2.28e-7  1.62e-7  2.08e-7      lengths 1, 110, 37, 5
    gru_empty   1.51e-7  1.50e-7  1.87e-7      lengths 3, 0, 8, 1
    gru_b33     2.18e-7  1.72e-7  2.36e-7      33 dialogues, lengths 1 .. 12
    gru_clamp   1.76e-7  1.76e-7  1.79e-7      lengths 12, 9 launched with T = 9
Sensitivity, reference alone on the CPU (float64, `gru_b33`; relative change of the worst tensor of the class, and that as a
multiple of the bound) for (d) b_hn outside r * (.):
    (d)  fwd=1.89e-1 (2.1e5 x)  dgate=3.84e-2 (5.5e4 x)  wgrad=1.34e-1 (1.3e5 x)
The kernels on an MI355X (worse dropout setting of each case; error and its multiple of the yardstick; the bound is 4 x).  The
forward class comes closest (the scan sums its 200 recurrent products in one float32 chain, the yardstick in a tree of
eights: a different order of summation is what the factor is for):
    gru_ragged  5.93e-7 (2.61)  2.28e-7 (1.40)  1.70e-7 (0.82)
    gru_empty   5.89e-7 (3.89)  2.05e-7 (1.37)  1.84e-7 (0.98)
    gru_b33     6.13e-7 (2.82)  2.05e-7 (1.19)  1.46e-7 (0.62)
    gru_clamp   4.97e-7 (2.82)  2.69e-7 (1.52)  2.41e-7 (1.35)
The file takes 5 s on an MI355X box (`gru_ragged` 1.8 s, nearly all of it the references on the CPU).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests import rnn_scan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, G3 = 200, 600
P, RNG, STREAM = 0.3, (5, 4321), 11

# 4 x the float32 yardstick, one significant digit up: (forward outputs and saves, gate gradients, weight-gradient products)
TOL = {
    "gru_ragged": (1e-06, 7e-07, 9e-07),
    "gru_empty": (7e-07, 6e-07, 8e-07),
    "gru_b33": (9e-07, 7e-07, 1e-06),
    "gru_clamp": (8e-07, 8e-07, 8e-07),
}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    return R.yardstick(R.make_case(name))


def _nan(*s):
    return torch.full(s, float("nan"), device=DEV)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class _Launch:
    """the buffers of one case: [3][rows = N + 7][.]; GX and the upstream gradient are NaN on every row that is not run"""

    def __init__(self, name, p):
        self.c = c = R.make_case(name)
        self.p = p
        B, Tc = c["B"], c["Tc"]
        n, _, self.rows, _, _, lengths, node_off = R.layout("compact_len", B, Tc, c["lens"])
        self.N = n - R.SPARE
        self.cap = self.N + 7
        self.valid = torch.arange(Tc)[None, :] < torch.tensor(c["run"])[:, None]
        self.written = torch.zeros(self.cap, dtype=torch.bool)
        self.written[self.rows[self.valid]] = True
        GX, up = torch.full((3, self.cap, 2 * G3), float("nan")), torch.full((3, self.cap, 2 * H), float("nan"))
        GX[:, self.rows[self.valid]] = c["GX"][:, self.valid]
        up[:, self.rows[self.valid]] = c["up"][:, self.valid]
        W = c["W_hh"].reshape(6, G3, H)
        self.GX, self.up, self.W, self.WT, self.b, self.lengths, self.node_off = (
            t.to(DEV) for t in (GX, up, W, W.transpose(1, 2).contiguous(), c["b_hh"].reshape(6, G3), lengths, node_off))
        self.rng = torch.tensor(list(RNG), dtype=torch.int64, device=DEV) if p > 0 else None
        self.keep_scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))

    def fwd(self):
        n, c = self.cap, self.c
        o = dict(Hout=_nan(3, n, 2 * H), Hdrop=_nan(3, n, 2 * H) if self.p > 0 else None, gates=_nan(3, n, 2 * G3), ghn=_nan(3, n, 2 * H),
                 Hprev=_nan(3, n, 2 * H))
        capi.gru_scan_fwd(self.GX, self.WT, self.b, self.lengths, self.node_off, c["B"], c["T"], n, o["Hout"], o["Hdrop"], self.p, self.rng,
                          STREAM, o["gates"], o["ghn"], o["Hprev"])
        torch.cuda.synchronize()
        return o

    def bwd(self, o, zero_to=None):
        n, c = self.cap, self.c
        dGX, dGH = _nan(3, n, 2 * G3), _nan(3, n, 2 * G3)
        args = (self.W, self.lengths, self.node_off, c["B"], c["T"], n, o["gates"], o["ghn"], o["Hprev"], self.up, self.p, self.rng, STREAM,
                dGX, dGH)
        if zero_to is None:
            capi.gru_scan_bwd(*args)
        else:
            capi.gru_scan_bwd_cap(*args, zero_to)
        torch.cuda.synchronize()
        return dGX, dGH

    def positions(self, buf):
        """[3, B, Tc, w] float64 from the rows of a buffer, zero where the dialogue does not run"""
        out = torch.zeros(3, self.c["B"], self.c["Tc"], buf.shape[-1], dtype=torch.float64)
        out[:, self.valid] = buf[:, self.rows[self.valid]].double()
        return out


@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("name", R.GRU_CASES)
def test_gru_scan_matches_the_float64_chain(name, drop):
    p = P * drop
    ln = _Launch(name, p)
    c, written, valid, N = ln.c, ln.written, ln.valid, ln.N
    if name == "gru_clamp":
        assert written.tolist() == [True] * 9 + [False] * 3 + [True] * 9 + [False] * 7      # rows 9 .. 11 belong to nobody's run
    o = ln.fwd()
    saved = {k: o[k].clone() for k in ("gates", "ghn", "Hprev")}
    dGX, dGH = ln.bwd(o)
    cpu = {k: v.cpu() for k, v in dict(o, dGX=dGX, dGH=dGH).items() if v is not None}
    # ---- write discipline: the rows that are run, nothing else (rows >= N, the clamped dialogue's last rows)
    for k in saved:
        assert _same_bits(o[k], saved[k]), "the backward changed " + k
    for k, v in cpu.items():
        assert torch.isfinite(v[:, written]).all() and torch.isnan(v[:, ~written]).all(), k
    for b in range(c["B"]):
        if c["run"][b] > 0:
            first, last = ln.rows[b, 0], ln.rows[b, c["run"][b] - 1]
            assert float(cpu["Hprev"][:, first, :H].abs().max()) == 0.0 and float(cpu["Hprev"][:, last, H:].abs().max()) == 0.0
    # ---- _bwd_cap: the same rows bit for bit, the tail rows [N, N + 5) written 0, the rest untouched
    cGX, cGH = ln.bwd(o, zero_to=N + 5)
    for cap, exact in ((cGX, dGX), (cGH, dGH)):
        assert _same_bits(cap[:, :N], exact[:, :N])
        assert bool((cap[:, N:N + 5] == 0).all()) and torch.isnan(cap[:, N + 5:]).all()
    # ---- dropout
    got = {k: ln.positions(v) for k, v in cpu.items()}
    mask = None
    if drop:
        live = valid[None, :, :, None] & (got["Hout"] != 0)
        kept = got["Hdrop"] != 0
        assert torch.equal(kept[live], R.drop_mask(c, "compact_len", p, RNG, STREAM)[live])
        assert torch.allclose(got["Hdrop"][kept], (got["Hout"] / (1.0 - p))[kept], rtol=1e-6, atol=0)
        parts = [kept[m][valid][:, d * H:(d + 1) * H] for m in range(3) for d in (0, 1)]
        assert all(not torch.equal(x, y) for x, y in itertools.combinations(parts, 2))
        mask = kept.double() * ln.keep_scale       # the backward must have used the mask the forward applied
    # ---- every tensor of the contract against float64
    ref = R.reference(c, mask=mask)
    got = [{k: v[m] for k, v in got.items()} for m in range(3)]
    for m in range(3):
        got[m].update(R.contract_products(got[m]["dGX"], got[m]["dGH"], got[m]["Hprev"], c["X"][m].double(), G3, H))
    err, yard = R.class_errors(got, ref), _yardstick(name)
    print("gru %s p=%g: %s" % (name, p, "  ".join("%s=%.3g (%.2f x yardstick)" % (k, err[k], err[k] / yard[k]) for k in R.CLASSES)))
    for i, k in enumerate(R.CLASSES):
        assert err[k] <= TOL[name][i], (k, err[k], TOL[name][i])
    # ---- a second backward run
    aGX, aGH = ln.bwd(o)
    assert _same_bits(aGX, dGX) and _same_bits(aGH, dGH)


def test_gru_scan_refuses_bad_arguments():
    """host checks that return before any launch"""
    f32 = lambda *s: torch.zeros(*s, device=DEV)
    B, T, n = 2, 4, 8
    GX, WT, W, bh = f32(3, n, 2 * G3), f32(6, H, G3), f32(6, G3, H), f32(6, G3)
    Hout, Hd, gates, ghn, Hp, dGX, dGH = f32(3, n, 2 * H), f32(3, n, 2 * H), f32(3, n, 2 * G3), f32(3, n, 2 * H), f32(3, n, 2 * H), \
        f32(3, n, 2 * G3), f32(3, n, 2 * G3)
    rng = torch.tensor([0, 1], dtype=torch.int64, device=DEV)
    lengths = torch.tensor([4, 4], dtype=torch.int64, device=DEV)
    node_off = torch.tensor([0, 4, 8], dtype=torch.int32, device=DEV)

    def fwd(**kw):
        a = dict(GX=GX, rows=n, Hdrop=None, p=0.0, rng=None, Hprev=Hp)
        a.update(kw)
        capi.gru_scan_fwd(a["GX"], WT, bh, lengths, node_off, B, T, a["rows"], Hout, a["Hdrop"], a["p"], a["rng"], 0, gates, ghn, a["Hprev"])

    def bwd(**kw):
        a = dict(W=W, rows=n, p=0.0, rng=None, dGH=dGH, zero_to=0)
        a.update(kw)
        capi.gru_scan_bwd_cap(a["W"], lengths, node_off, B, T, a["rows"], gates, ghn, Hp, Hout, a["p"], a["rng"], 0, dGX, a["dGH"],
                              a["zero_to"])
    fwd()
    bwd()
    bwd(zero_to=n)
    torch.cuda.synchronize()
    for kw, msg in ((dict(GX=None), "null pointer"), (dict(Hprev=None), "null pointer"), (dict(rows=0), "rows=0"),
                    (dict(Hdrop=Hd, p=0.3), "rng_state"), (dict(Hdrop=Hd, p=1.0, rng=rng), "drop_p")):
        with pytest.raises(capi.ErcGraftError, match=msg):
            fwd(**kw)
    for kw, msg in ((dict(W=None), "null pointer"), (dict(dGH=None), "null pointer"), (dict(rows=0), "rows=0"),
                    (dict(zero_to=n + 1), "zero_to"), (dict(p=0.3), "rng_state"), (dict(p=1.0, rng=rng), "drop_p")):
        with pytest.raises(capi.ErcGraftError, match=msg):
            bwd(**kw)
