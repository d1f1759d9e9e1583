"""GPU: erc_lstm_scan_fwd / _bwd / _bwd_cap (csrc/lstm.hip) through the C ABI on random hoisted products, in every launch
form -- unpacked padded rows time-major and batch-major, packed (lengths) on both, compact rows (node_off) without and with
lengths and a slot of length 0 -- against the float64 chain of tests/rnn_scan_ref.py.  Every tensor of the contract is
compared (Hout, Hdrop, the saved gates / Cst / Hprev, dGX and the weight-gradient products formed from the kernel's own dGX
and Hprev), every buffer is NaN beforehand so that what a form must not write is seen, the dropout mask is predicted
element by element, and a second backward run is bit-identical.  Pitches are wider than the payload (ldgx 816, ldh = lddh
208, ldhd 216).  The lengths are set by the chunk arithmetic of the scans (8 steps forward, pairs of chunks backward).

TOLERANCES (TOL below; tests/test_rnn_scan_ref.py recomputes the table without a GPU).  Yardstick: the reference in float32
on the CPU (one thread; float32 sums and activations in the machine-independent form of rnn_scan_ref.ops) against itself in
float64, per case and class as max|x32 - x64| / max|x64| of the worst tensor of the class.  The bound is 4 x that, rounded up
to one significant digit.  Classes: forward outputs and saves | gate gradients | weight-gradient products.  Yardsticks:
    edges       1.44e-7  1.62e-7  1.79e-7        unpacked1   9.76e-8  6.19e-8  9.75e-8
    edges0      1.60e-7  1.31e-7  1.54e-7        unpacked8   1.35e-7  1.13e-7  1.72e-7
    b1          1.28e-7  1.21e-7  1.38e-7        unpacked9   1.42e-7  1.08e-7  1.64e-7
    workload    1.24e-7  1.50e-7  3.35e-7        unpacked16  1.05e-7  9.25e-8  1.67e-7
    long        1.33e-7  1.42e-7  2.09e-7        unpacked17  1.20e-7  1.31e-7  1.33e-7
                                                 unpacked33  1.60e-7  1.66e-7  1.95e-7
Sensitivity, reference alone on the CPU (float64, `edges`; relative change of the worst tensor of the class, and that as a
multiple of the bound) for (a) c_{t-1} taken as 0 at steps s % 8 == 0, s > 0, (b) the reverse direction of a packed dialogue
starting at T - 1 instead of L - 1, (c) gates f and o exchanged:
    (a)  fwd=6.06e-1 (1.0e6 x)  dgate=5.08e-1 (7.3e5 x)  wgrad=2.95e-1 (3.7e5 x)
    (b)  fwd=7.79e-1 (1.3e6 x)  dgate=1.89e-1 (2.7e5 x)  wgrad=2.89e-1 (3.6e5 x)
    (c)  fwd=6.60e-1 (1.1e6 x)  dgate=5.24e-1 (7.5e5 x)  wgrad=3.54e-1 (4.4e5 x)
The kernels on an MI355X (worst form and dropout setting of each case; error and its multiple of the yardstick; the bound is
4 x).  The forward class carries the hardware exp2 / rcp activations of rnn100_dev.h (< 3e-7 absolute):
    edges       2.82e-7 (1.96)  2.10e-7 (1.30)  3.03e-7 (1.69)
    edges0      3.44e-7 (2.14)  1.84e-7 (1.41)  2.72e-7 (1.77)
    b1          3.07e-7 (2.39)  1.58e-7 (1.30)  2.60e-7 (1.88)
    workload    3.55e-7 (2.86)  2.00e-7 (1.33)  2.99e-7 (0.89)
    long        3.38e-7 (2.54)  1.90e-7 (1.34)  2.92e-7 (1.40)
    unpacked1   3.10e-7 (3.18)  1.74e-7 (2.82)  1.68e-7 (1.72)
    unpacked8   3.79e-7 (2.81)  1.90e-7 (1.69)  2.94e-7 (1.70)
    unpacked9   2.93e-7 (2.06)  1.87e-7 (1.73)  3.12e-7 (1.90)
    unpacked16  3.14e-7 (3.00)  1.40e-7 (1.51)  3.65e-7 (2.19)
    unpacked17  2.69e-7 (2.25)  2.19e-7 (1.68)  2.69e-7 (2.02)
    unpacked33  2.75e-7 (1.72)  1.97e-7 (1.19)  3.14e-7 (1.60)
The file takes 7 s on an MI355X box, most of it the references on the CPU (`workload` 1.2 s, `long` 0.9 s, `edges` 0.6 s).
"""
import functools
import math

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests import rnn_scan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, G4 = 100, 400
LDGX, LDH, LDHD = 816, 208, 216

# 4 x the float32 yardstick, one significant digit up: (forward outputs and saves, gate gradients, weight-gradient products)
TOL = {
    "edges": (6e-07, 7e-07, 8e-07),
    "edges0": (7e-07, 6e-07, 7e-07),
    "b1": (6e-07, 5e-07, 6e-07),
    "workload": (5e-07, 7e-07, 2e-06),
    "long": (6e-07, 6e-07, 9e-07),
    "unpacked1": (4e-07, 3e-07, 4e-07),
    "unpacked8": (6e-07, 5e-07, 7e-07),
    "unpacked9": (6e-07, 5e-07, 7e-07),
    "unpacked16": (5e-07, 4e-07, 7e-07),
    "unpacked17": (5e-07, 6e-07, 6e-07),
    "unpacked33": (7e-07, 7e-07, 8e-07),
}

RUNS = ([("edges", f) for f in ("packed_bm", "packed_tm", "compact")] + [("edges0", "compact_len")]
        + [("unpacked%d" % T, f) for T in R.UNPACKED_T for f in ("time_major", "batch_major")]
        + [("b1", f) for f in ("time_major", "batch_major", "packed_bm", "compact", "compact_len")]
        + [("workload", f) for f in ("packed_bm", "compact")] + [("long", f) for f in ("time_major", "packed_tm")])


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
    """the buffers of one case in one form; every output and saved buffer NaN, GX NaN outside its 800 columns and on rows
    no position owns, the upstream gradient random on every row a position owns (padded ones included)"""

    def __init__(self, name, form, p, rng, rng_stream, spare=R.SPARE):
        self.c = c = R.make_case(name)
        self.form, self.p, self.rng_stream = form, p, rng_stream
        B, T = c["B"], c["T"]
        n_rows, self.run, self.rows, self.sb, self.st, lengths, node_off = R.layout(form, B, T, c["lens"])
        self.n_rows = n_rows = n_rows - R.SPARE + spare if node_off is not None else n_rows
        self.valid = torch.arange(T)[None, :] < torch.tensor(self.run)[:, None]
        has_row = self.rows >= 0
        self.written = torch.zeros(n_rows, dtype=torch.bool)
        self.written[self.rows[self.valid]] = True
        GX, up = torch.full((n_rows, LDGX), float("nan")), torch.full((n_rows, LDH), float("nan"))
        GX[self.rows[has_row], :2 * G4] = c["GX"][has_row]
        up[self.rows[has_row], :2 * H] = c["up"][has_row]
        dev = lambda t: None if t is None else t.to(DEV)
        self.GX, self.up, self.W, self.b, self.lengths, self.node_off = (dev(t) for t in (GX, up, c["W_hh"], c["b_hh"], lengths, node_off))
        self.rng = torch.tensor(list(rng), dtype=torch.int64, device=DEV) if p > 0 else None
        self.keep_scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))

    def fwd(self, rng_stream=None):
        n, c = self.n_rows, self.c
        o = dict(Hout=_nan(n, LDH), Hdrop=_nan(n, LDHD) if self.p > 0 else None, gates=_nan(n, 2 * G4), Cst=_nan(n, 2 * H),
                 Hprev=_nan(n, 2 * H))
        capi.lstm_scan_fwd(self.GX, LDGX, self.W, self.b, self.lengths, self.node_off, self.sb, self.st, c["B"], c["T"], o["Hout"], LDH,
                           o["Hdrop"], LDHD if self.p > 0 else 0, self.p, self.rng, self.rng_stream if rng_stream is None else rng_stream,
                           o["gates"], o["Cst"], o["Hprev"])
        torch.cuda.synchronize()
        return o

    def bwd(self, o, zero_to=0):
        dGX = _nan(self.n_rows, 2 * G4)
        capi.lstm_scan_bwd(self.W, self.lengths, self.node_off, self.sb, self.st, self.c["B"], self.c["T"], o["gates"], o["Cst"], self.up,
                           LDH, self.p, self.rng, self.rng_stream, dGX, zero_to=zero_to)
        torch.cuda.synchronize()
        return dGX

    def positions(self, buf, w):
        """[B, T, w] float64 from the rows of a buffer, zero where the dialogue does not run"""
        out = torch.zeros(self.c["B"], self.c["T"], w, dtype=torch.float64)
        out[self.valid] = buf[self.rows[self.valid], :w].double()
        return out


def _run_case(name, form, p, rng=(3, 1234), rng_stream=0x77):
    ln = _Launch(name, form, p, rng, rng_stream)
    c, written, valid, drop = ln.c, ln.written, ln.valid, p > 0
    pad = ~written
    o = ln.fwd()
    cpu = {k: v.cpu() for k, v in o.items() if v is not None}
    saved = {k: o[k].clone() for k in ("gates", "Cst")}
    dGX_dev = ln.bwd(o)
    cpu["dGX"] = dGX_dev.cpu()
    # ---- write discipline
    for k in ("gates", "Cst"):
        assert _same_bits(o[k], saved[k]), "the backward changed " + k
    outs = ("Hout", "Hdrop", "dGX") if drop else ("Hout", "dGX")
    width = {"Hout": 2 * H, "Hdrop": 2 * H, "dGX": 2 * G4}
    for k, v in cpu.items():
        w = width.get(k, v.shape[1])
        assert torch.isfinite(v[written, :w]).all(), k
        assert torch.isnan(v[:, w:]).all(), k + ": columns beyond the payload"
        if ln.node_off is None and k in outs:
            assert bool((v[pad, :w] == 0).all()), k + ": padded positions"
        else:                                      # saved state of padded positions; every buffer's rows no dialogue owns
            assert torch.isnan(v[pad]).all(), k + ": rows that are not run"
    assert int(pad.sum()) == (R.SPARE if ln.node_off is not None else c["B"] * c["T"] - int(valid.sum()))
    for b in range(c["B"]):
        if ln.run[b] > 0:
            first, last = ln.rows[b, 0], ln.rows[b, ln.run[b] - 1]
            assert float(cpu["Hprev"][first, :H].abs().max()) == 0.0 and float(cpu["Hprev"][last, H:].abs().max()) == 0.0
    # ---- dropout: the mask element by element
    got = {k: ln.positions(cpu[k], width.get(k, cpu[k].shape[1])) for k in cpu}
    mask = None
    if drop:
        live = valid[:, :, None] & (got["Hout"] != 0)
        kept = got["Hdrop"] != 0
        want = R.drop_mask(c, form, p, rng, rng_stream)
        assert torch.equal(kept[live], want[live])
        assert torch.allclose(got["Hdrop"][kept], (got["Hout"] / (1.0 - p))[kept], rtol=1e-6, atol=0)
        n = int(live.sum())
        assert abs(float(kept[live].double().mean()) - (1.0 - p)) <= 4.0 * math.sqrt(p * (1.0 - p) / n), n
        if n >= 2000:
            assert not torch.equal(kept[..., :H][live[..., :H]], kept[..., H:][live[..., H:]])
        other = ln.fwd(rng_stream ^ 0x10)
        kept2 = ln.positions(other["Hdrop"].cpu(), 2 * H) != 0
        assert torch.equal(kept2[live], R.drop_mask(c, form, p, rng, rng_stream ^ 0x10)[live])
        assert n < 2000 or not torch.equal(kept2[live], kept[live])
        assert _same_bits(other["Hout"], o["Hout"])
        mask = kept.double() * ln.keep_scale       # the backward must have used the mask the forward applied
    # ---- every tensor of the contract against float64
    ref = R.reference(c, mask=mask, run=ln.run)
    got.update(R.contract_products(got["dGX"], got["dGX"], got["Hprev"], c["X"].double(), G4, H))
    err, yard = R.class_errors(got, ref), _yardstick(name)
    print("lstm %s %s p=%g: %s" % (name, form, p, "  ".join("%s=%.3g (%.2f x yardstick)" % (k, err[k], err[k] / yard[k]) for k in R.CLASSES)))
    for i, k in enumerate(R.CLASSES):
        assert err[k] <= TOL[name][i], (k, err[k], TOL[name][i])
    # ---- a second backward run
    again = ln.bwd(o)
    assert _same_bits(again[written.to(DEV)], dGX_dev[written.to(DEV)])


@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("name,form", RUNS)
def test_lstm_scan_matches_the_float64_chain(name, form, drop):
    _run_case(name, form, 0.5 * drop)


@pytest.mark.parametrize("name,form", RUNS[:4])
def test_lstm_scan_dropout_with_another_rate_stream_and_offset(name, form):
    """p = 0.3, a non-zero offset rng[0] and another rng_stream"""
    _run_case(name, form, 0.3, rng=(11, 987654321), rng_stream=0x1234)


@pytest.mark.parametrize("name,extra", [("cap5", 13), ("edges", 4), ("cap5", 0)])
def test_lstm_scan_bwd_cap_zeroes_the_capacity_rows(name, extra):
    """erc_lstm_scan_bwd_cap (compact rows, dropout on), dGX of n + 20 NaN rows: zero_to = n + 13 with B = 5 (the tail is no
    multiple of B), n + 4 with B = 15 (fewer tail rows than workgroups), n (an empty tail): rows < n bit-identical to
    erc_lstm_scan_bwd on the same saves, rows [n, zero_to) exactly 0 in all 800 columns, rows >= zero_to still NaN"""
    ln = _Launch(name, "compact", 0.5, (3, 1234), 0x77, spare=20)
    n = ln.n_rows - 20
    assert n == sum(ln.c["lens"]) and bool(ln.written[:n].all()) and ln.c["B"] == (5 if name == "cap5" else 15)
    o = ln.fwd()
    exact, cap = ln.bwd(o), ln.bwd(o, zero_to=n + extra)
    assert torch.isfinite(exact[:n]).all() and torch.isnan(exact[n:]).all()
    assert _same_bits(cap[:n], exact[:n])
    assert bool((cap[n:n + extra] == 0).all())
    assert torch.isnan(cap[n + extra:]).all()


def test_lstm_scan_refuses_bad_arguments():
    """host checks that return before any launch"""
    f32 = lambda *s: torch.zeros(*s, device=DEV)
    B, T = 2, 4
    n = B * T
    GX, W, bh = f32(n, 800), f32(2, 400, 100), f32(2, 400)
    Hout, Hd, gates, Cst, Hp, dGX = f32(n, 200), f32(n, 200), f32(n, 800), f32(n, 200), f32(n, 200), f32(n, 800)
    rng = torch.tensor([0, 1], dtype=torch.int64, device=DEV)
    lengths = torch.tensor([4, 4], dtype=torch.int64, device=DEV)
    t_dev = torch.tensor([4], dtype=torch.int32, device=DEV)

    def fwd(**kw):
        a = dict(GX=GX, ldgx=800, B=B, T=T, ldh=200, Hdrop=None, ldhd=0, p=0.0, rng=None, gates=gates, lengths=None, t_dev=None)
        a.update(kw)
        capi.lstm_scan_fwd(a["GX"], a["ldgx"], W, bh, a["lengths"], None, 1, B, a["B"], a["T"], Hout, a["ldh"], a["Hdrop"], a["ldhd"],
                           a["p"], a["rng"], 0, a["gates"], Cst, Hp, t_dev=a["t_dev"])

    def bwd(**kw):
        a = dict(B=B, T=T, lddh=200, p=0.0, rng=None, dGX=dGX, zero_to=0, lengths=None, t_dev=None)
        a.update(kw)
        capi.lstm_scan_bwd(W, a["lengths"], None, 1, B, a["B"], a["T"], gates, Cst, Hout, a["lddh"], a["p"], a["rng"], 0, a["dGX"],
                           zero_to=a["zero_to"], t_dev=a["t_dev"])
    fwd()
    bwd()
    torch.cuda.synchronize()
    for kw, msg in ((dict(GX=None), "null pointer"), (dict(gates=None), "null pointer"), (dict(ldgx=799), "ldgx=799"),
                    (dict(ldh=199), "ldh=199"), (dict(B=0), "B=0"), (dict(T=0), "T=0"), (dict(Hdrop=Hd, ldhd=100), "ldhd=100"),
                    (dict(Hdrop=Hd, ldhd=200, p=0.5), "rng_state"), (dict(Hdrop=Hd, ldhd=200, p=1.0, rng=rng), "drop_p"),
                    (dict(Hdrop=Hd, ldhd=200, p=-0.1, rng=rng), "drop_p"), (dict(lengths=lengths, t_dev=t_dev), "t_dev is the unpacked")):
        with pytest.raises(capi.ErcGraftError, match=msg):
            fwd(**kw)
    for kw, msg in ((dict(dGX=None), "null pointer"), (dict(lddh=199), "lddh=199"), (dict(B=0), "B=0"), (dict(T=0), "T=0"),
                    (dict(p=0.5), "rng_state"), (dict(p=1.0, rng=rng), "drop_p"), (dict(p=-0.1, rng=rng), "drop_p"),
                    (dict(zero_to=5), "zero_to needs compact rows"), (dict(lengths=lengths, t_dev=t_dev), "t_dev is the unpacked")):
        with pytest.raises(capi.ErcGraftError, match=msg):
            bwd(**kw)
