"""GPU: erc_gru100_scan_fwd / _bwd (csrc/gru100.hip, the weight-stationary hidden-100 GRU scan) through the C-ABI on random
hoisted products against the float64 chain of tests/bcrnn_oracle.py, in every launch form: unpacked padded rows time-major
and batch-major, packed with lengths, compact rows with node_off; with and without the dropped copy Hdrop.

Bounds (the project's scan bounds, tests/test_gpu_dialogrnn.py): outputs < 1e-5 absolute; dGX, dGH and every weight gradient
formed from them <= 1e-4 of the reference's largest entry, for a random upstream gradient.  Rows and columns a form must not
write are filled with NaN beforehand and stay NaN; dGX / dGH are exactly zero on the padded rows of the packed form; a
second backward run is bit-identical.  Each case prints the kernel's output error as a multiple of the error of the same
chain evaluated in float32 on the CPU."""
import functools

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests import bcrnn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, G3, LDH, LDGX, DX = 100, 300, 208, 616, 16
FORMS = ("time_major", "batch_major", "packed", "compact")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _lens(B, T):
    if B == 1:
        return [T]
    g = torch.Generator().manual_seed(7 + B)
    lens = [int(v) for v in torch.randint(2, T + 1, (B,), generator=g)]
    lens[0], lens[1], lens[B - 1] = T, 1, T
    return lens


def _layout(form, B, T, lens):
    """-> (number of rows of every buffer, per dialogue: steps run, rows [steps] in time order; sb, st, lengths, node_off)"""
    if form == "compact":
        off = np.concatenate([[0], np.cumsum(lens)])
        rows = [torch.arange(int(off[b]), int(off[b]) + lens[b]) for b in range(B)]
        return int(off[-1]) + 5, lens, rows, 0, 0, None, torch.tensor(off, dtype=torch.int32)
    sb, st = (T, 1) if form == "batch_major" else (1, B)
    run = lens if form == "packed" else [T] * B
    rows = [b * sb + torch.arange(run[b]) * st for b in range(B)]
    return B * T, run, rows, sb, st, (torch.tensor(lens, dtype=torch.int64) if form == "packed" else None), None


def _close(got, ref, what):
    ref = ref.float()
    assert torch.isfinite(got).all(), what
    err = float((got - ref).abs().max())
    assert err <= 1e-4 * (float(ref.abs().max()) + 1e-12), (what, err, float(ref.abs().max()))


def _run_case(form, B, T, drop, seed):
    lens = _lens(B, T)
    n_rows, run, rows, sb, st, lengths, node_off = _layout(form, B, T, lens)
    g = torch.Generator().manual_seed(seed)
    W = (torch.rand(2, G3, H, generator=g) * 2 - 1) * 0.1
    bh = (torch.rand(2, G3, generator=g) * 2 - 1) * 0.1
    GX = torch.randn(n_rows, LDGX, generator=g) * 0.5
    X = torch.randn(n_rows, DX, generator=g)
    up = torch.randn(n_rows, LDH, generator=g)
    written = torch.zeros(n_rows, dtype=torch.bool)
    for r in rows:
        written[r] = True
    padded = ~written
    if form == "compact":
        padded[:] = False                          # rows past node_off[B] are not the scan's: they stay untouched
    elif form == "packed":
        pass                                       # positions >= L_b: zero outputs and zero gate gradients
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    dev = lambda t: None if t is None else t.to(DEV)
    Hout, Hdrop = nan(n_rows, LDH), (nan(n_rows, LDH) if drop else None)
    gates, ghn, Hprev = nan(n_rows, 2 * G3), nan(n_rows, 2 * H), nan(n_rows, 2 * H)
    rng = torch.tensor([3, 1234 + seed], dtype=torch.int64, device=DEV) if drop else None
    p = 0.5 if drop else 0.0
    Wd, bd, GXd, len_d, off_d = dev(W), dev(bh), dev(GX), dev(lengths), dev(node_off)
    capi.gru100_scan_fwd(GXd, LDGX, Wd, bd, len_d, off_d, sb, st, B, T, Hout, LDH, Hdrop, LDH if drop else 0, p, rng, 0x77,
                         gates, ghn, Hprev)
    torch.cuda.synchronize()
    # float64 chain (and the same chain in float32, the yardstick), dialogues of equal length batched
    W64, b64 = W.double().requires_grad_(), bh.double().requires_grad_()
    G64 = GX.double().requires_grad_()
    eps = torch.zeros(n_rows, 2 * G3, dtype=torch.float64, requires_grad=True)
    H_ref = torch.zeros(n_rows, 2 * H, dtype=torch.float64)
    H_f32 = torch.zeros(n_rows, 2 * H)
    groups = {}
    for b in range(B):
        groups.setdefault(run[b], []).append(b)
    for L, bs in groups.items():
        idx = torch.stack([rows[b] for b in bs], 1)                    # [L, n] rows in time order
        for d in (0, 1):
            ix = idx if d == 0 else idx.flip(0)
            h = O.gru_scan(G64[ix][..., d * G3:(d + 1) * G3], W64[d], b64[d], eps[ix][..., d * G3:(d + 1) * G3])
            H_ref = H_ref.index_put((ix.reshape(-1)[:, None], torch.arange(d * H, (d + 1) * H)[None, :]), h.reshape(-1, H))
            with torch.no_grad():
                h32 = O.gru_scan(GX[ix][..., d * G3:(d + 1) * G3], W[d], bh[d])
            H_f32[ix.reshape(-1), d * H:(d + 1) * H] = h32.reshape(-1, H)
    Hc = Hout.cpu()
    err = float((Hc[written, :2 * H] - H_ref.detach()[written].float()).abs().max())
    err32 = float((H_f32[written].double() - H_ref.detach()[written]).abs().max())
    print("gru100 %s B=%d T=%d drop=%d: |Hout - f64| = %.3g, float32 CPU chain %.3g, ratio %.2f"
          % (form, B, T, drop, err, err32, err / max(err32, 1e-30)))
    assert err < 1e-5
    # what must not be written stays NaN; padded positions of the packed form are zero
    assert torch.isnan(Hc[:, 2 * H:]).all()
    sv = {k: v.cpu() for k, v in (("gates", gates), ("ghn", ghn), ("Hprev", Hprev))}
    for k, v in sv.items():
        assert torch.isfinite(v[written]).all() and torch.isnan(v[~written]).all(), k
    assert bool((Hc[padded, :2 * H] == 0).all()) and torch.isnan(Hc[~written & ~padded]).all()
    # saved state against the chain: h_{t-1} in scan order is the neighbour's output
    for b in range(min(B, 3)):
        r = rows[b]
        assert float((sv["Hprev"][r[1:], :H] - H_ref.detach()[r[:-1], :H].float()).abs().max() if len(r) > 1 else 0.0) < 1e-5
        assert float((sv["Hprev"][r[:-1], H:] - H_ref.detach()[r[1:], H:].float()).abs().max() if len(r) > 1 else 0.0) < 1e-5
        assert float(sv["Hprev"][r[0], :H].abs().max()) == 0.0 and float(sv["Hprev"][r[-1], H:].abs().max()) == 0.0
    mask = torch.ones(n_rows, 2 * H, dtype=torch.float64)
    if drop:
        Hd = Hdrop.cpu()
        assert torch.isnan(Hd[:, 2 * H:]).all() and bool((Hd[padded, :2 * H] == 0).all())
        kept = Hd[written, :2 * H] != 0
        assert abs(float(kept.float().mean()) - 0.5) < 0.03
        assert torch.allclose(Hd[written, :2 * H][kept], (Hc[written, :2 * H] * 2.0)[kept], rtol=1e-6, atol=0)
        mask = torch.where(Hd[:, :2 * H] != 0, 2.0, 0.0).double()
    # backward: random upstream gradient on every row (the padded ones must be ignored)
    (H_ref * mask * up[:, :2 * H].double())[written].sum().backward()
    upd = up.to(DEV)

    def run_bwd():
        dGX, dGH = nan(n_rows, 2 * G3), nan(n_rows, 2 * G3)
        capi.gru100_scan_bwd(Wd, len_d, off_d, sb, st, B, T, gates, ghn, Hprev, upd, LDH, p, rng, 0x77, dGX, dGH)
        torch.cuda.synchronize()
        return dGX, dGH
    dGX, dGH = run_bwd()
    gx, gh = dGX.cpu(), dGH.cpu()
    assert bool((gx[padded] == 0).all()) and bool((gh[padded] == 0).all())
    assert torch.isnan(gx[~written & ~padded]).all() and torch.isnan(gh[~written & ~padded]).all()
    dgx_ref = torch.cat([G64.grad[:, :G3], G64.grad[:, G3:2 * G3]], -1)
    _close(gx[written], dgx_ref[written], "dGX")
    _close(gh[written], eps.grad[written], "dGH")
    gx64, gh64, hp64 = gx[written].double(), gh[written].double(), sv["Hprev"][written].double()
    _close((gx64.t() @ X[written].double()).float(), dgx_ref[written].t() @ X[written].double(), "dW_ih")
    _close(gx64.sum(0).float(), dgx_ref[written].sum(0), "db_ih")
    for d in (0, 1):
        _close((gh64[:, d * G3:(d + 1) * G3].t() @ hp64[:, d * H:(d + 1) * H]).float(), W64.grad[d], "dW_hh[%d]" % d)
        _close(gh64[:, d * G3:(d + 1) * G3].sum(0).float(), b64.grad[d], "db_hh[%d]" % d)
    dGX2, dGH2 = run_bwd()
    assert torch.equal(dGX[written.to(DEV)], dGX2[written.to(DEV)]) and torch.equal(dGH[written.to(DEV)], dGH2[written.to(DEV)])


@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("B", [1, 5, 32, 33])
@pytest.mark.parametrize("form", FORMS)
def test_gru100_scan_matches_the_float64_chain(form, B, drop):
    _run_case(form, B, 110, drop, 1000 * FORMS.index(form) + 10 * B + drop)


@pytest.mark.parametrize("form", ["time_major", "packed"])
def test_gru100_scan_has_no_limit_on_T(form):
    """T = 300: nothing of the history is kept on chip"""
    _run_case(form, 5, 300, 1, 77)


def test_gru100_scan_refuses_bad_arguments():
    f32 = lambda *s: torch.zeros(*s, device=DEV)
    B, T = 2, 4
    n = B * T
    GX, W, bh = f32(n, 600), f32(2, 300, 100), f32(2, 300)
    Hout, Hd, gates, ghn, Hp, dGX, dGH = f32(n, 200), f32(n, 200), f32(n, 600), f32(n, 200), f32(n, 200), f32(n, 600), f32(n, 600)
    rng = torch.tensor([0, 1], dtype=torch.int64, device=DEV)

    def fwd(**kw):
        a = dict(GX=GX, ldgx=600, W=W, b=bh, B=B, T=T, Hout=Hout, ldh=200, Hdrop=None, ldhd=0, p=0.0, rng=None, gates=gates)
        a.update(kw)
        capi.gru100_scan_fwd(a["GX"], a["ldgx"], a["W"], a["b"], None, None, 1, B, a["B"], a["T"], a["Hout"], a["ldh"], a["Hdrop"],
                             a["ldhd"], a["p"], a["rng"], 0, a["gates"], ghn, Hp)

    def bwd(**kw):
        a = dict(W=W, B=B, T=T, lddh=200, p=0.0, rng=None, dGH=dGH)
        a.update(kw)
        capi.gru100_scan_bwd(a["W"], None, None, 1, B, a["B"], a["T"], gates, ghn, Hp, Hout, a["lddh"], a["p"], a["rng"], 0, dGX,
                             a["dGH"])
    fwd()
    bwd()
    torch.cuda.synchronize()
    for kw, msg in ((dict(GX=None), "null"), (dict(gates=None), "null"), (dict(ldgx=599), "ldgx"), (dict(ldh=199), "ldh"),
                    (dict(B=0), "B=0"), (dict(T=0), "T=0"), (dict(Hdrop=Hd, ldhd=100), "ldhd"),
                    (dict(Hdrop=Hd, ldhd=200, p=0.5), "rng_state"), (dict(Hdrop=Hd, ldhd=200, p=1.0, rng=rng), "drop_p")):
        with pytest.raises(capi.ErcGraftError, match=msg):
            fwd(**kw)
    for kw, msg in ((dict(W=None), "null"), (dict(dGH=None), "null"), (dict(lddh=100), "lddh"), (dict(B=0), "B=0"),
                    (dict(p=0.5), "rng_state"), (dict(p=-0.1, rng=rng), "drop_p")):
        with pytest.raises(capi.ErcGraftError, match=msg):
            bwd(**kw)


@functools.lru_cache(maxsize=None)
def _padded_rows_run(lens):
    """forward (with the dropped copy) + backward on batch-major padded rows, B = 2, T = 9, with the given lengths: every output,
    saved buffer and gate gradient, on the CPU.  Everything is NaN beforehand."""
    B, T = 2, 9
    n = B * T
    g = torch.Generator().manual_seed(99)
    W = ((torch.rand(2, G3, H, generator=g) * 2 - 1) * 0.1).to(DEV)
    bh = ((torch.rand(2, G3, generator=g) * 2 - 1) * 0.1).to(DEV)
    GX, up = (torch.randn(n, 2 * G3, generator=g) * 0.5).to(DEV), torch.randn(n, 2 * H, generator=g).to(DEV)
    nan = lambda w: torch.full((n, w), float("nan"), device=DEV)
    o = dict(Hout=nan(2 * H), Hdrop=nan(2 * H), gates=nan(2 * G3), ghn=nan(2 * H), Hprev=nan(2 * H), dGX=nan(2 * G3), dGH=nan(2 * G3))
    rng = torch.tensor([3, 1234], dtype=torch.int64, device=DEV)
    lengths = torch.tensor(lens, dtype=torch.int64, device=DEV)
    capi.gru100_scan_fwd(GX, 2 * G3, W, bh, lengths, None, T, 1, B, T, o["Hout"], 2 * H, o["Hdrop"], 2 * H, 0.5, rng, 0x77,
                         o["gates"], o["ghn"], o["Hprev"])
    capi.gru100_scan_bwd(W, lengths, None, T, 1, B, T, o["gates"], o["ghn"], o["Hprev"], up, 2 * H, 0.5, rng, 0x77, o["dGX"],
                         o["dGH"])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@pytest.mark.parametrize("lens", [(12, 9), (0, 9)])
def test_padded_row_lengths_stay_inside_the_dialogues_rows(lens):
    """``lengths`` is a device input.  On padded rows a dialogue owns T rows: a longer length runs T steps and never reaches the
    next dialogue's rows, a zero length leaves zero outputs and zero gate gradients.  T = 9 crosses one chunk boundary of the
    scans (8 steps): chunk store, chunk request and tail meet.  Bit for bit against the run with lengths [9, 9]."""
    T = 9
    ref, got = _padded_rows_run((9, 9)), _padded_rows_run(lens)
    assert all(torch.isfinite(v).all() for v in ref.values())
    if lens[0] > T:
        for k in ref:
            assert torch.equal(got[k], ref[k]), k
    else:
        for k in ("Hout", "Hdrop", "dGX", "dGH"):
            assert bool((got[k][:T] == 0).all()), k
        for k in ref:
            assert torch.equal(got[k][T:], ref[k][T:]), k
