"""CPU: the float64 references of tests/rnn_scan_ref.py and the bounds of tests/test_gpu_lstm_scan.py / test_gpu_gru_scan.py,
checkable without a GPU: the chains against torch.nn.LSTM / torch.nn.GRU on a packed ragged batch, the contract's
weight-gradient products against autograd, the committed TOL tables against the float32 yardstick recomputed here, and the
sensitivity of every tensor class to four plausible kernel defects."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from tests import rnn_scan_ref as R
from tests.test_gpu_gru_scan import TOL as TOL_GRU
from tests.test_gpu_lstm_scan import TOL as TOL_LSTM

TOL = dict(TOL_LSTM, **TOL_GRU)
ROUND_OFF = 1e-12
LENS = [1, 9, 17]


def _torch_case(cell, seed, leaves=False):
    """a case whose GX = X W_ih^T + b_ih comes from torch modules (.double()), lengths 1, 9, 17; the GRU: three modules"""
    torch.manual_seed(seed)
    Hh, G = (100, 400) if cell == "lstm" else (200, 600)
    B, T = len(LENS), max(LENS)
    n_mod = 1 if cell == "lstm" else 3
    mods = [(torch.nn.LSTM if cell == "lstm" else torch.nn.GRU)(R.DX, Hh, bidirectional=True, batch_first=True).double()
            for _ in range(n_mod)]
    cat = lambda k: torch.stack([torch.stack([getattr(m, k + "_l0"), getattr(m, k + "_l0_reverse")]) for m in mods]).detach().clone()
    W_ih, b_ih, W_hh, b_hh = cat("weight_ih"), cat("bias_ih"), cat("weight_hh"), cat("bias_hh")
    if leaves:
        for t in (W_ih, b_ih, W_hh, b_hh):
            t.requires_grad_()
    X = torch.randn(n_mod, B, T, R.DX, dtype=torch.float64)
    up = torch.randn(n_mod, B, T, 2 * Hh, dtype=torch.float64)
    GX = X @ W_ih.reshape(n_mod, 2 * G, R.DX).transpose(1, 2)[:, None] + b_ih.reshape(n_mod, 1, 1, 2 * G)
    sq = (lambda t: t[0]) if cell == "lstm" else (lambda t: t)
    c = dict(name="torch", cell=cell, lens=LENS, run=LENS, B=B, T=T, Tc=T, H=Hh, G=G, W_hh=sq(W_hh), b_hh=sq(b_hh), GX=sq(GX),
             up=sq(up), X=sq(X))
    return c, mods, (W_ih, b_ih, W_hh, b_hh), X, up


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_chains_match_torch_on_a_packed_ragged_batch(cell):
    """float64, bidirectional, pack_padded_sequence with lengths 1, 9, 17: outputs and every parameter gradient (the latter
    through the contract's products) within float64 round-off of torch's"""
    c, mods, _, X, up = _torch_case(cell, 3)
    G = c["G"]
    out = R.reference(c)
    out = [out] if cell == "lstm" else out
    for m, (mod, o) in enumerate(zip(mods, out)):
        y, _ = mod(pack_padded_sequence(X[m], torch.tensor(LENS), batch_first=True, enforce_sorted=False))
        y, _ = pad_packed_sequence(y, batch_first=True, total_length=c["T"])
        (y * up[m]).sum().backward()
        assert R.rel(o["Hout"], y.detach()) < ROUND_OFF
        for d, sfx in enumerate(("", "_reverse")):
            want = {k: getattr(mod, k + "_l0" + sfx).grad for k in ("weight_ih", "bias_ih", "weight_hh", "bias_hh")}
            assert R.rel(o["dW_ih"][d * G:(d + 1) * G], want["weight_ih"]) < ROUND_OFF, (m, d)
            assert R.rel(o["db_ih"][d * G:(d + 1) * G], want["bias_ih"]) < ROUND_OFF, (m, d)
            assert R.rel(o["dW_hh%d" % d], want["weight_hh"]) < ROUND_OFF, (m, d)
            assert R.rel(o["db_hh%d" % d], want["bias_hh"]) < ROUND_OFF, (m, d)


@pytest.mark.parametrize("masked", [0, 1])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_contract_products_match_autograd(cell, masked):
    """dW_ih = dGX^T X, db_ih, dW_hh[d] = dG^T Hprev[d], db_hh[d] of reference() equal the autograd gradients of the loss it
    returns wrt W_ih, b_ih (GX = X W_ih^T + b_ih), W_hh, b_hh -- also under an inverted-dropout mask"""
    c, _, prm, _, _ = _torch_case(cell, 4 + masked, leaves=True)
    G, lead = c["G"], (() if cell == "lstm" else (3, ))
    mask = None
    if masked:
        mask = (torch.rand(*lead, c["B"], c["T"], 2 * c["H"]) >= 0.3).double() / 0.7
    out = R.reference(c, mask=mask)
    out = [out] if cell == "lstm" else out
    gW_ih, gb_ih, gW_hh, gb_hh = torch.autograd.grad(sum(o["loss"] for o in out), prm)
    for m, o in enumerate(out):
        assert R.rel(o["dW_ih"], gW_ih[m].reshape(2 * G, -1)) < ROUND_OFF and R.rel(o["db_ih"], gb_ih[m].reshape(-1)) < ROUND_OFF
        for d in (0, 1):
            assert R.rel(o["dW_hh%d" % d], gW_hh[m, d]) < ROUND_OFF and R.rel(o["db_hh%d" % d], gb_hh[m, d]) < ROUND_OFF
        if masked:
            assert torch.equal(o["Hdrop"], o["Hout"] * mask[m] if lead else o["Hout"] * mask)


def test_the_tolerance_tables_cover_the_cases():
    assert sorted(TOL) == sorted(R.CASES) and sorted(TOL_LSTM) == sorted(R.LSTM_CASES)


@pytest.mark.parametrize("name", R.CASES)
def test_committed_bounds_are_four_times_the_float32_yardstick(name):
    """TOL of the GPU files is exactly 4 x the yardstick (reference in float32 against float64, one torch thread), rounded up
    to one significant digit, per case and class"""
    y = R.yardstick(R.make_case(name))
    print("%s yardstick: %s" % (name, "  ".join("%s=%.3g" % (k, y[k]) for k in R.CLASSES)))
    assert tuple(R.bound(y[k]) for k in R.CLASSES) == tuple(TOL[name])


SENSITIVITY = {"a": ("edges", "c0_at_8"), "b": ("edges", "rev_from_T"), "c": ("edges", "swap_fo"), "d": ("gru_b33", "bhn_outside")}


@pytest.mark.parametrize("which", sorted(SENSITIVITY))
def test_plausible_defects_move_every_class_far_beyond_its_bound(which):
    """the reference alone, float64: (a) c_{t-1} taken as 0 at steps s % 8 == 0, s > 0 (a lost carry at a chunk boundary;
    the backward chain of that forward run inherits it), (b) the reverse direction of a packed dialogue starting at T - 1
    instead of L - 1, (c) gates f and o exchanged, (d) GRU: b_hn outside r * (.) -- each moves every class by more than
    1000 x its bound"""
    name, mutate = SENSITIVITY[which]
    c = R.make_case(name)
    moved = R.class_errors(R.reference(c, mutate=mutate), R.reference(c))
    ratios = {k: moved[k] / TOL[name][i] for i, k in enumerate(R.CLASSES)}
    print("(%s) %s %s: %s" % (which, name, mutate, "  ".join("%s=%.3g (%.3g x bound)" % (k, moved[k], ratios[k]) for k in R.CLASSES)))
    assert all(r > 1000 for r in ratios.values()), ratios
