"""GPU: DialogueRNN (--module=dialogrnn) in capacity mode -- the index tables of a bucket / resident step
(erc_dialogrnn_meta_cap) against erc_dialogrnn_meta and numpy, the backward scan that owns the tails of its gradient buffers
(erc_dialogrnn_scan_bwd_cap) against erc_dialogrnn_scan_bwd at the same strides, the forward scan at capacity sizes against the
exact-size launch (bit for bit, with and without dropout: the masks are keyed by the compact row), the capacity step against
the exact-shape step after a larger batch has used the same bucket, dropout with the applied masks, bucket graph replay against
eager steps on the bucket's buffers, resident epochs against the bucketed loop, eval_scores, and the command line.

Kernel level: D_m = 8, GX given directly, every output buffer NaN (integer tables: a sentinel) beforehand, so that what a form
must not write is seen.  Every step-level test prints its measured figures.

Measured on one MI355X: the capacity step after a larger batch is bit-equal to
the exact-shape step -- loss, every gradient, the parameters after three Adam steps (the zero rows add +0 in the same order; the
asserted bounds are the sibling trainers'); with dropout the bucket step and the exact step from the same rng_state give bit-equal
E and Zc rows and the same loss (asserted); resident epochs end bit-equal to the bucketed loop (asserted); eval_scores'
log-probabilities are within 3.6e-7 of the exact-shape eval forward's."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests import dialogrnn_oracle as O
from tests.util_cases import fill_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W6 = torch.tensor([1 / 0.086747, 1 / 0.144406, 1 / 0.227883, 1 / 0.160585, 1 / 0.127711, 1 / 0.252668])
GXW, DREC_ROW, D_K, GUARD, SENT = 1050, 1500, 8, 3, -77
RNG_STREAM = 0x5d10
B_CAP, T_CAP = 32, 110

# name -> (lens, B, T, n_cap, n, S): (a) the LDS history limit, a length-1 dialogue and an empty slot; (b) no tail; (c) all tail;
# (d) the clipped capacity B * T; (e) sum 140 > 128: the second dialogue is clamped to 58 rows; (f) = (a) with speaker ids 0..8
CASES = {"a": ([110, 1, 0, 7], 4, 110, 128, 118, 2), "b": ([100, 28], 2, 110, 128, 128, 2), "c": ([0, 0, 0], 3, 5, 15, 0, 2),
         "d": ([5, 5], 2, 5, 10, 10, 2), "e": ([70, 70], 2, 110, 128, 128, 2), "f": ([110, 1, 0, 7], 4, 110, 128, 118, 9)}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _gpu(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def sent(n, dtype=torch.int32):
    return torch.full((n, ), SENT, dtype=dtype, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def plus_zero(t):
    """every element is +0.0, bit for bit (== 0 with a clear sign bit)"""
    return bool((bits(t) == 0).all())


def all_nan(t):
    return bool(torch.isnan(t).all())


def _clamped(lens, T, n_cap):
    """the lengths erc_dialogrnn_meta_cap counts: clamped to [0, T] and to the capacity that is left"""
    out, acc = [], 0
    for L in lens:
        L = min(min(max(L, 0), T), n_cap - acc)
        out.append(L)
        acc += L
    return out


def _node_tables(lens_c):
    """(node_off, dialogue of every node, position of every node) of compact rows"""
    off = np.concatenate([[0], np.cumsum(lens_c)]).astype(np.int64)
    b_of = np.repeat(np.arange(len(lens_c)), lens_c).astype(np.int64)
    t_of = np.concatenate([np.arange(L) for L in lens_c] + [np.zeros(0, np.int64)]).astype(np.int64)
    return off, b_of, t_of


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """the case's random inputs on the host, computed once and left unchanged"""
    lens, B, T, n_cap, n, S = CASES[case]
    r = np.random.RandomState(11 + ord(case))
    ids = r.randint(0, S, (T, B))
    if S == 9:
        ids = (np.arange(T)[:, None] * 4 + np.arange(B)[None, :] + r.randint(0, 2, (T, B))) % 9      # every id 0..8 occurs
    onehot = np.eye(S, dtype=np.float32)[ids]
    onehot[0, 0] = 0.0                                   # no maximum: index 0
    if T > 3:
        onehot[3, 0] = 0.5                               # all equal: the first index
        onehot[2, 0, :] = np.linspace(0.1, 0.2, S)       # a soft row: the last index
    lens_c = _clamped(lens, T, n_cap)
    assert sum(lens_c) == n
    off, b_of, t_of = _node_tables(lens_c)
    spk = onehot[t_of, b_of].argmax(-1).astype(np.int32) if n else np.zeros(0, np.int32)
    spk = np.concatenate([spk, r.randint(0, S, n_cap - n).astype(np.int32)])          # capacity rows: whatever, never read
    return dict(onehot=torch.from_numpy(onehot), lens_c=lens_c, off=off, b_of=b_of, t_of=t_of, spk=torch.from_numpy(spk),
                GX=torch.from_numpy((r.randn(n_cap, 2 * GXW) * 0.5).astype(np.float32)),
                dEmo=torch.from_numpy(r.randn(n_cap, 200).astype(np.float32)))


@pytest.fixture(scope="module")
def mod():
    """a DialogRNNModule at D_m = 8 with its recurrent blocks packed"""
    from erc_amd.dialogrnn import DialogRNNModule
    m = DialogRNNModule(D_K, 150, 150, 100, 100, n_classes=6, context_attention="general")
    fill_params(m, 31)
    m.finalize(DEV)
    capi.dialogrnn_pack(m.flat.data, m.offs, D_K, m.WT)
    torch.cuda.synchronize()
    return m


# ------------------------------------------------------------------------------------------------------------ meta_cap
@pytest.mark.parametrize("case", sorted(CASES))
def test_meta_cap_bucket_form_equals_meta_and_numpy(case):
    """node_off and rows < n of node_row / node_spk are bit-equal to erc_dialogrnn_meta's and to numpy's (t*B + b, first index
    of the one-hot maximum); capacity rows: row 0, speaker 0; counts = {n, longest dialogue}; nothing at or past n_cap"""
    lens, B, T, n_cap, n, S = CASES[case]
    inp = _inputs(case)
    onehot, lens_d = inp["onehot"].to(DEV), torch.tensor(lens, dtype=torch.int64, device=DEV)
    off_c, row_c, spk_c, counts = sent(B + 1 + GUARD), sent(n_cap + GUARD), sent(n_cap + GUARD), sent(2 + GUARD)
    capi.dialogrnn_meta_cap(onehot, S, lens_d, None, None, None, 0, B, T, n_cap, off_c, row_c, spk_c, None, counts)
    off_x, row_x, spk_x = sent(B + 1 + GUARD), sent(n_cap + GUARD), sent(n_cap + GUARD)
    capi.dialogrnn_meta(onehot, S, lens_d, B, T, n_cap, off_x, row_x, spk_x)
    torch.cuda.synchronize()
    assert torch.equal(off_c, off_x) and torch.equal(row_c[:n], row_x[:n]) and torch.equal(spk_c[:n], spk_x[:n])
    assert bool((row_x[n:] == SENT).all())                                  # the exact form has no capacity rows
    assert off_c[:B + 1].tolist() == inp["off"].tolist() and int(off_c[B]) == n
    assert row_c[:n].tolist() == (inp["t_of"] * B + inp["b_of"]).tolist()
    assert spk_c[:n].tolist() == inp["spk"][:n].tolist()
    assert bool((row_c[n:n_cap] == 0).all()) and bool((spk_c[n:n_cap] == 0).all())
    for t in (off_c[B + 1:], row_c[n_cap:], spk_c[n_cap:], counts[2:]):
        assert bool((t == SENT).all())
    assert counts[:2].tolist() == [n, max(inp["lens_c"])]
    assert torch.equal(onehot.cpu(), inp["onehot"])


@pytest.mark.parametrize("case", sorted(CASES))
def test_meta_cap_resident_form_equals_numpy(case):
    """desc = lengths | first store rows: node_row = the store row, node_spk = the store's id clamped to [0, S), labels gathered;
    capacity rows: the zero row behind the store, speaker 0, label 0"""
    lens, B, T, n_cap, n, S = CASES[case]
    inp = _inputs(case)
    r = np.random.RandomState(5 + ord(case))
    first, U = [0] * B, 4
    for b in reversed(range(B)):                       # the dialogues lie in the store in another order, with gaps
        first[b] = U
        U += lens[b] + 3
    store_spk = torch.from_numpy(r.randint(-2, S + 3, U).astype(np.int64))          # ids outside [0, S) are clamped
    store_lab = torch.from_numpy(r.randint(0, 6, U).astype(np.int64))
    desc = torch.tensor(lens + first, dtype=torch.int32, device=DEV)
    off_c, row_c, spk_c, counts = sent(B + 1 + GUARD), sent(n_cap + GUARD), sent(n_cap + GUARD), sent(2 + GUARD)
    lab_c = sent(n_cap + GUARD, torch.int64)
    capi.dialogrnn_meta_cap(None, S, None, desc, store_spk.to(DEV), store_lab.to(DEV), U, B, T, n_cap, off_c, row_c, spk_c, lab_c,
                            counts)
    torch.cuda.synchronize()
    rows = np.asarray(first, np.int64)[inp["b_of"]] + inp["t_of"]
    assert off_c[:B + 1].tolist() == inp["off"].tolist()
    assert row_c[:n].tolist() == rows.tolist()
    assert spk_c[:n].tolist() == store_spk.numpy()[rows].clip(0, S - 1).tolist()
    assert lab_c[:n].tolist() == store_lab.numpy()[rows].tolist()
    assert bool((row_c[n:n_cap] == U).all()) and bool((spk_c[n:n_cap] == 0).all()) and bool((lab_c[n:n_cap] == 0).all())
    for t in (off_c[B + 1:], row_c[n_cap:], spk_c[n_cap:], lab_c[n_cap:], counts[2:]):
        assert bool((t == SENT).all())
    assert counts[:2].tolist() == [n, max(inp["lens_c"])]


def test_meta_cap_refuses_mixed_forms_and_reads_the_zero_row_outside_the_store():
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=DEV)
    onehot = torch.zeros(4, 2, 2, device=DEV)
    with pytest.raises(capi.ErcGraftError, match="bucket form"):
        capi.dialogrnn_meta_cap(onehot, 2, i64(2), i32(4), i64(8), None, 8, 2, 4, 8, i32(3), i32(8), i32(8), None, i32(2))
    with pytest.raises(capi.ErcGraftError, match="bucket form"):
        capi.dialogrnn_meta_cap(None, 2, i64(2), None, None, None, 0, 2, 4, 8, i32(3), i32(8), i32(8), None, i32(2))
    with pytest.raises(capi.ErcGraftError, match="B="):
        capi.dialogrnn_meta_cap(onehot, 2, i64(2), None, None, None, 0, 1025, 4, 8, i32(3), i32(8), i32(8), None, i32(2))
    # a dialogue that runs over the end of a 6-row store: its last two nodes read the zero row, speaker 0, label 0
    desc = torch.tensor([4, 4], dtype=torch.int32, device=DEV)
    spk, lab = torch.ones(6, dtype=torch.int64, device=DEV), torch.full((6, ), 3, dtype=torch.int64, device=DEV)
    off, row, sp, lb, counts = i32(2), sent(8), sent(8), sent(8, torch.int64), i32(2)
    capi.dialogrnn_meta_cap(None, 2, None, desc, spk, lab, 6, 1, 4, 8, off, row, sp, lb, counts)
    torch.cuda.synchronize()
    assert row.tolist() == [4, 5, 6, 6, 6, 6, 6, 6] and sp.tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    assert lb.tolist() == [3, 3, 0, 0, 0, 0, 0, 0] and counts.tolist() == [4, 4]


# ----------------------------------------------------------------------------------------------------------- the scans
def _drop(drop):
    return (0.5, 0.35, torch.tensor([3, 1234], dtype=torch.int64, device=DEV)) if drop else (0.0, 0.0, None)


def _scan_fwd(m, GX, node_off, spk, B, T, S, N, drop):
    p_cell, p_emo, rng = _drop(drop)
    n_save = capi.dialogrnn_save_floats(N, B, T)
    E, save = nan(N + GUARD, 200), nan(n_save + GUARD)
    capi.dialogrnn_scan_fwd(GX, 2 * GXW, m.WT, m.flat.data, m.offs, D_K, node_off, spk, B, T, S, N, p_cell, p_emo, rng, RNG_STREAM, E,
                            200, save)
    torch.cuda.synchronize()
    return E, save


def _scan_bwd(m, GX, node_off, spk, B, T, S, N, drop, save, dEmo, n_dev=None, ld=2 * GXW):
    p_cell, p_emo, rng = _drop(drop)
    dGX, dREC = nan(N + GUARD, ld), nan(2 * N * DREC_ROW + GUARD)
    capi.dialogrnn_scan_bwd(GX, 2 * GXW, m.WT, m.flat.data, m.offs, D_K, node_off, spk, B, T, S, N, p_cell, p_emo, rng, RNG_STREAM, save,
                            dEmo, 200, dGX, ld, dREC, n_dev=n_dev)
    torch.cuda.synchronize()
    return dGX, dREC


def _check_bwd_cap(x, c, n, n_cap, ld=2 * GXW):
    """``x``: the exact launch, ``c``: the capacity launch, both (dGX, dREC) at the stride n_cap"""
    W = 2 * GXW
    assert same_bits(c[0][:n, :W], x[0][:n, :W]) and bool(torch.isfinite(c[0][:n, :W]).all())
    assert all_nan(x[0][n:]) and plus_zero(c[0][n:n_cap, :W])
    assert all_nan(c[0][n_cap:]) and all_nan(c[0][:, W:]) and all_nan(c[1][2 * n_cap * DREC_ROW:])          # guards
    px, pc = (capi.dialogrnn_planes(t[1], n_cap, capi.DIALOGRNN_DREC) for t in (x, c))
    for k in pc:
        assert same_bits(pc[k][:, :n], px[k][:, :n]) and bool(torch.isfinite(pc[k][:, :n]).all()), k
        assert all_nan(px[k][:, n:]) and plus_zero(pc[k][:, n:]), k
    if n:
        assert float(c[0][:n, :W].abs().max()) > 0 and all(float(v[:, :n].abs().max()) > 0 for v in pc.values())


@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_scan_bwd_cap_equals_scan_bwd_and_owns_the_tails(mod, case, drop):
    """rows < n of dGX and of the four dREC planes bit-identical to erc_dialogrnn_scan_bwd at the same strides (which leaves
    the rows past n alone); rows [n, n_cap): +0, both directions; guard rows behind n_cap still NaN; a second launch and a
    launch with *n_dev above n_cap (clamped) where n = n_cap give the same bits"""
    lens, B, T, n_cap, n, S = CASES[case]
    inp = _inputs(case)
    node_off = torch.tensor(inp["off"], dtype=torch.int32, device=DEV)
    GX, spk, dEmo = inp["GX"].to(DEV), inp["spk"].to(DEV), inp["dEmo"].to(DEV)
    E, save = _scan_fwd(mod, GX, node_off, spk, B, T, S, n_cap, drop)
    assert bool(torch.isfinite(E[:n]).all()) and all_nan(E[n:])
    n_dev = torch.tensor([n, max(inp["lens_c"])], dtype=torch.int32, device=DEV)
    args = (mod, GX, node_off, spk, B, T, S, n_cap, drop, save, dEmo)
    x, c, c2 = _scan_bwd(*args), _scan_bwd(*args, n_dev=n_dev), _scan_bwd(*args, n_dev=n_dev)
    _check_bwd_cap(x, c, n, n_cap)
    assert same_bits(c2[0], c[0]) and same_bits(c2[1], c[1]), "second launch"
    if n == n_cap:
        over = _scan_bwd(*args, n_dev=torch.tensor([n_cap + 1000], dtype=torch.int32, device=DEV))
        assert same_bits(over[0], c[0]) and same_bits(over[1], c[1]), "*n_dev above n_cap is clamped"
    assert n_dev.tolist() == [n, max(inp["lens_c"])] and same_bits(GX.cpu(), inp["GX"]) and same_bits(dEmo.cpu(), inp["dEmo"])


def test_scan_bwd_cap_with_a_wider_dgx_pitch_zeroes_rows_of_2100_columns(mod):
    """lddgx = 2104: the tail of dGX is one range per row; the four pad columns of every row stay NaN"""
    lens, B, T, n_cap, n, S = CASES["a"]
    inp = _inputs("a")
    node_off = torch.tensor(inp["off"], dtype=torch.int32, device=DEV)
    GX, spk, dEmo = inp["GX"].to(DEV), inp["spk"].to(DEV), inp["dEmo"].to(DEV)
    _, save = _scan_fwd(mod, GX, node_off, spk, B, T, S, n_cap, 0)
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV)
    args = (mod, GX, node_off, spk, B, T, S, n_cap, 0, save, dEmo)
    _check_bwd_cap(_scan_bwd(*args, ld=2104), _scan_bwd(*args, n_dev=n_dev, ld=2104), n, n_cap, ld=2104)
    with pytest.raises(capi.ErcGraftError, match="110"):
        _scan_bwd(mod, GX, node_off, spk, B, 111, S, n_cap, 0, save, dEmo, n_dev=n_dev)


@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_scan_fwd_at_capacity_sizes_equals_the_exact_size_launch(mod, case, drop):
    """erc_dialogrnn_scan_fwd with B + 2 slots (two more empty ones), T = T_cap and N = n_cap against the launch with the
    batch's own B, T = longest dialogue and N = n: emotions, every saved plane and the attention weights bit-equal on rows < n,
    with and without dropout from the same rng_state (the masks are keyed by the compact row); nothing written past n"""
    lens, B, T, n_cap, n, S = CASES[case]
    inp = _inputs(case)
    off = inp["off"].tolist()
    GX, spk = inp["GX"].to(DEV), inp["spk"].to(DEV)
    Bc = B + 2
    E_c, save_c = _scan_fwd(mod, GX, torch.tensor(off + [n, n], dtype=torch.int32, device=DEV), spk, Bc, T, S, n_cap, drop)
    assert all_nan(E_c[n:]) and all_nan(save_c[capi.dialogrnn_save_floats(n_cap, Bc, T):])
    pc = capi.dialogrnn_planes(save_c, n_cap, capi.DIALOGRNN_SAVE)
    for k in pc:
        assert all_nan(pc[k][:, n:]), k
    if n == 0:
        assert all_nan(save_c)                 # (c): no slot runs a step
        return
    Tx = max(inp["lens_c"])
    E_x, save_x = _scan_fwd(mod, GX[:n].contiguous(), torch.tensor(off, dtype=torch.int32, device=DEV), spk[:n].contiguous(), B, Tx,
                            S, n, drop)
    assert same_bits(E_c[:n], E_x[:n]) and bool(torch.isfinite(E_c[:n]).all())
    px = capi.dialogrnn_planes(save_x, n, capi.DIALOGRNN_SAVE)
    for k in pc:
        assert same_bits(pc[k][:, :n], px[k]), k
    if drop:
        for pre, post in (("g", "g_drop"), ("q", "q_drop"), ("e", "e_drop")):
            kept = pc[post][:, :n] != 0
            assert 0.4 < float(kept.float().mean()) < 0.6, post
    Ls = torch.tensor(inp["lens_c"], device=DEV)
    s, j = torch.arange(Tx, device=DEV)[None, :, None], torch.arange(Tx, device=DEV)[None, None, :]
    valid = ((s < Ls[:, None, None]) & (j < s))[None].expand(2, B, Tx, Tx)
    a_c = capi.dialogrnn_alpha(save_c, n_cap, Bc, T)[:, :B, :Tx, :Tx]
    a_x = capi.dialogrnn_alpha(save_x, n, B, Tx)
    assert torch.equal(bits(a_c)[valid], bits(a_x)[valid])
    assert all_nan(capi.dialogrnn_alpha(save_c, n_cap, Bc, T)[:, B:])          # the empty slots wrote nothing


# ------------------------------------------------------------------------------------------------------- step level
def _case(lens, D, S, C, seed):
    g = torch.Generator().manual_seed(seed)
    B, T = len(lens), max(lens)
    x = torch.randn(T, B, D, generator=g) * 0.5
    onehot = torch.nn.functional.one_hot(torch.randint(0, S, (T, B), generator=g), S).float()
    for b, L in enumerate(lens):
        x[L:, b] = 0.0
        onehot[L:, b] = 0.0
        onehot[L:, b, 0] = 1.0                 # the speaker-0 one-hot pad rows of the real collate
    return {"input_tensor": x, "speaker_tensor": onehot, "text_length": torch.tensor(lens, dtype=torch.int64),
            "attention_mask": (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float(),
            "label": torch.randint(0, C, (sum(lens),), generator=g)}


def _trainer(extra=("--capacity_buckets=True", ), t_cap=T_CAP, small=False):
    """``small``: features of width 24 (a 4 + t 12 + v 8) instead of the dataset's 712"""
    from track_mm.dialogrnn import DialogRNNParams
    from erc_amd.dialogrnn import DialogRNNTrainer
    params = DialogRNNParams().from_args(["--dataset=iemocap-cogmen-6"] + list(extra))
    if small:
        params.hidden_audio, params.hidden_text, params.hidden_visual, params.hidden_all = 4, 12, 8, 24
    tr = DialogRNNTrainer(params, DEV)
    tr.t_cap = t_cap
    return tr


def _state(tr):
    """everything a training step changes (what StepGraphs.precapture snapshots)"""
    flat, opt = tr.model.flat, tr.optim
    ts = [t for t in (getattr(flat, n, None) for n in ("data", "exp_avg", "exp_avg_sq", "grad_full")) if t is not None]
    if getattr(opt, "state", None) is not None:
        ts.append(opt.state)
    return ts


def _snapshot(tr):
    return [(t, t.clone()) for t in _state(tr)]


def _restore(snap):
    with torch.no_grad():
        for t, keep in snap:
            t.copy_(keep)
    torch.cuda.synchronize()


def _params(tr):
    return tr.model.flat.data.detach().clone()


def _grads(tr):
    return {k: tr.model.flat.g(k).detach().clone() for k in tr.model.flat.params}


SMALL, BIG = [12, 40, 3, 25], [110, 3, 3, 3, 3, 2, 2, 2]        # N = 80 and N = 128: both in the (32, 110, 128) bucket


def _capacity_step(tr, static, fill, batch, step=False):
    fill(static, batch)
    tr.model.dynamic_n = True
    try:
        stats = tr.train_step(static) if step else tr.model.loss_and_grads(static, tr.class_weight)
    finally:
        tr.model.dynamic_n = False
    torch.cuda.synchronize()
    return stats


def test_capacity_step_equals_the_exact_shape_step_after_a_larger_batch():
    """dropout 0: a ragged batch (lengths 12, 40, 3, 25; D = 712) in the (B_cap, T_cap, N_cap) = (32, 110, 128) bucket, run
    AFTER a larger batch (8 dialogues, T = 110, N = 128) has used the same bucket, against the exact-shape step from the same
    parameters: loss within 1e-4 (the forward GEMMs all take the unsplit kernel: zero is expected), every gradient within 1e-3
    of its largest entry; parameters after three Adam steps within the bounds of test_gpu_dialogrnn's Adam check.  The largest
    deviations are printed (the weight-gradient sums run over the capacity rows in another order)."""
    tr = _trainer(["--capacity_buckets=True", "--dropout=0", "--dropout_rec=0"])
    assert tr.model._drops(True) == pytest.approx((0.0, 0.15))          # dropout_rec' = dropout + 0.15 stays (dgcnv2_models.py:436-438) ...
    tr.model.drop_emo = 0.0                               # ... and is switched off here: this test compares two steps bit for bit
    tr.model.train()
    small, big = tr.prepare_batch(_case(SMALL, 712, 2, 6, 1)), tr.prepare_batch(_case(BIG, 712, 2, 6, 2))
    key, make, fill = tr.capacity_bucket(small)
    assert key == ("capacity", 32, 110, 128) and tr.capacity_bucket(big)[0] == key
    static = make()
    exact = tr.model.loss_and_grads(small, tr.class_weight)[:3].clone()          # loss, correct count, weight sum
    want_loss = float(exact[0])
    want = _grads(tr)
    _capacity_step(tr, static, fill, big)
    stats = _capacity_step(tr, static, fill, small)
    ws = tr.model._last_ws
    assert ws["counts"].tolist() == [80, 40]
    assert float(stats[1]) == float(exact[1]) and 0 <= float(stats[1]) <= 80
    assert float(stats[2]) == float(exact[2])
    assert abs(float(stats[2]) - float(tr.class_weight.cpu().double()[_case(SMALL, 712, 2, 6, 1)["label"]].sum())) < 1e-3
    d_loss = abs(float(stats[0]) - want_loss)
    worst = 0.0
    for k, g in want.items():
        got = tr.model.flat.g(k)
        scale = float(g.abs().max()) + 1e-6
        e = float((got - g).abs().max())
        worst = max(worst, e / scale)
        assert torch.isfinite(got).all() and e <= 1e-3 * scale, (k, e, scale)
    print("dialogrnn capacity vs exact: |loss diff| = %.3g, worst gradient deviation %.3g of the largest entry" % (d_loss, worst))
    assert np.isfinite(want_loss) and d_loss <= 1e-4
    # what the tails own is zero past the batch, whatever the larger batch left
    for k in ("dQ", "dE", "dA", "dZc", "dlogits", "dGX"):
        assert bool((ws[k][80:128] == 0).all()) and float(ws[k][:80].abs().max()) > 0, k
    assert bool((ws["dREC"].view(-1) != 0).any())
    for k, v in ws["dr"].items():
        assert bool((v[:, 80:128] == 0).all()) and float(v[:, :80].abs().max()) > 0, k
    assert float(ws["sv"]["g_prev"][:, 80:128].abs().max()) > 0          # ... and it did leave its saved states there
    # three Adam steps
    snap = _snapshot(tr)
    for _ in range(3):
        tr.train_step(small)
    torch.cuda.synchronize()
    exact = _params(tr)
    _restore(snap)
    _capacity_step(tr, static, fill, big, step=True)              # leaves its rows in the bucket's workspace ...
    _restore(snap)                                                # ... and nothing in the parameters
    for _ in range(3):
        _capacity_step(tr, static, fill, small, step=True)
    d = (_params(tr) - exact).abs()
    print("dialogrnn capacity vs exact after 3 Adam steps: max |dp| = %.3g, share above 1e-5 = %.3g"
          % (float(d.max()), float((d > 1e-5).float().mean())))
    assert float((d > 1e-5).float().mean()) < 0.01 and float(d.max()) < 7e-4


def test_capacity_dropout_step_matches_oracle_with_the_applied_masks():
    """training mode in the (32, 110, 128) bucket, D = 24: the masks of g, q[p], e, of the emotions and of the classifier are
    read back from the step's buffers (compact rows, as in the exact step); the CPU restatement given those masks reproduces
    loss and gradients within the bounds tests/test_gpu_dialogrnn.py holds the exact step to; keep rates near 0.5 / 0.5 / 0.5 /
    0.35 / 0.5.  The scans key their masks by (compact row, unit) and the classifier's GEMM epilogue by row * 100 + column of
    Zc (csrc/gemm.hip, csrc/gemm_stream.hip): neither the batch's nor the bucket's shape enters, so the exact-shape step from
    the same rng_state draws the same masks -- its E rows are bit-equal and its loss is equal."""
    from erc_amd.dialogrnn import DialogRNNModule
    lens, D = [14, 30, 1, 9], 24
    batch = _case(lens, D, 2, 6, 8)
    B, T, N = len(lens), max(lens), sum(lens)
    m = DialogRNNModule(D, 150, 150, 100, 100, n_classes=6, context_attention="general")
    fill_params(m, 4)
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.finalize(DEV)
    m.train()
    static = dict(input_tensor=torch.zeros(T_CAP, B_CAP, D, device=DEV), speaker_tensor=torch.zeros(T_CAP, B_CAP, 2, device=DEV),
                  text_length=torch.zeros(B_CAP, dtype=torch.int64, device=DEV), label=torch.zeros(128, dtype=torch.int64, device=DEV))
    static["input_tensor"][:T, :B] = batch["input_tensor"].to(DEV)
    static["speaker_tensor"][:T, :B] = batch["speaker_tensor"].to(DEV)
    static["text_length"][:B] = batch["text_length"].to(DEV)
    static["label"][:N] = batch["label"].to(DEV)
    m.dynamic_n = True
    stats = m.loss_and_grads(static, W6.to(DEV))
    m.dynamic_n = False
    torch.cuda.synchronize()
    ws = m._last_ws
    assert ws["counts"].tolist() == [N, T] and ws["E"].shape[0] == 128
    cap_loss, E_cap = float(stats[0]), ws["E"][:N].clone()
    sv = {k: v[:, :N].cpu() for k, v in ws["sv"].items()}
    masks, rates = {}, {}
    for key, pre, post in (("g", "g", "g_drop"), ("q", "q", "q_drop"), ("e", "e", "e_drop")):
        assert float((sv[pre] == 0).float().mean()) < 1e-3
        kept = sv[post] != 0
        masks[key] = kept.float() * 2.0
        rates[key] = float(kept.float().mean())
        on = kept & (sv[pre] != 0)
        assert torch.allclose(sv[post][on], sv[pre][on] * 2.0, rtol=1e-6, atol=0)
        assert not torch.equal(kept[0], kept[1])                      # the two directions differ
    e_post = torch.cat([sv["e_drop"][0], sv["e_drop"][1]], -1)        # [N, 200]
    E = E_cap.cpu()
    live = e_post != 0
    keep_emo = 1.0 / 0.35
    masks["emo"] = torch.where(E != 0, torch.full_like(E, keep_emo), torch.zeros_like(E))
    rates["emo"] = float(((E != 0) & live).float().sum() / live.float().sum())
    assert torch.allclose(E[E != 0], (e_post * keep_emo)[E != 0], rtol=1e-5, atol=0)
    pre = ws["A"][:N].cpu() @ P["linear.weight"].t() + P["linear.bias"]
    z = ws["Zc"][:N].cpu()
    masks["clf"] = torch.where((z != 0) | (pre <= 0), torch.full_like(pre, 2.0), torch.zeros_like(pre))
    rates["clf"] = float((z != 0).float().sum() / (pre > 0).float().sum())
    print("dialogrnn capacity dropout: keep rates %s" % {k: round(v, 3) for k, v in rates.items()})
    for key, want in (("g", 0.5), ("q", 0.5), ("e", 0.5), ("emo", 0.35), ("clf", 0.5)):
        assert abs(rates[key] - want) < 0.05, (key, rates)
    loss, _, _, grads = O.loss_and_grads(P, batch, W6, masks=masks)
    assert abs(cap_loss - float(loss)) < 1e-4
    assert sorted(grads) == sorted(m.flat.params)
    for name, g in grads.items():
        got = m.flat.g(name).detach().cpu()
        g = g.float()
        scale = float(g.abs().max()) + 1e-6
        assert float((got - g).abs().max()) <= 1e-3 * scale, (name, float((got - g).abs().max()), scale)
    # the exact-shape step from the same rng_state (no optimizer here: the counter has not moved)
    x_stats = m.loss_and_grads(_gpu(batch), W6.to(DEV))
    torch.cuda.synchronize()
    xs = m._last_ws
    assert xs is not ws and xs["E"].shape[0] == N
    print("dialogrnn dropout, bucket vs exact from the same rng_state: |loss diff| = %.3g, E bit-equal: %s"
          % (abs(float(x_stats[0]) - cap_loss), same_bits(xs["E"], E_cap)))
    assert same_bits(xs["E"], E_cap)
    assert same_bits(xs["Zc"], ws["Zc"][:N]), "the classifier's mask is keyed by row and column"
    assert float(x_stats[0]) == cap_loss


FOUR = ([12, 40, 3, 25], [110, 3, 3, 3, 3, 2, 2, 2], [7] * 9, [1, 2, 60, 30, 11])          # all in the (32, 110, 128) bucket


def test_bucket_graph_over_four_batches_equals_eager_steps_on_the_buckets_buffers():
    """StepGraphs with the buckets on (dropout 0.5): first batch eager + capture, three replays -- bit-identical to the same
    four steps run eagerly on the bucket's static buffers (capture=False); replaying one batch twice from a restored state is
    bit-identical"""
    from erc_amd.trainer import StepGraphs
    batches = [_case(l, 712, 2, 6, 20 + i) for i, l in enumerate(FOUR)]
    ends = []
    for capture in (False, True):
        tr = _trainer()
        assert tr.model._drops(True) == pytest.approx((0.5, 0.65))
        g = StepGraphs(tr, capture=capture)
        losses = []
        for b in batches:
            losses.append(g.step(tr.prepare_batch(b))[0].clone())
        torch.cuda.synchronize()
        assert list(g.cache) == [("capacity", 32, 110, 128)]
        assert (g.captures, g.replays, g.eager) == ((1, 3, 1) if capture else (0, 0, 4))
        assert not tr.model.dynamic_n
        ends.append((_params(tr), [float(v) for v in losses]))
    assert all(np.isfinite(ends[0][1]))
    assert torch.equal(ends[0][0], ends[1][0]) and ends[0][1] == ends[1][1]
    snap = _snapshot(tr)
    b = tr.prepare_batch(batches[3])
    outs = []
    for _ in range(2):
        _restore(snap)
        g.step(b)
        torch.cuda.synchronize()
        outs.append(_params(tr))
    assert g.replays == 5 and torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], ends[1][0])


def _dialogues(p, n, seed, max_len=45):
    from erc_amd.synthetic import make_dialogues
    return make_dialogues(n, p.dims(), n_speakers=p.n_speakers, n_classes=p.n_classes, min_len=1, max_len=max_len, seed=seed)


def test_resident_epochs_equal_the_bucketed_loop():
    """two epochs from a DeviceDialogueStore (28 dialogues, B = 8: one 2 B int32 copy + one replay per step) against StepGraphs
    fed the batches of the same permutations: per-epoch loss sums within 1e-4 per step, final parameters within the Adam check's
    bounds -- and, as measured, bit-equal"""
    from erc_amd.datasets import DeviceDialogueStore
    from erc_amd.trainer import ResidentEpochs, StepGraphs
    Bsz, seed = 8, 3
    ends = []
    for mode in ("resident", "bucketed"):
        tr = _trainer(["--capacity_buckets=True", "--train.batch_size=%d" % Bsz], t_cap=0, small=True)
        p = tr.params
        store = DeviceDialogueStore(_dialogues(p, 28, 9), p, torch.device(DEV))
        tr.t_cap = int(store.lengths.max())
        tr.model.train()
        sums = []
        if mode == "resident":
            res = ResidentEpochs(tr, store, Bsz, seed)
            assert res.supported()
            prev = 0.0
            for _ in range(2):
                n_utt, n_steps = res.epoch()
                torch.cuda.synchronize()
                tot = float(res.acc[0])
                sums.append(tot - prev)
                prev = tot
            assert n_steps == 4 and res.replays > 0 and res.eager == res.captures <= 3
        else:
            g, gen = StepGraphs(tr), torch.Generator().manual_seed(seed)
            for _ in range(2):
                order = torch.randperm(len(store), generator=gen)
                acc = torch.zeros((), dtype=torch.float64, device=DEV)
                for i in range(0, len(store), Bsz):
                    acc += g.step(tr.prepare_batch(store.batch(order[i:i + Bsz])))[0].double()
                torch.cuda.synchronize()
                sums.append(float(acc))
            assert g.replays > 0 and g.eager == g.captures <= 3
        assert not tr.model.dynamic_n
        ends.append((_params(tr), sums))
    (p_res, s_res), (p_buc, s_buc) = ends
    d = (p_res - p_buc).abs()
    print("dialogrnn resident vs bucketed: epoch loss sums %s vs %s, max |dp| = %.3g, bit-equal parameters: %s"
          % (s_res, s_buc, float(d.max()), torch.equal(p_res, p_buc)))
    assert all(np.isfinite(s_res)) and all(abs(a - b) <= 4 * 1e-4 for a, b in zip(s_res, s_buc))
    assert float((d > 1e-5).float().mean()) < 0.01 and float(d.max()) < 7e-4
    assert s_res == s_buc and torch.equal(p_res, p_buc)      # the same launches on the same rows: measured bit-equal


def test_eval_scores_adds_up_to_the_confusion_matrix_of_the_exact_path():
    """a resident test epoch over a 6-dialogue store (B = 4: two steps, every step eager): cm equals numpy's confusion matrix of
    the argmax of ``to_logits`` on the exact path (eval mode) over the same dialogues; cm is added to; the parameters, the
    optimizer state, the dropout counter, the training flag and the training step's workspace stay bit for bit as they were"""
    from erc_amd.datasets import DeviceDialogueStore
    from erc_amd.trainer import ResidentEval
    tr = _trainer(["--device_collate", "--resident", "--resident_eval", "--train.batch_size=4"], t_cap=0, small=True)
    p = tr.params
    store = DeviceDialogueStore(_dialogues(p, 6, 4), p, torch.device(DEV))
    tr.model.train()
    tr.train_step(tr.prepare_batch(store.batch([0, 1])))          # a non-zero dropout counter and optimizer state
    torch.cuda.synchronize()
    before = [t.clone() for t in _state(tr)]
    rng0, last0 = tr.model.rng_state.clone(), tr.model._last_ws
    ev = ResidentEval(tr, store, 4, capture=False)
    assert ev.supported() and ev.steps == 2
    cm = ev.epoch().numpy()
    torch.cuda.synchronize()
    assert tr.model.training and not tr.model.dynamic_n and torch.equal(tr.model.rng_state, rng0) and tr.model._last_ws is last0
    assert all(torch.equal(a, b) for a, b in zip(_state(tr), before))
    want = np.zeros((6, 6), np.int64)
    lens = store.lengths.tolist()
    tr.model.eval()
    worst = 0.0
    for s in range(2):
        idx = list(range(4 * s, min(4 * s + 4, 6)))
        batch = store.batch(idx)
        logp = tr.to_logits(tr.prepare_batch(batch))
        np.add.at(want, (batch["label"].cpu().numpy(), logp.argmax(-1).cpu().numpy()), 1)
        ws = ev.graphs[ev.caps[s]][2]
        if s == 1 or ev.caps[0] != ev.caps[1]:          # (a workspace shared by both steps holds the last one's logits)
            n = sum(lens[i] for i in idx)
            assert ws["counts"].tolist() == [n, max(lens[i] for i in idx)]
            worst = max(worst, float((torch.log_softmax(ws["logits"][:n], -1) - logp).abs().max()))
    tr.model.train()
    print("dialogrnn eval_scores: max |log-prob - exact-shape log-prob| = %.3g" % worst)
    assert worst < 1e-4 and int(want.sum()) == sum(lens)
    np.testing.assert_array_equal(cm, want)
    # added to, not overwritten: the last step once more on the cm the epoch left
    last = np.zeros((6, 6), np.int64)
    batch = store.batch([4, 5])
    tr.model.eval()
    np.add.at(last, (batch["label"].cpu().numpy(), tr.to_logits(tr.prepare_batch(batch)).argmax(-1).cpu().numpy()), 1)
    tr.model.train()
    ev.cur_desc.copy_(ev.table_dev[1])
    ev._step(ev._batch(ev.caps[-1]))
    np.testing.assert_array_equal(ev.cm.cpu().numpy(), want + last)
    assert tr.model.training and torch.equal(tr.model.rng_state, rng0)
    # erc_rows_score holds a fixed number of classes: more are refused before any launch
    tr.model.n_classes = capi.rows_score_max_classes() + 1
    with pytest.raises(capi.ErcGraftError, match="at most %d classes" % capi.rows_score_max_classes()):
        tr.model.eval_scores(ev._batch(ev.caps[-1]), ev.cm)
    tr.model.n_classes = 6


# -------------------------------------------------------------------------------------------------------------- CLI
def _cli(args):
    res = subprocess.run([sys.executable, "train_mm.py"] + args, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]


DATA = ["--dataset=iemocap-cogmen-6", "--modality=atv", "--epoch=2", "--n_train=24", "--n_test=6", "--train.batch_size=8"]
CLI = ["--module=dialogrnn"] + DATA
FLAGS = ["--device_collate", "--resident", "--resident_eval"]


def _cli_params(extra):
    from track_mm.dialogrnn import DialogRNNParams
    return DialogRNNParams().from_args(DATA + list(extra))


def _cli_node_capacities():
    """the node capacity of every training step of the command line below, from the run's own dialogues and the permutations
    ResidentEpochs draws (generator seeded with --seed, one randperm per epoch; T = the store's longest dialogue)"""
    from erc_amd import trainer as T
    from erc_amd.capacity import node_capacity
    p = _cli_params(FLAGS)
    lens = [len(d["label"]) for d in T.load_dialogues(p)[0]]
    B, t_cap, gen, caps = int(p.train.batch_size), max(lens), torch.Generator().manual_seed(p.seed), []
    for _ in range(p.epoch):
        order = torch.randperm(len(lens), generator=gen).tolist()
        caps += [node_capacity(sum(lens[j] for j in order[i:i + B]), 128, B * t_cap) for i in range(0, len(order), B)]
    return caps


def test_train_mm_cli_resident_and_resident_eval():
    """``train_mm.py --module=dialogrnn ... --device_collate --resident --resident_eval``: exit 0, finite losses; ONE captured
    training graph per node capacity the run's six batches fall into -- fewer than its steps -- and every other step a replay;
    the test metrics, scored on the device, equal those of the host test loop of the same run without ``--resident_eval`` (the
    same training, so the same state).

    "One training graph" holds per node capacity, not per run: with N_BUCKET = 128 a batch of 8 dialogues of 20..110 utterances
    has some 400 .. 700 nodes, and the six batches of this run fall into more than one multiple of 128 (the expected set is
    computed here from the run's own dialogues and permutations).  One graph per run would need one node capacity B_cap * T_cap,
    whose step carries all 880 rows through every node launch; DAG-ERC, where no launch scales with N, does that.  The epoch
    line does not carry the evaluation loop's counters: the test below holds the evaluation graph of this configuration."""
    caps = _cli_node_capacities()
    assert len(caps) == 2 * 3 and 1 <= len(set(caps)) < len(caps), caps          # (else this run could show no replay)
    lines = _cli(CLI + FLAGS)
    epochs = [l for l in lines if "test" in l]
    losses = [l["Lall"] for l in lines if "Lall" in l]
    assert len(epochs) == 2 and len(losses) == 2 and all(np.isfinite(losses))
    last = epochs[-1]
    print("dialogrnn CLI resident: node capacities %s; %d graphs captured, %d replays, %d eager steps" %
          (caps, last["graphs_captured"], last["graph_replays"], last["eager_steps"]))
    assert last["graphs_captured"] == len(set(caps)) and last["eager_steps"] == last["graphs_captured"]
    assert last["graph_replays"] == len(caps) - len(set(caps)) > 0
    first = epochs[0]
    assert first["graphs_captured"] == len(set(caps[:3])) and first["graph_replays"] == 3 - len(set(caps[:3]))
    host = [l for l in _cli(CLI + FLAGS[:2]) if "test" in l]
    assert len(host) == 2
    for e, h in zip(epochs, host):
        assert "test_s" in e and "test_s" not in h
        assert set(e["test"]) == set(h["test"])
        for k, v in h["test"].items():
            assert abs(e["test"][k] - v) < 1e-9, (k, e["test"][k], v)


def test_the_cli_configurations_test_epochs_replay_one_evaluation_graph():
    """the evaluation side of the command line above, in this process (trainer.run prints the training loop's counters only):
    the 6-dialogue test store at --test.batch_size 32 is one step of one node capacity -- the first epoch runs it eagerly and
    captures ONE graph, every later epoch is one replay -- and every epoch returns the same confusion matrix over all the
    store's utterances"""
    from erc_amd import trainer as T
    from erc_amd.dialogrnn import DialogRNNTrainer
    p = _cli_params(FLAGS)
    T.fix_seed(p.seed)
    tr = DialogRNNTrainer(p, torch.device(DEV))
    loop = T.EpochLoop(p, tr, torch.device(DEV))
    resident, ev, test_loader = loop.resident, loop.res_eval, loop.test_loader
    assert type(ev) is T.ResidentEval and ev.steps == 1 and len(set(ev.caps)) == 1
    tr.model.eval()
    cms = []
    for _ in range(3):
        cms.append(ev.epoch().numpy())
        torch.cuda.synchronize()
    assert (ev.captures, ev.eager, ev.replays) == (1, 1, 2)
    assert int(cms[0].sum()) == int(test_loader.store.lengths.sum())
    assert all(np.array_equal(cms[0], c) for c in cms[1:])
    assert (resident.captures, resident.eager, resident.replays) == (0, 0, 0)


def test_train_mm_cli_without_the_flags_runs_the_exact_shape_loop():
    """the same command without the three flags (host collate, no resident store): exact shapes, of which none repeats in two
    reshuffled epochs, so every step is eager and nothing is captured"""
    lines = _cli(CLI)
    steps = [l["Lall"] for l in lines if "Lall" in l]
    epochs = [l for l in lines if "test" in l]
    assert len(epochs) == 2 and steps and all(np.isfinite(steps))
    last = epochs[-1]
    assert "test_s" not in last
    assert last["graphs_captured"] == 0 and last["graph_replays"] == 0 and last["eager_steps"] == 2 * 3
