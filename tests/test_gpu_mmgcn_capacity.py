"""MMGCN in capacity mode on the GPU (MMGCNModule.dynamic_n): the node tables of erc_mm_meta_cap in both input forms
(integer-exact against a numpy table), every tail-safe row operator on its own against float64, and the capacity-sized step
-- static buffers, StepGraphs, graph replay, the resident step, resident_eval_step and a resident test epoch -- always
against ``oracle.mmgcn`` in float64 on the batch's own exact shape, with the bounds of tests/test_gpu_mmgcn.py: logits 1e-4,
loss 1e-5, every gradient within 5e-3 of its tensor's scale.

Shapes: B_cap = 4 dialogue slots with lengths (17, 0, 1, 33) -- one slot empty, 17 and 33 cross a 16-row part boundary of the
chain, length 1 is a pure-diagonal adjacency block -- T_cap = 40 above the batch's 33, N = 51 nodes in N_cap = 128; modalities
atv with two speakers and six classes, av with nine speakers and seven classes."""
import copy
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from tests.util_cases import _collate, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = dict(a=12, t=20, v=16)
KEYS = dict(a="audio_feature", t="text_feature", v="visual_feature")
B_CAP, T_CAP, N_CAP, FD = 4, 40, 128, 200
SLOTS = (17, 0, 1, 33)                      # lengths of the dialogue slots; N = 51
N = sum(SLOTS)
CASES = [("atv", 2, 6), ("av", 9, 7)]
# (parameter seed, dialogue seed) of the confusion-matrix tests: every row's top-two gap in the float64 oracle logits is above
# 1e-3, ten times the logit bound (found on the CPU; asserted again where it is used)
CM_SEEDS = {"atv": (4, 51), "av": (5, 53)}
TEST_LENGTHS = (9, 33, 1, 17, 5, 12)
U32 = 2.0 ** -24                            # unit roundoff of fp32


# ------------------------------------------------------------------------------------------------ shared, computed once
def _dialogues(lengths, S, C, seed):
    from erc_amd.synthetic import make_dialogues
    return [make_dialogues(1, DIMS, n_speakers=S, n_classes=C, min_len=n, max_len=n, seed=seed * 7919 + i)[0]
            for i, n in enumerate(lengths)]


def _exact_batch(dialogues, S, C, mods):
    return _collate(dialogues, S, C, mods, False, True)


def _new_oracle(mods, S, C, seed=4):
    from oracle.mmgcn import MMGCNOracle
    torch.manual_seed(seed)
    return MMGCNOracle(hidden_text=DIMS["t"], hidden_visual=DIMS["v"], hidden_audio=DIMS["a"], n_speakers=S, n_classes=C, modals=mods)


@functools.lru_cache(maxsize=None)
def _oracle(mods, S, C, seed=4):
    return _new_oracle(mods, S, C, seed)


def _dbl(batch):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}


def _oracle_step(ref, batch):
    """(loss, logits [N, C], {name: gradient}) of a float64 copy of the oracle ``ref`` in eval mode (every dropout off)"""
    torch.set_num_threads(8)
    r64 = copy.deepcopy(ref).double().eval()
    logits, _ = r64(**_dbl(batch))
    loss = F.cross_entropy(logits, batch["label"])
    loss.backward()
    return float(loss.detach()), logits.detach(), {n: p.grad.clone() for n, p in r64.named_parameters() if p.grad is not None}


@functools.lru_cache(maxsize=None)
def _reference(mods, S, C, lengths=SLOTS, seed=3):
    """the exact-shape batch of the non-empty slots of ``lengths`` and the float64 oracle's step on it (never modified)"""
    batch = _exact_batch(_dialogues([n for n in lengths if n > 0], S, C, seed), S, C, mods)
    return batch, _oracle_step(_oracle(mods, S, C), batch)


def _module(mods, S, C, ref=None):
    from erc_amd.mmgcn import MMGCNModule
    mine = MMGCNModule(hidden_text=DIMS["t"], hidden_visual=DIMS["v"], hidden_audio=DIMS["a"], n_speakers=S, n_classes=C, modals=mods)
    mine.load_state_dict((ref or _oracle(mods, S, C)).state_dict())
    return mine.finalize(DEV)


def _static(mods, S, junk=3.0):
    """capacity-sized static buffers holding what a step must not depend on: features of ``junk`` and speaker 1 in the empty
    slot and at t >= the batch's longest dialogue"""
    spk = torch.zeros(T_CAP, B_CAP, S, device=DEV)
    spk[:, :, 1] = 1.0
    st = {k: None for k in KEYS.values()}
    st.update({KEYS[m]: torch.full((T_CAP, B_CAP, DIMS[m]), junk, device=DEV) for m in mods})
    st.update(speaker_tensor=spk, text_length=torch.zeros(B_CAP, dtype=torch.int64, device=DEV),
              label=torch.zeros(N_CAP, dtype=torch.int64, device=DEV))
    return st


def _place(static, lengths, batch, mods):
    """the dialogues of the exact-shape ``batch`` into the non-empty slots of ``lengths``, zero padded up to the batch's T
    (what the collate gives); everything else stays"""
    slots = [b for b, n in enumerate(lengths) if n > 0]
    T = batch["speaker_tensor"].shape[0]
    for k in [KEYS[m] for m in mods] + ["speaker_tensor"]:
        for i, b in enumerate(slots):
            static[k][:T, b] = batch[k][:, i].to(DEV)
    static["text_length"].copy_(torch.tensor(lengths))
    n = int(batch["label"].shape[0])
    static["label"][:n] = batch["label"].to(DEV)
    static["label"][n:] = 0
    return static


def _valid_rows(Mo, n=N, n_cap=N_CAP):
    return torch.cat([m * n_cap + torch.arange(n) for m in range(Mo)])


def _tail_rows(Mo, n=N, n_cap=N_CAP):
    return torch.cat([m * n_cap + torch.arange(n, n_cap) for m in range(Mo)])


GRAD_SIDE = ("dlogits", "dFE", "DH", "DGl", "DZl", "dH0", "dX", "dXD", "dXH")


def _check_step(mine, stats, want, n=N, t_max=max(SLOTS), what=""):
    """loss, valid logits and every live gradient of the module's last capacity step against the oracle's; the tail invariant"""
    loss, logits, grads = want
    ws, Mo = mine._last_ws, len(mine.order)
    assert ws["counts"].tolist() == [n, t_max], what
    assert ws["cap"][:3] == (B_CAP, T_CAP, N_CAP) and ws["logits"].shape == (N_CAP, mine.n_classes)
    e_logits = float((ws["logits"][:n].cpu().double() - logits).abs().max())
    e_loss = abs(float(stats[0]) - loss)
    assert sorted(mine.flat.params) == sorted(grads), what
    errs = {name: rel_err(mine.flat.g(name).cpu(), grads[name]) for name in mine.flat.params}
    worst = max(errs, key=errs.get)
    print("mmgcn-cap %s logits=%.2e loss=%.2e grad=%.2e (%s)" % (what, e_logits, e_loss, errs[worst], worst))
    assert e_logits < 1e-4, what
    assert e_loss < 1e-5, what
    assert errs[worst] < 5e-3, (what, sorted(errs.items(), key=lambda kv: -kv[1])[:6])
    assert int(mine.flat.health[0]) == 0
    # a tail row's content is finite; the gradient-side tail rows are exactly zero
    tail = _tail_rows(Mo, n).to(DEV)
    for k in ("X", "XH", "H0", "FE", "logits", "Call", "HD"):
        assert bool(torch.isfinite(ws[k]).all()), (what, k)
    for k in GRAD_SIDE:
        rows = ws[k][n:N_CAP] if k in ("dlogits", "dFE") else ws[k][tail]
        assert int((rows != 0).sum()) == 0, (what, k)
    assert int((ws["dG"][0][tail] != 0).sum()) == 0, what


# ------------------------------------------------------------------------------------------------------------- meta
def _meta_out():
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)
    return dict(node_off=i32(B_CAP + 1), node_row=i32(N_CAP), node_pad=i32(N_CAP), node_dlg=i32(N_CAP), node_spk=i32(N_CAP),
                pad_node=i32(B_CAP * T_CAP), x_row=i32(B_CAP * T_CAP), label=torch.full((N_CAP, ), -7, dtype=torch.int64, device=DEV),
                counts=i32(2))


def _meta_numpy(lengths, spk_valid, first=None, zero_row=0, labels=None):
    """the table, slot by slot: spk_valid[b] = the speaker ids of slot b's utterances; first[b] = its first store row"""
    n = sum(lengths)
    t = dict(node_off=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), counts=np.array([n, max(lengths)], dtype=np.int32),
             node_row=np.full(N_CAP, zero_row if first is not None else 0, dtype=np.int32), node_pad=np.zeros(N_CAP, dtype=np.int32),
             node_dlg=np.zeros(N_CAP, dtype=np.int32), node_spk=np.zeros(N_CAP, dtype=np.int32),
             pad_node=np.full(B_CAP * T_CAP, N_CAP, dtype=np.int32), x_row=np.full(B_CAP * T_CAP, zero_row, dtype=np.int32),
             label=np.zeros(N_CAP, dtype=np.int64))
    i = 0
    for b, L in enumerate(lengths):
        for s in range(L):
            row = s * B_CAP + b
            t["node_pad"][i], t["node_dlg"][i], t["node_spk"][i], t["pad_node"][row] = row, b, spk_valid[b][s], i
            t["node_row"][i] = row if first is None else first[b] + s
            if first is not None:
                t["x_row"][row] = first[b] + s
                t["label"][i] = labels[first[b] + s]
            i += 1
    return t


LENGTH_SETS = (SLOTS, (0, 0, 0, 5), (40, 40, 40, 8), (32, 32, 32, 32))


@pytest.mark.parametrize("S", [2, 9])
@pytest.mark.parametrize("lengths", LENGTH_SETS, ids=str)
def test_meta_cap_bucket_form_against_a_numpy_table(lengths, S):
    """padded positions and empty slots hold speaker 1 in the qmask and must not show; tail entries are the fixed sentinel"""
    from erc_amd import capi
    g = torch.Generator().manual_seed(7)
    valid = [torch.randint(0, S, (n, ), generator=g).tolist() for n in lengths]
    ids = torch.ones(T_CAP, B_CAP, dtype=torch.int64)
    for b, v in enumerate(valid):
        ids[:len(v), b] = torch.tensor(v, dtype=torch.int64)
    qmask = torch.nn.functional.one_hot(ids, S).float().to(DEV)
    want = _meta_numpy(lengths, valid)
    o = _meta_out()
    capi.mm_meta_cap(torch.tensor(lengths, dtype=torch.int64, device=DEV), qmask, qmask.stride(0), qmask.stride(1), S, None, None,
                     None, 0, B_CAP, T_CAP, N_CAP, o["node_off"], o["node_row"], o["node_pad"], o["node_dlg"], o["node_spk"],
                     o["pad_node"], None, None, o["counts"])
    for name in ("node_off", "node_row", "node_pad", "node_dlg", "node_spk", "pad_node", "counts"):
        np.testing.assert_array_equal(o[name].cpu().numpy(), want[name], err_msg=name)
    assert int((o["x_row"] != -7).sum()) == 0 and int((o["label"] != -7).sum()) == 0      # not the bucket form's to write
    if sum(lengths) == N_CAP and min(lengths) > 0:       # the valid rows are erc_mm_meta's own
        e = _meta_out()
        capi.mm_meta(torch.tensor(lengths, dtype=torch.int64, device=DEV), qmask, qmask.stride(0), qmask.stride(1), S, B_CAP,
                     e["node_off"], e["node_row"], e["node_dlg"], e["node_spk"])
        for name in ("node_off", "node_row", "node_dlg", "node_spk"):
            assert torch.equal(e[name], o[name]), name


@pytest.mark.parametrize("lengths", LENGTH_SETS, ids=str)
def test_meta_cap_resident_form_against_a_numpy_table(lengths):
    """desc = lengths | first store rows over a store of 12 dialogues visited out of order; an empty slot names row 17"""
    from erc_amd import capi
    S = 9
    store_lens = [33, 5, 40, 1, 17, 40, 32, 8, 32, 40, 32, 32]
    offs = np.concatenate([[0], np.cumsum(store_lens)])
    U = int(offs[-1])
    g = torch.Generator().manual_seed(9)
    store_spk = torch.randint(0, S, (U, ), generator=g)
    store_lab = torch.randint(0, 7, (U, ), generator=g)
    pick = []
    for n in lengths:
        pick.append(next(i for i in reversed(range(len(store_lens))) if store_lens[i] == n and i not in pick) if n else None)
    first = [int(offs[d]) if d is not None else 17 for d in pick]
    desc = torch.tensor(list(lengths) + first, dtype=torch.int32, device=DEV)
    want = _meta_numpy(lengths, [store_spk[f:f + n].tolist() for f, n in zip(first, lengths)], first, U, store_lab.numpy())
    o = _meta_out()
    capi.mm_meta_cap(None, None, 0, 0, S, desc, store_spk.to(DEV), store_lab.to(DEV), U, B_CAP, T_CAP, N_CAP, o["node_off"],
                     o["node_row"], o["node_pad"], o["node_dlg"], o["node_spk"], o["pad_node"], o["x_row"], o["label"], o["counts"])
    for name in want:
        np.testing.assert_array_equal(o[name].cpu().numpy(), want[name], err_msg=name)


def test_meta_cap_refuses_mixed_forms():
    from erc_amd import capi
    o = _meta_out()
    out = (o["node_off"], o["node_row"], o["node_pad"], o["node_dlg"], o["node_spk"], o["pad_node"])
    lens = torch.zeros(B_CAP, dtype=torch.int64, device=DEV)
    qmask = torch.zeros(T_CAP, B_CAP, 2, device=DEV)
    desc = torch.zeros(2 * B_CAP, dtype=torch.int32, device=DEV)
    with pytest.raises(capi.ErcGraftError, match="resident form"):
        capi.mm_meta_cap(lens, qmask, 8, 2, 2, desc, lens, None, 5, B_CAP, T_CAP, N_CAP, *out, o["x_row"], None, o["counts"])
    with pytest.raises(capi.ErcGraftError, match="bucket form"):
        capi.mm_meta_cap(lens, None, 8, 2, 2, None, None, None, 0, B_CAP, T_CAP, N_CAP, *out, None, None, o["counts"])
    with pytest.raises(capi.ErcGraftError, match="bad sizes"):
        capi.mm_meta_cap(lens, qmask, 8, 2, 2, None, None, None, 0, 1025, T_CAP, N_CAP, *out, None, None, o["counts"])


# ---------------------------------------------------------------------------------------- the row operators, one by one
BIG = 1e30          # what the tail rows of every input hold: squared it overflows, summed it swamps any valid row


def _n_dev(n=N):
    return torch.tensor([n, 0], dtype=torch.int32, device=DEV)


def _rows_input(Mo, width, seed, n=N):
    """[Mo * N_CAP, width] standard normal on the valid rows, BIG on the tail rows (cpu float32)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Mo * N_CAP, width, generator=g)
    x[_tail_rows(Mo, n)] = BIG
    return x


def _assert_tail_zero_rest_finite(y, Mo, n=N):
    y = y.cpu()
    assert bool(torch.isfinite(y).all()) and int((y[_tail_rows(Mo, n)] != 0).sum()) == 0


@pytest.mark.parametrize("n", [N, 0, N_CAP])
def test_flatten_cap(n):
    """rows < n: src[row_map] + emb[spk], one fp32 addition (half an ulp of the sum); tail rows: 0 whatever the sentinel reads"""
    from erc_amd import capi
    g = torch.Generator().manual_seed(1)
    src, emb = torch.randn(B_CAP * T_CAP, FD, generator=g), torch.randn(9, FD, generator=g)
    row_map = torch.randint(0, B_CAP * T_CAP, (N_CAP, ), generator=g).to(torch.int32)
    spk = torch.randint(0, 9, (N_CAP, ), generator=g).to(torch.int32)
    src[0] = BIG
    row_map[:n].clamp_(min=1)
    row_map[n:], spk[n:] = 0, 0
    dst = torch.full((N_CAP, FD), BIG, device=DEV)
    capi.mm_flatten_cap(src.to(DEV), FD, row_map.to(DEV), emb.to(DEV), spk.to(DEV), N_CAP, _n_dev(n), dst, FD)
    want = src[row_map[:n].long()].double() + emb[spk[:n].long()].double()
    got = dst.cpu()
    assert bool(((got[:n].double() - want).abs() <= U32 * want.abs()).all())
    _assert_tail_zero_rest_finite(dst, 1, n)


def test_emb_grad_cap():
    """demb[s] = the sum of the rows < n of speaker s.  Bound: fp32 summation of k terms, (k - 1) u sum|x| per column"""
    from erc_amd import capi
    S = 9
    dl = _rows_input(1, FD, 2)
    g = torch.Generator().manual_seed(3)
    spk = torch.randint(0, S, (N_CAP, ), generator=g).to(torch.int32)
    spk[N:] = 0                                    # the sentinel speaker of the tail: BIG rows that must not reach speaker 0
    ws = torch.zeros(capi.mm_emb_grad_ws_floats(S), device=DEV)
    for n in (N, 0):
        demb = torch.full((S, FD), BIG, device=DEV)
        capi.mm_emb_grad_cap(dl.to(DEV), FD, spk.to(DEV), N_CAP, _n_dev(n), S, demb, ws)
        got = demb.cpu().double()
        for s in range(S):
            rows = dl[:n][spk[:n] == s].double()
            bound = max(len(rows) - 1, 0) * U32 * rows.abs().sum(0) + 1e-30
            assert bool(((got[s] - rows.sum(0)).abs() <= bound).all()), (n, s)


@pytest.mark.parametrize("Mo", [3, 2])
def test_row_normalize_cap_and_its_backward(Mo):
    """xhat = x / |x|, inv = 1 / |x| on the rows < n: |x|^2 is a 200-term fp32 sum of positive terms (relative error 200 u), square
    root, reciprocal and product one rounding each -> 104 u relative; tail rows: xhat = inv = 0 although x is BIG there.
    Backward dx += inv (d - xhat (xhat . d)): the 200-term dot product carries 200 u sum|xhat d|, the rest a few roundings of the
    terms' sizes; tail rows of dx are written 0 although dx, xhat, inv and d hold BIG there."""
    from erc_amd import capi
    x = _rows_input(Mo, FD, 4)
    xhat, inv = torch.full((Mo * N_CAP, FD), BIG, device=DEV), torch.full((Mo * N_CAP, ), BIG, device=DEV)
    capi.mm_row_normalize_cap(x.to(DEV), Mo, N_CAP, _n_dev(), xhat, inv)
    v = _valid_rows(Mo)
    nrm = x[v].double().norm(dim=1)
    assert bool(((inv.cpu()[v].double() - 1 / nrm).abs() <= 104 * U32 / nrm).all())
    assert bool(((xhat.cpu()[v].double() - x[v].double() / nrm[:, None]).abs() <= 104 * U32 * (x[v].double().abs() / nrm[:, None]) + 1e-30).all())
    _assert_tail_zero_rest_finite(xhat, Mo)
    assert int((inv.cpu()[_tail_rows(Mo)] != 0).sum()) == 0
    # backward, on operands of its own (BIG in every tail row)
    h = (x[v].double() / nrm[:, None]).float()
    hh, rn, d, base = (torch.full((Mo * N_CAP, w), BIG).squeeze(-1) for w in (FD, 1, FD, FD))
    g = torch.Generator().manual_seed(5)
    hh[v], rn[v], d[v], base[v] = h, 0.5 + torch.rand(len(v), generator=g), torch.randn(len(v), FD, generator=g), torch.randn(len(v), FD, generator=g)
    dx = base.clone().to(DEV)
    capi.mm_row_normalize_bwd_cap(hh.to(DEV), rn.to(DEV), d.to(DEV), Mo, N_CAP, _n_dev(), dx)
    h64, d64, r64 = h.double(), d[v].double(), rn[v].double()[:, None]
    dot = (h64 * d64).sum(1, keepdim=True)
    want = base[v].double() + r64 * (d64 - h64 * dot)
    bound = U32 * (r64 * (200 * (h64 * d64).abs().sum(1, keepdim=True) * h64.abs() + 4 * (d64.abs() + (h64 * dot).abs())) + 2 * want.abs() +
                   base[v].double().abs())
    assert bool(((dx.cpu()[v].double() - want).abs() <= bound).all())
    _assert_tail_zero_rest_finite(dx, Mo)


@pytest.mark.parametrize("plain", [1, 0])
def test_gcnii_combine_bwd_cap(plain):
    """dout = d_hd [hd > 0] ks; dG = theta dout, dhi = (1 - theta)(1 - alpha) dout, dh0 += (1 - theta) alpha dout (plain: dG = dout): at
    most three fp32 roundings per value.  Tail rows: dG (and dhi) 0, dh0 as it was."""
    from erc_amd import capi
    Mo, theta, alpha, ks = 3, 0.3, 0.1, 1.0 / 0.6
    d_hd, hd = _rows_input(Mo, FD, 6), _rows_input(Mo, FD, 7)
    dh0_0 = torch.randn(Mo * N_CAP, FD, generator=torch.Generator().manual_seed(8))
    dG, dhi, dh0 = torch.full((Mo * N_CAP, FD), BIG, device=DEV), torch.full((Mo * N_CAP, FD), BIG, device=DEV), dh0_0.clone().to(DEV)
    capi.gcnii_combine_bwd_cap(d_hd.to(DEV), hd.to(DEV), Mo, N_CAP, _n_dev(), theta, alpha, ks, plain, dG, None if plain else dhi,
                               None if plain else dh0, FD, FD)
    v, t = _valid_rows(Mo), _tail_rows(Mo)
    dout = torch.where(hd[v] > 0, d_hd[v].double() * ks, torch.zeros((), dtype=torch.float64))
    close = lambda got, want: bool(((got.cpu()[v].double() - want).abs() <= 4 * U32 * (want.abs() + dh0_0[v].double().abs())).all())
    assert close(dG, dout if plain else theta * dout)
    _assert_tail_zero_rest_finite(dG, Mo)
    if not plain:
        assert close(dhi, (1 - theta) * (1 - alpha) * dout) and close(dh0, dh0_0[v].double() + (1 - theta) * alpha * dout)
        _assert_tail_zero_rest_finite(dhi, Mo)
        assert torch.equal(dh0.cpu()[t], dh0_0[t])


def test_dropout_fwd_cap():
    """kept entries are x ks (two roundings), the dropped share of the 30 600 valid entries is p within 0.02 (sigma 0.003), the
    tail rows are 0; with the device count at the capacity the launch IS erc_dropout_fwd's (same counter per element)"""
    from erc_amd import capi
    Mo, p = 3, 0.4
    x = _rows_input(Mo, FD, 9)
    rng = torch.tensor([11, 5], dtype=torch.int64, device=DEV)
    y = torch.full((Mo * N_CAP, FD), BIG, device=DEV)
    capi.dropout_fwd_cap(x.to(DEV), Mo, N_CAP, _n_dev(), FD, p, rng, 1000, y)
    v = _valid_rows(Mo)
    got, keep = y.cpu()[v].double(), y.cpu()[v] != 0
    want = x[v].double() / (1 - p)
    assert bool(((got - want)[keep].abs() <= 4 * U32 * want[keep].abs()).all())
    assert abs(1.0 - float(keep.double().mean()) - p) < 0.02
    _assert_tail_zero_rest_finite(y, Mo)
    full, plain_y = torch.empty(Mo * N_CAP, FD, device=DEV), torch.empty(Mo * N_CAP, FD, device=DEV)
    xs = torch.randn(Mo * N_CAP, FD, device=DEV)
    capi.dropout_fwd_cap(xs, Mo, N_CAP, _n_dev(N_CAP), FD, p, rng, 1000, full)
    capi.dropout_fwd(xs, Mo * N_CAP * FD, p, rng, 1000, plain_y)
    assert torch.equal(full, plain_y)
    assert torch.equal(full.cpu()[v] != 0, keep)          # the mask of an element does not depend on the batch's count


@pytest.mark.parametrize("Mo", [3, 2])
def test_regroup_cap_forward_and_backward(Mo):
    """FE[i, m 400 + c] = relu(cat[xd, h][(m, i), c]) exactly (p = 0: no arithmetic), 0 on the tail rows; backward: d_xd / d_h =
    dFE [FE > 0] ks (one rounding), tail rows 0 although dFE and FE hold BIG there"""
    from erc_amd import capi
    xd, hl = _rows_input(Mo, FD, 10), _rows_input(Mo, FD, 11)
    FE = torch.full((N_CAP, Mo * 2 * FD), BIG, device=DEV)
    capi.mm_regroup_fwd_cap(xd.to(DEV), hl.to(DEV), Mo, N_CAP, _n_dev(), 0.0, None, 3000, FE)
    cat = torch.cat([xd, hl], 1)
    want = torch.relu(torch.cat([cat[m * N_CAP:m * N_CAP + N] for m in range(Mo)], 1))
    assert torch.equal(FE.cpu()[:N], want)
    _assert_tail_zero_rest_finite(FE, 1)
    ks = 1.0 / 0.6
    g = torch.Generator().manual_seed(12)
    dFE, FEin = torch.full((N_CAP, Mo * 2 * FD), BIG), torch.full((N_CAP, Mo * 2 * FD), BIG)
    dFE[:N], FEin[:N] = torch.randn(N, Mo * 2 * FD, generator=g), want
    d_xd, d_h = torch.full((Mo * N_CAP, FD), BIG, device=DEV), torch.full((Mo * N_CAP, FD), BIG, device=DEV)
    capi.mm_regroup_bwd_cap(dFE.to(DEV), FEin.to(DEV), Mo, N_CAP, _n_dev(), ks, d_xd, d_h)
    gr = torch.where(want > 0, dFE[:N].double() * ks, torch.zeros((), dtype=torch.float64)).view(N, Mo, 2, FD)
    for m in range(Mo):
        for half, out in enumerate((d_xd, d_h)):
            w = gr[:, m, half]
            assert bool(((out.cpu()[m * N_CAP:m * N_CAP + N].double() - w).abs() <= 2 * U32 * w.abs()).all())
    _assert_tail_zero_rest_finite(d_xd, Mo)
    _assert_tail_zero_rest_finite(d_h, Mo)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("masked", [False, True])
def test_axpy_mask_cap(masked, accumulate):
    """y (+)= scale x [mask != 0]: two roundings; the tail rows of y are written 0 whether it accumulates or not"""
    from erc_amd import capi
    Mo, scale = 3, 1.0 / 0.6
    x, mask, y0 = _rows_input(Mo, FD, 13), _rows_input(Mo, FD, 14), _rows_input(Mo, FD, 15)
    mask[mask.abs() < 0.5] = 0.0
    y = y0.clone().to(DEV)
    capi.axpy_mask_cap(x.to(DEV), mask.to(DEV) if masked else None, Mo, N_CAP, _n_dev(), FD, scale, accumulate, y)
    v = _valid_rows(Mo)
    add = x[v].double() * scale
    if masked:
        add = torch.where(mask[v] != 0, add, torch.zeros((), dtype=torch.float64))
    want = add + (y0[v].double() if accumulate else 0.0)
    assert bool(((y.cpu()[v].double() - want).abs() <= 2 * U32 * (want.abs() + add.abs())).all())
    _assert_tail_zero_rest_finite(y, Mo)


def test_zero_tail_and_the_cross_operators_leave_the_tail_alone():
    """erc_mm_zero_tail clears the tail rows of a pitched buffer and nothing else.  erc_mm_cross_apply_cap / erc_mm_cross_grad_cap
    on the rows < n are the plain operators on the compact layout, bit for bit, and touch neither a tail row of ``out`` nor --
    with the tail's sentinel dialogue 0 and BIG operands there -- any entry of dCR."""
    from erc_amd import capi
    Mo, P, ld = 3, T_CAP, 264
    buf0 = torch.randn(Mo * N_CAP, ld, generator=torch.Generator().manual_seed(16))
    buf = buf0.clone().to(DEV)
    capi.mm_zero_tail(buf, ld, FD, Mo, N_CAP, _n_dev())
    want = buf0.clone()
    want[_tail_rows(Mo), :FD] = 0
    assert torch.equal(buf.cpu(), want)
    capi.mm_zero_tail(buf, ld, FD, Mo, N_CAP, _n_dev(N_CAP))          # a full batch: nothing to write
    assert torch.equal(buf.cpu(), want)
    # node tables of the slots (17, 0, 1, 33), compact and capacity-sized
    off = torch.tensor(np.concatenate([[0], np.cumsum(SLOTS)]), dtype=torch.int32, device=DEV)
    dlg = torch.cat([torch.full((L, ), b, dtype=torch.int32) for b, L in enumerate(SLOTS)])
    dlg_cap = torch.zeros(N_CAP, dtype=torch.int32)
    dlg_cap[:N] = dlg
    g = torch.Generator().manual_seed(17)
    CR = torch.randn(B_CAP, Mo * Mo, P, generator=g).to(DEV)
    h, d = _rows_input(Mo, FD, 18), _rows_input(Mo, FD, 19)
    v = _valid_rows(Mo)
    out_c, out_cap = torch.zeros(Mo * N, FD, device=DEV), torch.full((Mo * N_CAP, FD), 0.25, device=DEV)
    capi.mm_cross_apply(CR, h[v].contiguous().to(DEV), FD, dlg.to(DEV), off, Mo, N, P, out_c, FD)
    capi.mm_cross_apply_cap(CR, h.to(DEV), FD, dlg_cap.to(DEV), off, Mo, N_CAP, _n_dev(), P, out_cap, FD)
    assert torch.equal(out_cap.cpu()[v], out_c.cpu() + 0.25) and bool((out_cap.cpu()[_tail_rows(Mo)] == 0.25).all())
    dCR_c, dCR_cap = torch.zeros(B_CAP, Mo * Mo, P, device=DEV), torch.zeros(B_CAP, Mo * Mo, P, device=DEV)
    capi.mm_cross_grad(d[v].contiguous().to(DEV), FD, h[v].contiguous().to(DEV), FD, dlg.to(DEV), off, Mo, N, P, dCR_c)
    capi.mm_cross_grad_cap(d.to(DEV), FD, h.to(DEV), FD, dlg_cap.to(DEV), off, Mo, N_CAP, _n_dev(), P, dCR_cap)
    assert torch.equal(dCR_cap, dCR_c) and bool(torch.isfinite(dCR_cap).all())


# ------------------------------------------------------------------------------------------------------- the step
@pytest.mark.parametrize("mods,S,C", CASES)
def test_capacity_step_against_the_oracle(mods, S, C):
    """eager, dropout off (eval mode), junk in the empty slot and above the batch's T"""
    batch, want = _reference(mods, S, C)
    mine = _module(mods, S, C).eval()
    static = _place(_static(mods, S), SLOTS, batch, mods)
    mine.dynamic_n = True
    stats = mine.loss_and_grads(static).cpu()
    mine.dynamic_n = False
    _check_step(mine, stats, want, what="eager %s" % mods)
    assert len(mine._ws._d) == 1 and mine._last_ws["HI"].shape[0] == 1        # no per-layer planes in a capacity workspace


def _trainer(mods, S, C, extra=(), ref=None, drop=0.0, lr=None):
    from erc_amd.mmgcn import MMGCNTrainer
    from track_mm.mmgcn import MMGCNParams
    ds = "iemocap-cogmen-6" if C == 6 else "meld-mmgcn-7"
    p = MMGCNParams().from_args(["--dataset=" + ds, "--modality=" + mods, "--train.batch_size=4", "--test.batch_size=4",
                                 "--capacity_buckets=True"] + list(extra))
    p.hidden_audio, p.hidden_text, p.hidden_visual, p.n_speakers = DIMS["a"], DIMS["t"], DIMS["v"], S      # (the features of this file)
    assert p.n_classes == C
    tr = MMGCNTrainer(p, DEV)
    tr.model.load_state_dict((ref or _oracle(mods, S, C)).state_dict())
    tr.model.drop_p = drop
    if tr.model.lstm is not None:
        tr.model.lstm.drop_p = drop
    if lr is not None:
        tr.optim.lr = lr
    return tr, p


@pytest.mark.parametrize("mods,S,C", CASES)
def test_three_optimizer_steps_through_stepgraphs(mods, S, C):
    """StepGraphs on the trainer: one eager step on the bucket's static buffers, its capture, two replays -- batches of other
    lengths, fewer dialogues than slots, a longer one than before.  Before each step the module's parameters go into the
    oracle, so every step is compared on its own."""
    from erc_amd.trainer import StepGraphs
    tr, p = _trainer(mods, S, C)
    tr.t_cap = T_CAP
    ref = _new_oracle(mods, S, C)
    graphs = StepGraphs(tr)
    for step, lengths in enumerate(((17, 1, 33), (5, ), (40, 16, 31, 2))):
        batch = _exact_batch(_dialogues(lengths, S, C, seed=20 + step), S, C, mods)
        ref.load_state_dict({k: v.cpu() for k, v in tr.model.state_dict().items()})
        want = _oracle_step(ref, batch)
        before = tr.model.flat.data.clone()
        stats = graphs.step(tr.prepare_batch(batch)).cpu()
        _check_step(tr.model, stats, want, n=sum(lengths), t_max=max(lengths), what="stepgraphs %s step %d" % (mods, step))
        assert not torch.equal(tr.model.flat.data, before) and int(tr.optim.state[0]) == step + 1
    assert (graphs.captures, graphs.eager, graphs.replays) == (1, 1, 2)
    assert list(graphs.cache) == [("capacity", B_CAP, T_CAP, N_CAP)] and tr.model.dynamic_n is False
    tr.model.check_cluster()


def _sliced(ws, mine, slots, T):
    """the buffers tests/test_gpu_mmgcn._applied_masks reads, cut down to the batch's own rows"""
    Mo = len(mine.order)
    v = _valid_rows(Mo).to(DEV)
    out = dict(X=ws["X"][v], XD=ws["XD"][v], HD=ws["HD"][:, v], H0=ws["H0"][v], FE=ws["FE"][:N])
    out["_XD"], out["_H0"] = out["XD"], out["H0"]
    assert ws["_XD"] is ws["XD"] and ws["_H0"] is ws["H0"], "dropout on: the separate XD / H0 buffers"
    if "t" in mine.order:
        lw = ws["lstm:lstm_l."]
        cut = lambda t: t.view(T_CAP, B_CAP, 200)[:T, slots].contiguous()
        out["lstm:lstm_l."] = dict(H0=cut(lw["H0"]), H0d=cut(lw["H0d"]))
    return out


@pytest.mark.parametrize("mods,S,C", CASES)
def test_dropout_capacity_step_matches_oracle_with_the_applied_masks(mods, S, C):
    """One training-mode capacity step (p = 0.4 at every site) against tests/mmgcn_step_ref.py in float64, which is given the
    keep masks the step applied -- read back from the workspace's valid rows -- checked the way
    test_gpu_mmgcn.test_dropout_step_matches_oracle_with_the_applied_masks does: kept entries are the input times 1 / (1 - p),
    the dropped share per site is p within 0.04 (each layer within 0.06), and the bounds are the eval-mode ones."""
    from tests.mmgcn_step_ref import mmgcn_step_ref
    from tests.test_gpu_mmgcn import _applied_masks, _dropped_shares
    batch, _ = _reference(mods, S, C)
    for k in KEYS.values():
        batch.setdefault(k, None)
    ref = _oracle(mods, S, C)
    mine = _module(mods, S, C).train()
    p, ks = mine.drop_p, 1.0 / (1.0 - mine.drop_p)
    assert p == 0.4
    static = _place(_static(mods, S), SLOTS, batch, mods)
    mine.dynamic_n = True
    stats = mine.loss_and_grads(static).cpu()
    mine.dynamic_n = False
    ws = mine._last_ws
    assert ws["_p"] == p and int(mine.flat.health[0]) == 0 and ws["counts"].tolist() == [N, 33]
    slots = [b for b, n in enumerate(SLOTS) if n > 0]
    T = batch["speaker_tensor"].shape[0]
    masks = _applied_masks(mine, _sliced(ws, mine, slots, T), len(slots), T, N)
    torch.set_num_threads(8)
    want = mmgcn_step_ref(ref, batch, masks=masks, ks=ks)
    shares = _dropped_shares(masks, want["pre"], p)
    e_logits = float((ws["logits"][:N].cpu().double() - want["logits"]).abs().max())
    e_loss = abs(float(stats[0]) - float(want["loss"]))
    assert sorted(mine.flat.params) == sorted(want["grads"])
    errs = {n: rel_err(mine.flat.g(n).cpu(), want["grads"][n]) for n in mine.flat.params}
    worst = max(errs, key=errs.get)
    print("mmgcn-cap dropout %s logits=%.2e loss=%.2e grad=%.2e (%s) dropped %s"
          % (mods, e_logits, e_loss, errs[worst], worst, " ".join("%s=%.3f" % kv for kv in sorted(shares.items()))))
    assert e_logits < 1e-4
    assert e_loss < 1e-5
    assert errs[worst] < 5e-3, sorted(errs.items(), key=lambda kv: -kv[1])[:6]
    Mo = len(mine.order)
    tail = _tail_rows(Mo).to(DEV)
    for k in GRAD_SIDE:
        rows = ws[k][N:N_CAP] if k in ("dlogits", "dFE") else ws[k][tail]
        assert int((rows != 0).sum()) == 0, k
    assert int((ws["XD"][tail] != 0).sum()) == 0 and int((ws["FE"][N:] != 0).sum()) == 0


def test_nothing_of_a_full_batch_is_carried_over_in_the_tail():
    """Staleness: a full batch (N = 128 = N_cap: the chain and the grouped products write every row) and then the 51-node batch
    through the SAME bucket, in training mode with dropout on; the 51-node batch alone in a fresh trainer given the first one's
    parameters, Adam moments, step count and dropout counter.  Same launches, same shapes: loss, gradients and updated
    parameters must be equal bit for bit."""
    mods, S, C = "atv", 2, 6
    full = _exact_batch(_dialogues((40, 40, 40, 8), S, C, seed=61), S, C, mods)
    small = _exact_batch(_dialogues((17, 1, 33), S, C, seed=62), S, C, mods)
    a, _ = _trainer(mods, S, C, drop=0.4)
    b, _ = _trainer(mods, S, C, drop=0.4)
    results = []
    for tr, batches in ((a, (full, small)), (b, (small, ))):
        key, make, fill = tr._bucket(tr.prepare_batch(small), B_CAP, T_CAP, N_CAP)
        static = make()
        tr.model.dynamic_n = True
        for i, batch in enumerate(batches):
            fill(static, tr.prepare_batch(batch))
            if tr is a and i == 1:          # the fresh trainer starts where this one stands now
                for name in ("data", "exp_avg", "exp_avg_sq"):
                    getattr(b.model.flat, name).copy_(getattr(a.model.flat, name))
                b.optim.state.copy_(a.optim.state)
            stats = tr.train_step(static).clone()
        tr.model.dynamic_n = False
        assert tr.model._last_ws["counts"].tolist() == [N, 33]
        results.append((stats, tr.model.flat.grad.clone(), tr.model.flat.data.clone(), tr.model._last_ws["logits"][:N].clone()))
    assert int(a.optim.state[0]) == 2 and int(b.optim.state[0]) == 2
    for got, want, what in zip(results[0], results[1], ("stats", "gradients", "parameters", "logits")):
        assert torch.equal(got, want), what
    assert bool(torch.isfinite(results[0][0][:3]).all()) and float(results[0][0][0]) > 0
    a.model.check_cluster(), b.model.check_cluster()


# ------------------------------------------------------------------------------------------------------- resident
def _store(p, dialogues):
    from erc_amd.datasets import DeviceDialogueStore
    return DeviceDialogueStore(dialogues, p, torch.device(DEV), torch.float32)


def _desc(store, pick):
    lengths = [int(store.lengths[d]) if d is not None else 0 for d in pick]
    first = [int(store.offsets[d]) if d is not None else 0 for d in pick]
    return torch.tensor(lengths + first, dtype=torch.int32, device=DEV), lengths


@pytest.mark.parametrize("mods,S,C", CASES)
def test_resident_step_and_resident_eval_step_against_the_oracle(mods, S, C):
    """the batch (17, 0, 1, 33) read from a store of six dialogues through desc: the training step, then resident_eval_step on
    the same dialogues -- logits within 1e-4 and the confusion matrix the float64 oracle's (its top-two gaps are checked first)"""
    pseed, dseed = CM_SEEDS[mods]
    ref = _new_oracle(mods, S, C, pseed)
    tr, p = _trainer(mods, S, C, extra=["--device_collate", "--resident", "--resident_eval"], ref=ref, lr=0.0)
    dialogues = _dialogues(TEST_LENGTHS, S, C, dseed)          # lengths (9, 33, 1, 17, 5, 12)
    store = _store(p, dialogues)
    pick = [3, None, 2, 1]
    desc, lengths = _desc(store, pick)
    assert tuple(lengths) == SLOTS
    exact = _exact_batch([dialogues[d] for d in pick if d is not None], S, C, mods)
    want = _oracle_step(ref, exact)
    top = want[1].topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 1e-3
    batch = tr.resident_batch(store, desc, B_CAP, T_CAP, N_CAP)
    assert batch is not None and all(batch[KEYS[m]].shape[0] == int(store.lengths.sum()) + 1 for m in mods)
    tr.model.dynamic_n = True
    stats = tr.train_step(batch).cpu()
    tr.model.dynamic_n = False
    _check_step(tr.model, stats, want, what="resident %s" % mods)
    # the eval step: a workspace of its own, eval mode whatever the module's flag says, nothing of the training state touched
    tr.model.train()
    state, grad = tr.optim.state.clone(), tr.model.flat.grad.clone()
    cm = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    ews = tr.resident_eval_step(tr.resident_eval_batch(store, desc, B_CAP, T_CAP, N_CAP), cm)
    assert ews is not tr.model._last_ws and tr.model.training and "DGl" in ews and ews["DGl"] is None
    assert torch.equal(tr.optim.state, state) and torch.equal(tr.model.flat.grad, grad)
    assert float((ews["logits"][:N].cpu().double() - want[1]).abs().max()) < 1e-4
    want_cm = np.zeros((C, C), dtype=np.int64)
    np.add.at(want_cm, (exact["label"].numpy(), want[1].argmax(1).numpy()), 1)
    np.testing.assert_array_equal(cm.cpu().numpy(), want_cm)
    tr.model.check_cluster()


@pytest.mark.parametrize("mods,S,C", CASES)
def test_resident_test_epoch_confusion_matrix_equals_the_host_loops(mods, S, C):
    """ResidentEval over the six test dialogues at batch 4 (two steps, the second with two empty slots; a first visit and a
    replay of the one bucket) against the default host loop (StoreLoader batches through to_logits, argmax on the host) and
    against the float64 oracle, whose top-two gap exceeds 1e-3 in every row -- so no row is left out"""
    from erc_amd.trainer import ResidentEval, StoreLoader, test_epoch_loader
    pseed, dseed = CM_SEEDS[mods]
    ref = _new_oracle(mods, S, C, pseed)
    tr, p = _trainer(mods, S, C, extra=["--device_collate", "--resident", "--resident_eval"], ref=ref)
    dialogues = _dialogues(TEST_LENGTHS, S, C, dseed)
    oracle_cm = np.zeros((C, C), dtype=np.int64)
    r64 = copy.deepcopy(ref).double().eval()
    for i in range(0, len(dialogues), 4):
        b = _exact_batch(dialogues[i:i + 4], S, C, mods)
        with torch.no_grad():
            lg, _ = r64(**_dbl(b))
        top = lg.topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) > 1e-3
        np.add.at(oracle_cm, (b["label"].numpy(), lg.argmax(1).numpy()), 1)
    store = _store(p, dialogues)
    ev = ResidentEval(tr, store, 4)
    assert ev.supported() and ev.steps == 2 and ev.caps == [N_CAP, N_CAP] and ev.T == 33
    tr.model.eval()
    cms = [ev.epoch().numpy(), ev.epoch().numpy()]            # the second epoch is replays alone
    assert (ev.captures, ev.eager, ev.replays) == (1, 1, 3)
    true, pred, _, _ = test_epoch_loader(tr, StoreLoader(store, 4, False, 0), False)
    host_cm = np.zeros((C, C), dtype=np.int64)
    np.add.at(host_cm, (np.asarray(true), np.asarray(pred)), 1)
    assert int(host_cm.sum()) == sum(TEST_LENGTHS)
    for cm in cms:
        np.testing.assert_array_equal(cm, host_cm)
        np.testing.assert_array_equal(cm, oracle_cm)
    tr.model.check_cluster()


def test_train_mm_resident_run_reports_graph_replays():
    """``train_mm.py --module=mmgcn ... --device_collate --resident --resident_eval``: two epochs end with finite losses, and
    the epoch lines report graph replays"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(repo, "train_mm.py"), "--module=mmgcn", "--dataset=iemocap-cogmen-6", "--modality=atv",
           "--device_collate", "--resident", "--resident_eval", "--epoch=2", "--n_train=20", "--n_test=6"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=repo, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    losses = [l["Lall"] for l in lines if "Lall" in l]
    epochs = [l for l in lines if "graph_replays" in l]
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses), losses
    assert len(epochs) == 2 and epochs[-1]["graph_replays"] > 0 and epochs[-1]["graphs_captured"] >= 1, epochs
    assert "test_s" in epochs[-1] and 0.0 <= epochs[-1]["test"]["acc"] <= 1.0
