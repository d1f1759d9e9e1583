"""CIM in capacity mode on the GPU (CIMModule.dynamic_n): the tables of erc_cim_meta_cap in both input forms (integer-exact
against a numpy restatement), erc_gru_scan_bwd_cap against erc_gru_scan_bwd, erc_ce_bce_multitask_cap against float64, and the
capacity-sized step -- static buffers, StepGraphs, graph replay, the resident step, eval_scores and a resident test epoch, the
command line -- always against tests/cim_oracle.py (tests/cim_mosei_oracle.py for the multi-task head) on the batch's own exact
shape, with the tolerances tests/test_gpu_cim.py and tests/test_gpu_cim_mosei.py apply to the exact step: logits 1e-4 on the
valid rows, loss 1e-5 absolute (multi-task head: 1e-5 * max(1, |L|) per term, as its file has it), every live gradient within 1e-3 of its largest entry.  Shapes: the feature widths of the cim_tiny
fixture (a 12, t 16, v 20), B_cap = 4, T_cap = 40, N_cap = 128; lengths (17, 0, 1, 33) -- an empty slot, a one-utterance
dialogue, n = 51 < N_cap -- and (40, 40, 40, 8), n == N_cap."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests.cim_mosei_oracle import cim_mosei_loss_and_grads
from tests.cim_oracle import FEATURE, cim_loss_and_grads
from tests.util_cases import fill_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = dict(a=12, t=16, v=20)
B_CAP, T_CAP, N_CAP = 4, 40, 128
LENS, FULL, EDGES = (17, 0, 1, 33), (40, 40, 40, 8), (0, 5, 0, 3)
GRAD_BUFFERS = ("dlogits", "dmerged", "dH", "dGX", "dGH")
FWD_BUFFERS = ("GX", "Hout", "Hdrop", "merged", "logits")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


# ------------------------------------------------------------------------------------------------ shared, computed once
def _classes(multi):
    return 2 if multi else 6


def _dialogues(lengths, multi, seed):
    """sample dicts (the keys datasets.DeviceDialogueStore reads) of the non-empty entries of ``lengths``"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for L in lengths:
        if L == 0:
            continue
        d = {"audio": (torch.randn(L, DIMS["a"], generator=g) * 0.5).numpy(), "text": (torch.randn(L, DIMS["t"], generator=g) * 0.5).numpy(),
             "visual": (torch.randn(L, DIMS["v"], generator=g) * 0.5).numpy(),
             "label": torch.randint(0, _classes(multi), (L, ), generator=g).numpy(), "speakers": [0] if multi else [[1, 0]] * L}
        if multi:
            emo = (torch.rand(L, 7, generator=g) < 0.2).long()
            emo[:, 6] = 0
            emo[emo.sum(1) == 0, 6] = 1
            d["emo_label"], d["senti2_label"] = emo.numpy(), d["label"]
        out.append(d)
    return out


def _exact_batch(dialogues):
    """the collated batch of ``dialogues`` at its own exact shape: batch-first blocks, zero padding"""
    lens = [len(d["label"]) for d in dialogues]
    B, T = len(lens), max(lens)
    batch = {"text_length": torch.tensor(lens, dtype=torch.int64), "speaker_tensor": torch.zeros(B, T, dtype=torch.int64),
             "attention_mask": (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float(),
             "label": torch.from_numpy(np.concatenate([d["label"] for d in dialogues]))}
    for m, key in (("a", "audio"), ("t", "text"), ("v", "visual")):
        x = torch.zeros(B, T, DIMS[m])
        for b, d in enumerate(dialogues):
            x[b, :lens[b]] = torch.from_numpy(d[key])
        batch[FEATURE[m]] = x
    if "emo_label" in dialogues[0]:
        batch["emo_label"] = torch.from_numpy(np.concatenate([d["emo_label"] for d in dialogues]))
        batch["senti2_label"] = batch["label"].clone()
    return batch


@functools.lru_cache(maxsize=None)
def _params(multi):
    """one parameter set per head, as a CPU state_dict (never modified)"""
    from erc_amd.cim import CIMModule
    m = CIMModule(DIMS["t"], DIMS["a"], DIMS["v"], 200, _classes(multi), multitask=multi)
    fill_params(m, 31)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _oracle_step(P, batch, multi, masks=None):
    """(losses, logits2, logits7, gradients) of the CPU restatement: losses = {Lall, Lce, Lmulti} (single task: Lall = Lce)"""
    torch.set_num_threads(8)
    if multi:
        losses, l2, l7, grads, _ = cim_mosei_loss_and_grads(P, batch, masks)
        return {k: float(v) for k, v in losses.items()}, l2, l7, grads
    loss, l2, l7, grads, _ = cim_loss_and_grads(P, batch, masks)
    return {"Lall": float(loss)}, l2, l7, grads


@functools.lru_cache(maxsize=None)
def _reference(lengths, multi, seed=3):
    """the dialogues of ``lengths``, their exact-shape batch and the eval-mode restatement's step on it (never modified)"""
    dialogues = _dialogues(lengths, multi, seed)
    batch = _exact_batch(dialogues)
    return dialogues, batch, _oracle_step(_params(multi), batch, multi)


def _module(multi, drop=0.3):
    from erc_amd.cim import CIMModule
    m = CIMModule(DIMS["t"], DIMS["a"], DIMS["v"], 200, _classes(multi), drop0=drop, drop1=drop, multitask=multi)
    m.load_state_dict(_params(multi))
    return m.finalize(DEV)


def _static(multi):
    """capacity-sized static buffers filled with what a step must not depend on: features of 3.0 in every padded position"""
    s = {FEATURE[m]: torch.full((B_CAP, T_CAP, DIMS[m]), 3.0, device=DEV) for m in "atv"}
    s.update(text_length=torch.zeros(B_CAP, dtype=torch.int64, device=DEV), label=torch.zeros(N_CAP, dtype=torch.int64, device=DEV),
             speaker_tensor=torch.zeros(B_CAP, T_CAP, dtype=torch.int64, device=DEV))
    if multi:
        s["emo_label"] = torch.ones(N_CAP, 7, dtype=torch.int64, device=DEV)
    return s


def _place(static, lengths, batch):
    """the dialogues of the exact-shape ``batch`` into the slots of ``lengths`` that are not empty; everything else stays"""
    slots = [b for b, n in enumerate(lengths) if n > 0]
    T = batch["text_feature"].shape[1]
    for i, b in enumerate(slots):
        for key in FEATURE.values():
            static[key][b, :T] = batch[key][i].to(DEV)
    static["text_length"].copy_(torch.tensor(lengths))
    n = int(batch["label"].shape[0])
    static["label"][:n] = batch["label"].to(DEV)
    if "emo_label" in static:
        static["emo_label"][:n] = batch["emo_label"].to(DEV)
    return static


def _cap_step(m, batch):
    m.dynamic_n = True
    try:
        return m.loss_and_grads(batch).cpu()
    finally:
        m.dynamic_n = False


def _err(a, b):
    return float((a.detach().cpu() - b).abs().max())


def _check_grads(m, grads, multi, tol=1e-3):
    dead = ("rnn_adapter.", ) if multi else ("rnn_adapter.", "cls7.")
    for name, g in grads.items():
        if name.startswith(dead):
            assert g is None, name
            continue
        scale = float(g.abs().max()) + 1e-6
        assert _err(m.flat.g(name), g) <= tol * scale, (name, _err(m.flat.g(name), g), scale)


def _check_loss(stats, losses, multi, what=""):
    """the bounds of the exact step's own tests, in this one place: single task 1e-5 absolute (tests/test_gpu_cim.py), multi-task
    1e-5 * max(1, |L|) on each of Lall, Lce, Lmulti (tests/test_gpu_cim_mosei.py)"""
    if multi:
        for i, k in ((0, "Lall"), (2, "Lce"), (3, "Lmulti")):
            assert abs(float(stats[i]) - losses[k]) < 1e-5 * max(1.0, abs(losses[k])), (what, k, float(stats[i]), losses[k])
    else:
        assert abs(float(stats[0]) - losses["Lall"]) < 1e-5, (what, float(stats[0]), losses["Lall"])


def _check_step(m, stats, lengths, want, multi, what=""):
    """loss, valid logits and every live gradient of the module's last capacity step against the restatement's, and the
    tail invariant: finite forward buffers, gradient buffers exactly zero on the rows [n, N_cap)"""
    losses, l2, l7, grads = want
    ws, n, C = m._last_ws, sum(lengths), _classes(multi)
    assert ws["counts"].tolist() == [n, max(lengths)] and ws["lens"].tolist() == list(lengths), what
    assert ws["logits"].shape[0] == N_CAP and ws["node_row"].shape == (N_CAP, ), what
    assert _err(ws["logits"][:n, :C], l2) < 1e-4, what
    if multi:
        assert _err(ws["logits"][:n, C:], l7) < 1e-4, what
    _check_loss(stats, losses, multi, what)
    _check_grads(m, grads, multi)
    for k in FWD_BUFFERS:
        assert bool(torch.isfinite(ws[k]).all()), (what, k)
    for k in GRAD_BUFFERS:
        tail = ws[k][n:] if ws[k].dim() == 2 else ws[k][:, n:]
        assert int(tail.count_nonzero()) == 0, (what, k)


# ------------------------------------------------------------------------------------------------------------- meta
def _meta_out():
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)
    i64 = lambda *s: torch.full(s, -7, dtype=torch.int64, device=DEV)
    return dict(node_off=i32(B_CAP + 1), node_row=i32(N_CAP), lens=i64(B_CAP), label=i64(N_CAP), emo=i64(N_CAP, 7), counts=i32(2))


def _meta_numpy(lengths, rows_of, tail_row):
    """numpy restatement: rows_of(b, t) = the row node (b, t) gathers"""
    node_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    node_row = np.full(N_CAP, tail_row, dtype=np.int32)
    rows = [rows_of(b, t) for b, n in enumerate(lengths) for t in range(n)]
    node_row[:len(rows)] = rows
    return node_off, node_row, np.asarray(lengths, dtype=np.int64), np.array([sum(lengths), max(lengths)], dtype=np.int32)


@pytest.mark.parametrize("tail_row", [0, B_CAP * T_CAP])
@pytest.mark.parametrize("lengths", [LENS, FULL, EDGES], ids=str)
def test_meta_cap_bucket_form_is_integer_exact(lengths, tail_row):
    o = _meta_out()
    lens = torch.tensor(lengths, dtype=torch.int64, device=DEV)
    capi.cim_meta_cap(lens, None, None, None, tail_row, B_CAP, T_CAP, N_CAP, o["node_off"], o["node_row"], o["lens"], None, None,
                      o["counts"])
    want = _meta_numpy(lengths, lambda b, t: b * T_CAP + t, tail_row)
    for name, w in zip(("node_off", "node_row", "lens", "counts"), want):
        np.testing.assert_array_equal(o[name].cpu().numpy(), w, err_msg=name)
    assert int((o["label"] != -7).sum()) == 0 and int((o["emo"] != -7).sum()) == 0      # not the bucket form's to write
    if sum(lengths) == N_CAP:      # the valid rows are erc_cim_meta's own
        e = _meta_out()
        capi.cim_meta(lens, B_CAP, T_CAP, N_CAP, e["node_off"], e["node_row"])
        assert torch.equal(e["node_off"], o["node_off"]) and torch.equal(e["node_row"], o["node_row"])


def test_meta_cap_clamps_lengths_to_t_cap_and_to_what_n_cap_holds():
    o = _meta_out()
    lens = torch.tensor([45, -3, 40, 40], dtype=torch.int64, device=DEV)
    capi.cim_meta_cap(lens, None, None, None, 0, B_CAP, T_CAP, 100, o["node_off"], o["node_row"], o["lens"], None, None, o["counts"])
    assert o["lens"].tolist() == [40, 0, 40, 20] and o["node_off"].tolist() == [0, 40, 40, 80, 100]
    assert o["counts"].tolist() == [100, 40] and o["node_row"][99].item() == 3 * T_CAP + 19 and o["node_row"][100].item() == -7


@pytest.mark.parametrize("with_emo", [False, True], ids=["label", "label+emo"])
@pytest.mark.parametrize("lengths", [LENS, FULL, EDGES], ids=str)
def test_meta_cap_resident_form_is_integer_exact(lengths, with_emo):
    """desc = lengths | first store rows over a store of 9 dialogues visited out of order; an empty slot names row 17"""
    store_lens = [40, 5, 33, 1, 17, 40, 3, 40, 8]
    offs = np.concatenate([[0], np.cumsum(store_lens)])
    U = int(offs[-1])
    g = torch.Generator().manual_seed(9)
    store_lab = torch.randint(0, 6, (U, ), generator=g)
    store_emo = torch.randint(0, 2, (U, 7), generator=g)
    pick = []
    for n in lengths:
        pick.append(next(i for i in reversed(range(9)) if store_lens[i] == n and i not in pick) if n else None)
    first = [int(offs[d]) if d is not None else 17 for d in pick]
    desc = torch.tensor(list(lengths) + first, dtype=torch.int32, device=DEV)
    o = _meta_out()
    capi.cim_meta_cap(None, desc, store_lab.to(DEV), store_emo.to(DEV) if with_emo else None, U, B_CAP, T_CAP, N_CAP, o["node_off"],
                      o["node_row"], o["lens"], o["label"], o["emo"] if with_emo else None, o["counts"])
    want = _meta_numpy(lengths, lambda b, t: first[b] + t, U)
    for name, w in zip(("node_off", "node_row", "lens", "counts"), want):
        np.testing.assert_array_equal(o[name].cpu().numpy(), w, err_msg=name)
    n = sum(lengths)
    rows = want[1][:n]
    label, emo = np.zeros(N_CAP, dtype=np.int64), np.zeros((N_CAP, 7), dtype=np.int64)
    label[:n], emo[:n] = store_lab.numpy()[rows], store_emo.numpy()[rows]
    np.testing.assert_array_equal(o["label"].cpu().numpy(), label)
    np.testing.assert_array_equal(o["emo"].cpu().numpy(), emo if with_emo else np.full((N_CAP, 7), -7))


def test_meta_cap_refuses_mixed_forms_and_a_t_beyond_the_attention_before_launch():
    o = _meta_out()
    out = (o["node_off"], o["node_row"], o["lens"])
    lens = torch.zeros(B_CAP, dtype=torch.int64, device=DEV)
    desc = torch.zeros(2 * B_CAP, dtype=torch.int32, device=DEV)
    lab = torch.zeros(50, dtype=torch.int64, device=DEV)
    with pytest.raises(capi.ErcGraftError, match="one of them"):
        capi.cim_meta_cap(lens, desc, None, None, 0, B_CAP, T_CAP, N_CAP, *out, None, None, o["counts"])
    with pytest.raises(capi.ErcGraftError, match="one of them"):
        capi.cim_meta_cap(None, None, None, None, 0, B_CAP, T_CAP, N_CAP, *out, None, None, o["counts"])
    with pytest.raises(capi.ErcGraftError, match="bucket form"):
        capi.cim_meta_cap(lens, None, lab, None, 0, B_CAP, T_CAP, N_CAP, *out, o["label"], None, o["counts"])
    with pytest.raises(capi.ErcGraftError, match="store_label with label_out"):
        capi.cim_meta_cap(None, desc, lab, None, 50, B_CAP, T_CAP, N_CAP, *out, None, None, o["counts"])
    with pytest.raises(capi.ErcGraftError, match="up to 118 utterances"):
        capi.cim_meta_cap(lens, None, None, None, 0, B_CAP, 119, N_CAP, *out, None, None, o["counts"])
    with pytest.raises(capi.ErcGraftError, match="n_cap <= B \\* T"):
        capi.cim_meta_cap(lens, None, None, None, 0, B_CAP, T_CAP, B_CAP * T_CAP + 1, *out, None, None, o["counts"])
    torch.cuda.synchronize()
    assert all(int((v != -7).sum()) == 0 for v in o.values())      # nothing was launched


# ------------------------------------------------------------------------------------------------------------- scans
@pytest.mark.parametrize("lengths", [LENS, FULL], ids=str)
def test_gru_scans_with_empty_slots_and_the_zeroed_tail(lengths):
    """forward: a slot of length 0 runs no step and rows >= n keep a NaN sentinel, the valid rows equal those of a launch over
    the non-empty dialogues alone.  backward: erc_gru_scan_bwd_cap equals erc_gru_scan_bwd on the rows < n and writes exact
    zeros on [n, zero_to) of NaN-prefilled dGX / dGH, nothing beyond zero_to; zero_to = 0 is erc_gru_scan_bwd"""
    n, zero_to = sum(lengths), N_CAP - 3
    g = torch.Generator().manual_seed(4)
    GX = (torch.randn(3, N_CAP, 1200, generator=g) * 0.5).to(DEV)
    W = (torch.randn(6, 600, 200, generator=g) * 0.05).to(DEV)
    WT = W.transpose(1, 2).contiguous()
    bhh = (torch.randn(6, 600, generator=g) * 0.05).to(DEV)
    dH = torch.randn(3, N_CAP, 400, generator=g).to(DEV)
    rng = torch.tensor([5, 7], dtype=torch.int64, device=DEV)
    lens = torch.tensor(lengths, dtype=torch.int64, device=DEV)
    node_off = torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device=DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)

    def forward(lens, node_off, B):
        out = dict(Hout=nan(3, N_CAP, 400), Hdrop=nan(3, N_CAP, 400), gates=nan(3, N_CAP, 1200), ghn=nan(3, N_CAP, 400),
                   Hprev=nan(3, N_CAP, 400))
        capi.gru_scan_fwd(GX, WT, bhh, lens, node_off, B, T_CAP, N_CAP, out["Hout"], out["Hdrop"], 0.3, rng, 11, out["gates"],
                          out["ghn"], out["Hprev"])
        return out
    cap = forward(lens, node_off, B_CAP)
    full = [b for b, L in enumerate(lengths) if L > 0]
    dense = forward(lens[full].contiguous(), torch.cat([node_off[full], node_off[-1:]]).contiguous(), len(full))
    for k, v in cap.items():
        assert bool(torch.isnan(v[:, n:]).all()) and bool(torch.isfinite(v[:, :n]).all()), k
        assert torch.equal(v[:, :n], dense[k][:, :n]), k
    args = (W, lens, node_off, B_CAP, T_CAP, N_CAP, cap["gates"], cap["ghn"], cap["Hprev"], dH, 0.3, rng, 11)
    exact = (nan(3, N_CAP, 1200), nan(3, N_CAP, 1200))
    capi.gru_scan_bwd(*args, *exact)
    for z in (zero_to, 0, N_CAP):
        got = (nan(3, N_CAP, 1200), nan(3, N_CAP, 1200))
        capi.gru_scan_bwd_cap(*args, *got, z)
        for a, e in zip(got, exact):
            assert torch.equal(a[:, :n], e[:, :n]) and bool(torch.isfinite(a[:, :n]).all())
            assert int(a[:, n:max(n, z)].count_nonzero()) == 0 and bool(torch.isnan(a[:, max(n, z):]).all()), z
    with pytest.raises(capi.ErcGraftError, match="zero_to"):
        capi.gru_scan_bwd_cap(*args, *exact, N_CAP + 1)


# ------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("n_cap", [128, 600], ids=["one-workgroup", "three-workgroups"])
def test_ce_bce_multitask_cap_against_float64(n_cap):
    """n in {0, 1, 51, n_cap}.  Rows at or beyond n hold NaN logits and labels far outside the classes: reading one would turn
    the loss into NaN.  Their dlogits rows are written exactly 0 over a sentinel; the columns past C + 7 keep it.  Bounds: loss
    1e-5, the gradient 1e-6 absolute (entries are at most 1 / n), as test_cross_entropy_cap_against_float64."""
    C, pitch = 2, 12
    g = torch.Generator().manual_seed(n_cap)
    x = torch.randn(n_cap, pitch, generator=g) * 4
    labels = torch.randint(0, C, (n_cap, ), generator=g)
    emo = (torch.rand(n_cap, 9, generator=g) < 0.3).long()      # read through a row pitch of 9
    stats, n_dev = torch.zeros(256, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    for n in (0, 1, 51, n_cap):
        xd, yd, ed = x.clone(), labels.clone(), emo.clone()
        xd[n:], yd[n:], ed[n:] = float("nan"), 1 << 40, 1 << 40
        d = torch.full((n_cap, pitch), 7.0, device=DEV)
        n_dev[0] = n
        ed = ed.to(DEV)
        capi.ce_bce_multitask_cap(xd.to(DEV), pitch, C, n_cap, n_dev, yd.to(DEV), ed[:, :7], ed.stride(0), 1.0, 1.0, 1.0, d, pitch,
                                  stats)
        st, d = stats.cpu(), d.cpu()
        z = x[:n, :C + 7].double().requires_grad_(True)
        want = torch.full((n_cap, pitch), 7.0, dtype=torch.float64)
        want[:, :C + 7] = 0.0
        lce = lmulti = torch.zeros((), dtype=torch.float64)
        if n:
            lce = torch.nn.functional.cross_entropy(z[:, :C], labels[:n])
            lmulti = torch.nn.functional.binary_cross_entropy_with_logits(z[:, C:], emo[:n, :7].double())
            (lce + lmulti).backward()
            want[:n, :C + 7] = z.grad
        for got, w in ((st[0], lce + lmulti), (st[2], lce), (st[3], lmulti)):
            assert abs(float(got) - float(w.detach())) < 1e-5, (n, float(got), float(w.detach()))
        assert int(st[1]) == (int((x[:n, :C].argmax(-1) == labels[:n]).sum()) if n else 0), n
        assert bool(torch.isfinite(st[:4]).all()) and int(st[4:5].view(torch.int32)[0]) == 0      # the counter is back at zero
        assert float((d.double() - want).abs().max()) < 1e-6, n
        assert int(d[n:, :C + 7].count_nonzero()) == 0 and torch.equal(d[:, C + 7:], torch.full((n_cap, pitch - C - 7), 7.0)), n
        if n == n_cap:      # a full batch is the exact form, bit for bit
            d2, s2 = torch.full((n_cap, pitch), 7.0, device=DEV), torch.zeros(256, device=DEV)
            capi.ce_bce_multitask(x.to(DEV), pitch, C, n_cap, labels.to(DEV), ed[:, :7], ed.stride(0), 1.0, 1.0, 1.0, d2, pitch, s2)
            assert torch.equal(d2.cpu(), d) and torch.equal(s2.cpu()[:4], st[:4])


# ------------------------------------------------------------------------------------------------------- the step
@pytest.mark.parametrize("lengths,multi", [(LENS, False), (LENS, True), (FULL, False), (FULL, True), (EDGES, False), (EDGES, True)],
                         ids=str)
def test_capacity_step_against_the_oracle(lengths, multi):
    """eval mode, hand-made static buffers (3.0 in every padded position; the tail nodes gather row 0): (17, 0, 1, 33) has its
    empty slot in the middle, (0, 5, 0, 3) starts with one, (40, 40, 40, 8) fills the capacity"""
    _, batch, want = _reference(lengths, multi)
    m = _module(multi).eval()
    stats = _cap_step(m, _place(_static(multi), lengths, batch))
    _check_step(m, stats, lengths, want, multi)
    assert int(stats[1]) == int((want[1].argmax(-1) == batch["label"]).sum())          # #correct counts the batch's rows alone
    assert int(m._last_ws["node_row"][sum(lengths):].abs().sum()) == 0


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multitask"])
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_stale_data_does_not_leak(multi, training):
    """a full batch, then (17, 0, 1, 33) through the SAME static buffers and the same workspace, against that small batch in a
    fresh module's fresh workspace: the loss and every gradient bit for bit (the tail rows differ -- zeros there, the full
    batch's rows here -- and must not matter)"""
    m = _module(multi).train(training)
    static = _static(multi)
    _cap_step(m, _place(static, FULL, _reference(FULL, multi)[1]))
    big_ws = m._last_ws
    assert int(big_ws["dGX"][:, 51:].count_nonzero()) > 0 and int(big_ws["dlogits"][51:].count_nonzero()) > 0
    stats = _cap_step(m, _place(static, LENS, _reference(LENS, multi)[1]))
    assert m._last_ws is big_ws and len(m._ws) == 1
    fresh = _module(multi).train(training)
    want = _cap_step(fresh, _place(_static(multi), LENS, _reference(LENS, multi)[1]))
    assert torch.equal(stats[:4], want[:4]) and torch.equal(m.flat.grad, fresh.flat.grad)
    assert int(m._last_ws["Hout"][:, 51:].count_nonzero()) > 0 and int(fresh._last_ws["Hout"][:, 51:].count_nonzero()) == 0
    if not training:
        _check_step(m, stats, LENS, _reference(LENS, multi)[2], multi)


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multitask"])
def test_training_mode_draws_the_exact_shape_step_s_masks(multi):
    """drop0 (keyed by row * 400 + column) and drop1 (row * 100 + column) do not see the row count: from the same rng_state the
    capacity step draws the masks of the exact-shape step on the same dialogues -- read back from Hdrop and the dense block --
    and loss and gradients agree within the bounds both have against the restatement"""
    _, batch, _ = _reference(LENS, multi)
    exact = _module(multi).train()
    want = exact.loss_and_grads({k: v.to(DEV) for k, v in batch.items()}).cpu()
    cap = _module(multi).train()
    stats = _cap_step(cap, _place(_static(multi), LENS, batch))
    we, wc, n = exact._last_ws, cap._last_ws, 51
    assert torch.equal(we["Hdrop"] != 0, wc["Hdrop"][:, :n] != 0) and torch.equal(we["merged"][:, 600:] != 0, wc["merged"][:n, 600:] != 0)
    keep = float((we["Hdrop"] != 0).float().mean())
    assert 0.6 < keep < 0.8
    assert _err(wc["Hdrop"][:, :n], we["Hdrop"].cpu()) < 1e-5 and _err(wc["logits"][:n], we["logits"].cpu()) < 1e-4
    _check_loss(stats, {"Lall": float(want[0]), "Lce": float(want[2]), "Lmulti": float(want[3])}, multi)
    for name in exact.flat.params:
        g = exact.flat.g(name).cpu()
        assert _err(cap.flat.g(name), g) <= 1e-3 * (float(g.abs().max()) + 1e-6), name


# ------------------------------------------------------------------------------------------------------- trainer level
def _trainer(multi=False, extra=(), lr=None, drop=None):
    from erc_amd.cim import CIMTrainer
    from track_mm.cim import CIMParams
    p = CIMParams().from_args(["--dataset=" + ("mosei-cim-2" if multi else "iemocap-cogmen-6"), "--train.batch_size=4",
                               "--test.batch_size=4", "--capacity_buckets=True"] + list(extra))
    p.hidden_audio, p.hidden_text, p.hidden_visual = DIMS["a"], DIMS["t"], DIMS["v"]      # (the features of this file)
    tr = CIMTrainer(p, DEV)
    tr.model.load_state_dict(_params(multi))
    if lr is not None:
        tr.optim.lr = lr
    if drop is not None:
        tr.model.p0 = tr.model.p1 = drop
    return tr, p


def _cpu_params(tr):
    return {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multitask"])
def test_three_optimizer_steps_through_stepgraphs(multi):
    """StepGraphs on the trainer (dropout off, so that each step has a restatement): one eager step on the bucket's static
    buffers -- the trainer's own, with the zero row behind every block --, its capture, two replays.  Before each step the
    module's parameters go into the restatement, so every step is compared on its own."""
    from erc_amd.trainer import StepGraphs
    tr, p = _trainer(multi, drop=0.0)
    tr.t_cap = T_CAP
    graphs = StepGraphs(tr)
    for step, lengths in enumerate(((17, 1, 33), (5, ), (40, 40, 40, 7))):
        batch = _exact_batch(_dialogues(lengths, multi, seed=20 + step))
        want = _oracle_step(_cpu_params(tr), batch, multi)
        before = tr.model.flat.data.clone()
        stats = graphs.step(tr.prepare_batch(batch)).cpu()
        ws, n = tr.model._last_ws, sum(lengths)
        assert ws["counts"].tolist() == [n, max(lengths)]
        assert int((ws["node_row"][n:] != B_CAP * T_CAP).sum()) == 0          # the tail nodes gather the bucket's zero row
        assert _err(ws["logits"][:n, :_classes(multi)], want[1]) < 1e-4
        _check_loss(stats, want[0], multi, "step %d" % step)
        _check_grads(tr.model, want[3], multi)
        assert int(ws["dGX"][:, n:].count_nonzero()) == 0 and int(ws["dlogits"][n:].count_nonzero()) == 0
        assert not torch.equal(tr.model.flat.data, before) and int(tr.optim.state[0]) == step + 1
    assert (graphs.captures, graphs.eager, graphs.replays) == (1, 1, 2)
    assert list(graphs.cache) == [("capacity", B_CAP, T_CAP, N_CAP)] and tr.model.dynamic_n is False


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multitask"])
def test_graph_replay_is_bit_identical_to_the_eager_capacity_step(multi):
    """training mode, lr = 0 and the dropout counter put back before every step: the eager step and the replay on the same
    static buffers must agree bit for bit in the statistics, the logits and the whole gradient buffer, for every batch"""
    tr, p = _trainer(multi, lr=0.0)
    tr.t_cap = T_CAP
    prep = lambda lengths: tr.prepare_batch(_reference(lengths, multi)[1])
    key, make, fill = tr.capacity_bucket(prep(LENS))
    assert key == ("capacity", B_CAP, T_CAP, N_CAP)
    static = make()
    fill(static, prep(LENS))
    tr.model.dynamic_n = True
    tr.train_step(static)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tr.train_step(static)
    grab = lambda st: (st[:4].clone(), tr.model._last_ws["logits"].clone(), tr.model.flat.grad.clone())
    for lengths in (FULL, EDGES, LENS):
        fill(static, prep(lengths))
        tr.optim.state[1:2].zero_()
        eager = grab(tr.train_step(static))
        tr.model.flat.grad.zero_()
        tr.optim.state[1:2].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, grab(out)):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), lengths
    tr.model.dynamic_n = False


# ------------------------------------------------------------------------------------------------------- resident
STORE_LENGTHS = (17, 1, 33, 5, 40, 9, 40, 40, 8, 22)


def _store(p, multi):
    from erc_amd.datasets import DeviceDialogueStore
    dialogues = _dialogues(STORE_LENGTHS, multi, seed=31)
    return dialogues, DeviceDialogueStore(dialogues, p, torch.device(DEV))


def _desc(store, pick):
    lengths = [int(store.lengths[d]) if d is not None else 0 for d in pick]
    first = [int(store.offsets[d]) if d is not None else 0 for d in pick]
    return torch.tensor(lengths + first, dtype=torch.int32, device=DEV), lengths


@pytest.mark.parametrize("multi", [False, True], ids=["iemocap", "mosei"])
def test_resident_step_against_the_oracle_on_the_same_dialogues(multi):
    tr, p = _trainer(multi, extra=["--device_collate", "--resident"])
    dialogues, store = _store(p, multi)
    assert ("emo_label" in store.extra) is multi
    tr.model.eval()
    for pick in ([0, None, 1, 2], [None, None, None, 3], [4, 6, 7, 8]):
        desc, lengths = _desc(store, pick)
        batch = tr.resident_batch(store, desc, B_CAP, T_CAP, N_CAP)
        assert batch is not None and batch["text_feature"].shape == (int(store.label.shape[0]) + 1, DIMS["t"])
        stats = _cap_step(tr.model, batch)
        want = _oracle_step(_params(multi), _exact_batch([dialogues[d] for d in pick if d is not None]), multi)
        ws, n, U = tr.model._last_ws, sum(lengths), int(store.label.shape[0])
        assert ws["counts"].tolist() == [n, max(lengths)] and int((ws["node_row"][n:] != U).sum()) == 0
        assert _err(ws["logits"][:n, :_classes(multi)], want[1]) < 1e-4
        _check_loss(stats, want[0], multi, str(pick))
        _check_grads(tr.model, want[3], multi)
        for k in GRAD_BUFFERS:
            tail = ws[k][n:] if ws[k].dim() == 2 else ws[k][:, n:]
            assert int(tail.count_nonzero()) == 0, (pick, k)
    assert len(tr.model._ws) == 1


def test_eval_scores_is_numpy_s_confusion_matrix_of_the_exact_step():
    """eval_scores on a static capacity batch and on a resident one: the confusion matrix of the exact-shape forward's argmax,
    added to what ``cm`` held; the training flag, the dropout counter and the training workspaces stay as they were"""
    tr, p = _trainer(extra=["--device_collate", "--resident"])
    dialogues, store = _store(p, False)
    tr.model.train()
    rng = tr.model.rng_state.clone()
    cm = torch.zeros(6, 6, dtype=torch.int64, device=DEV)
    want = np.zeros((6, 6), dtype=np.int64)
    for pick in ([0, None, 1, 2], [4, 6, 7, 8]):
        batch = _exact_batch([dialogues[d] for d in pick if d is not None])
        tr.model.eval()
        pred = tr.to_logits(tr.prepare_batch(batch)).argmax(-1).cpu().numpy()
        tr.model.train()
        np.add.at(want, (batch["label"].numpy(), pred), 1)
        desc, lengths = _desc(store, pick)
        ws = tr.model.eval_scores(tr.resident_batch(store, desc, B_CAP, T_CAP, N_CAP), cm)
        assert ws["dlogits"] is None and ws is not tr.model._last_ws
        np.testing.assert_array_equal(cm.cpu().numpy(), want)
    static = _place(_static(False), LENS, _reference(LENS, False)[1])
    tr.model.eval_scores(static, cm)
    l2, label = _reference(LENS, False)[2][1], _reference(LENS, False)[1]["label"]
    np.add.at(want, (label.numpy(), l2.argmax(-1).numpy()), 1)
    np.testing.assert_array_equal(cm.cpu().numpy(), want)
    assert tr.model.training and torch.equal(tr.model.rng_state, rng) and int(want.sum()) == 51 + 128 + 51


def test_a_resident_test_epoch_equals_the_default_test_loop():
    """ResidentEval over the 10-dialogue store at B = 4 (three steps, the last with two empty slots) against the host loop's
    confusion matrix, twice: the second epoch is replays alone"""
    from erc_amd.trainer import ResidentEval, StoreLoader, test_epoch_loader
    tr, p = _trainer(extra=["--device_collate", "--resident", "--resident_eval"])
    _, store = _store(p, False)
    tr.model.eval()
    true, pred, _, _ = test_epoch_loader(tr, StoreLoader(store, 4, False, 0), False)
    want = np.zeros((6, 6), dtype=np.int64)
    np.add.at(want, (np.asarray(true), np.asarray(pred)), 1)
    ev = ResidentEval(tr, store, 4)
    assert ev.supported() and ev.steps == 3 and ev.T == 40
    for _ in range(2):
        np.testing.assert_array_equal(ev.epoch().numpy(), want)
    assert ev.captures == len(set(ev.caps)) and ev.replays == 6 - ev.eager and int(want.sum()) == sum(STORE_LENGTHS)


# ------------------------------------------------------------------------------------------------------- command line
def _cli(dataset, extra):
    args = ["--module=cim", "--dataset=" + dataset, "--modality=atv", "--epoch=2", "--n_train=12", "--n_test=6", "--syn_min_len=33",
            "--syn_max_len=40", "--train.batch_size=4", "--test.batch_size=4", "--device_collate"] + extra
    res = subprocess.run([sys.executable, "train_mm.py"] + args, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    losses = [l for l in lines if "Lall" in l]
    epochs = [l for l in lines if "test" in l]
    assert len(epochs) == 2 and losses and all(np.isfinite(l["Lall"]) for l in losses)
    return losses, epochs


def test_train_mm_cli_resident_and_resident_eval_report_the_same_metrics():
    """two resident epochs on IEMOCAP-shaped dialogues, the test epochs once through the host loop and once from HBM: the same
    training (bit-identical epoch losses) and the same test metrics"""
    l_host, e_host = _cli("iemocap-cogmen-6", ["--resident"])
    l_dev, e_dev = _cli("iemocap-cogmen-6", ["--resident", "--resident_eval"])
    assert [l["Lall"] for l in l_host] == [l["Lall"] for l in l_dev]
    for a, b in zip(e_host, e_dev):
        assert a["graph_replays"] > 0 and b["graph_replays"] > 0 and "test_s" in b and "test_s" not in a
        for k in ("acc", "wa", "pre", "rec", "f1", "mif1", "maf1"):
            assert abs(a["test"][k] - b["test"][k]) < 1e-9, k


def test_train_mm_cli_resident_on_mosei_keeps_the_host_test_loop():
    losses, epochs = _cli("mosei-cim-2", ["--resident"])
    assert all(e["graph_replays"] > 0 and len(e["multiemo"]["acc"]) == 7 and "test_s" not in e for e in epochs)
    res = subprocess.run([sys.executable, "train_mm.py", "--module=cim", "--dataset=mosei-cim-2", "--device_collate", "--resident",
                          "--resident_eval", "--epoch=1", "--n_train=8", "--n_test=4"], cwd=REPO, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode != 0 and "multi-label metrics" in res.stderr
