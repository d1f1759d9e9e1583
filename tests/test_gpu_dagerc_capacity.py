"""DAG-ERC in capacity mode on the GPU (DAGERCModule.dynamic_n): the index tables of erc_dag_meta_cap in both input forms
(integer-exact against a numpy restatement), erc_cross_entropy_cap against float64, and the capacity-sized step -- static
buffers, StepGraphs, graph replay, the resident step and a resident epoch -- always against ``oracle.dagerc`` on the batch's
own exact shape, with the tolerances of tests/test_gpu_dagerc.py: logits 1e-4 on the valid rows, loss 1e-5, rel_err < 2e-3
for every live gradient.  Shapes: D = 24, two layers, B_cap = 4, T_cap = 13."""
import functools

import numpy as np
import pytest
import torch

from tests.util_cases import _collate, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = dict(a=8, t=8, v=8)
D, L, B_CAP, T_CAP = 24, 2, 4, 13
N_CAP = B_CAP * T_CAP
LENGTH_SETS = ([13, 1, 0, 7], [0, 0, 0, 5], [13, 13, 13, 13])


# ------------------------------------------------------------------------------------------------ shared, computed once
def _dialogues(lengths, S, C, seed):
    from erc_amd.synthetic import make_dialogues
    return [make_dialogues(1, DIMS, n_speakers=S, n_classes=C, min_len=n, max_len=n, seed=seed * 7919 + i)[0]
            for i, n in enumerate(lengths) if n > 0]


def _exact_batch(dialogues, S, C):
    return _collate(dialogues, S, C, "atv", True, True)


@functools.lru_cache(maxsize=None)
def _oracle(C):
    from oracle.dagerc import DAGERCOracle
    torch.manual_seed(5)
    return DAGERCOracle(emb_dim=D, dropout=0.0, n_classes=C, gnn_layers=L).train()


def _oracle_step(ref, batch):
    """(loss, valid logits [N, C], {name: gradient}) of the oracle on ``batch`` with its present parameters"""
    from oracle.dagerc import dagerc_loss
    torch.set_num_threads(8)
    ref.zero_grad()
    loss, sel = dagerc_loss(ref, batch)
    loss.backward()
    return float(loss.detach()), sel.detach().clone(), {n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}


@functools.lru_cache(maxsize=None)
def _reference(lengths, S, C, seed=3):
    """the exact-shape batch of the non-empty dialogues of ``lengths`` and the oracle's step on it (never modified)"""
    batch = _exact_batch(_dialogues(lengths, S, C, seed), S, C)
    return batch, _oracle_step(_oracle(C), batch)


def _module(C):
    from erc_amd.dagerc import DAGERCModule
    mine = DAGERCModule(emb_dim=D, dropout=0.0, n_classes=C, gnn_layers=L)
    mine.load_state_dict(_oracle(C).state_dict())
    return mine.finalize(DEV).train()


def _static(S):
    """capacity-sized static buffers, filled with what a step must not depend on: features of 3.0, speaker 1 everywhere"""
    spk = torch.zeros(B_CAP, T_CAP, S, device=DEV)
    spk[:, :, 1] = 1.0
    return dict(input_tensor=torch.full((B_CAP, T_CAP, D), 3.0, device=DEV), speaker_tensor=spk,
                text_length=torch.zeros(B_CAP, dtype=torch.int64, device=DEV),
                label=torch.zeros(N_CAP, dtype=torch.int64, device=DEV))


def _place(static, lengths, batch):
    """the dialogues of the exact-shape ``batch`` into the slots of ``lengths`` that are not empty; everything else stays"""
    slots = [b for b, n in enumerate(lengths) if n > 0]
    T = batch["input_tensor"].shape[1]
    for i, b in enumerate(slots):
        static["input_tensor"][b, :T] = batch["input_tensor"][i].to(DEV)
        static["speaker_tensor"][b, :T] = batch["speaker_tensor"][i].to(DEV)
    static["text_length"].copy_(torch.tensor(lengths))
    n = int(batch["label"].shape[0])
    static["label"][:n] = batch["label"].to(DEV)
    static["label"][n:] = 0
    return static


def _check_step(mine, stats, lengths, want, what=""):
    """loss, valid logits and every live gradient of the module's last capacity step against the oracle's"""
    loss, sel, grads = want
    ws = mine._last_ws
    n = sum(lengths)
    rows = ws["node_row"][:n].long()
    got = ws["logits"][rows].cpu()
    assert ws["counts"].tolist() == [n, max(lengths)], what
    assert float((got - sel).abs().max()) < 1e-4, what
    assert abs(float(stats[0]) - loss) < 1e-5, what
    assert set(mine.flat.params) == set(grads)
    for name in mine.flat.params:
        assert rel_err(mine.flat.g(name).cpu(), grads[name]) < 2e-3, (what, name)
    assert bool(torch.isfinite(ws["logits"]).all()) and int((ws["dlogits"] != 0).any(1).sum()) <= n


# ------------------------------------------------------------------------------------------------------------- meta
def _meta_numpy(lengths, spk_valid, T, n_cap):
    """numpy restatement: spk_valid[b] = the speaker ids of slot b's utterances"""
    B = len(lengths)
    spk = np.zeros((B, T), dtype=np.int32)
    for b, ids in enumerate(spk_valid):
        spk[b, :len(ids)] = ids
    pred = np.full((B, T), -1, dtype=np.int32)
    for b in range(B):
        for t in range(T):
            same = [j for j in range(t) if spk[b, j] == spk[b, t]]
            pred[b, t] = same[-1] if same else -1
    node_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    node_row = np.zeros(n_cap, dtype=np.int32)
    rows = [b * T + t for b, n in enumerate(lengths) for t in range(n)]
    node_row[:len(rows)] = rows
    return spk, pred, node_off, node_row, np.array([sum(lengths), max(lengths)], dtype=np.int32)


def _meta_out():
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)
    return dict(spk=i32(B_CAP, T_CAP), pred=i32(B_CAP, T_CAP), node_off=i32(B_CAP + 1), node_row=i32(N_CAP), counts=i32(2),
                x_row=i32(B_CAP * T_CAP), label=torch.full((N_CAP, ), -7, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("S", [2, 9])
@pytest.mark.parametrize("lengths", LENGTH_SETS, ids=str)
def test_meta_cap_bucket_form_is_integer_exact(lengths, S):
    """one-hot and id speakers; padded positions and empty slots hold speaker 1 in the tensors and must come out as 0"""
    from erc_amd import capi
    g = torch.Generator().manual_seed(7)
    valid = [torch.randint(0, S, (n, ), generator=g).tolist() for n in lengths]
    ids = torch.ones(B_CAP, T_CAP, dtype=torch.int64)
    for b, v in enumerate(valid):
        ids[b, :len(v)] = torch.tensor(v, dtype=torch.int64)
    want = _meta_numpy(lengths, valid, T_CAP, N_CAP)
    lens = torch.tensor(lengths, dtype=torch.int64, device=DEV)
    onehot = torch.nn.functional.one_hot(ids, S).float().to(DEV)
    ids = ids.to(DEV)
    for form in ("onehot", "ids"):
        o = _meta_out()
        out = (o["spk"], o["pred"], o["node_off"], o["node_row"], None, None, o["counts"])
        if form == "onehot":
            capi.dag_meta_cap(onehot, None, onehot.stride(0), onehot.stride(1), S, lens, None, None, None, 0, B_CAP, T_CAP, N_CAP, *out)
        else:
            capi.dag_meta_cap(None, ids, ids.stride(0), ids.stride(1), 1 << 30, lens, None, None, None, 0, B_CAP, T_CAP, N_CAP, *out)
        for name, w in zip(("spk", "pred", "node_off", "node_row", "counts"), want):
            np.testing.assert_array_equal(o[name].cpu().numpy(), w, err_msg="%s %s" % (form, name))
        assert int((o["x_row"] != -7).sum()) == 0 and int((o["label"] != -7).sum()) == 0      # not the bucket form's to write
        # the valid rows are erc_dag_meta's own
        if sum(lengths) == N_CAP and form == "onehot":
            e = _meta_out()
            capi.dag_meta(onehot, None, onehot.stride(0), onehot.stride(1), S, lens, B_CAP, T_CAP, e["spk"], e["pred"],
                          e["node_off"], e["node_row"])
            for name in ("spk", "pred", "node_off", "node_row"):
                assert torch.equal(e[name], o[name]), name


@pytest.mark.parametrize("lengths", LENGTH_SETS, ids=str)
def test_meta_cap_resident_form_is_integer_exact(lengths):
    """desc = lengths | first store rows over a store of 9 dialogues visited out of order"""
    from erc_amd import capi
    S = 9
    store_lens = [13, 5, 13, 1, 7, 13, 2, 13, 9]
    offs = np.concatenate([[0], np.cumsum(store_lens)])
    U = int(offs[-1])
    g = torch.Generator().manual_seed(9)
    store_spk = torch.randint(0, S, (U, ), generator=g)
    store_lab = torch.randint(0, 7, (U, ), generator=g)
    pick = []
    for n in lengths:          # a dialogue of each wanted length, none twice, from the back of the store; an empty slot names row 17
        pick.append(next(i for i in reversed(range(9)) if store_lens[i] == n and i not in pick) if n else None)
    first = [int(offs[d]) if d is not None else 17 for d in pick]
    desc = torch.tensor(list(lengths) + first, dtype=torch.int32, device=DEV)
    valid = [store_spk[f:f + n].tolist() for f, n in zip(first, lengths)]
    want = _meta_numpy(lengths, valid, T_CAP, N_CAP)
    x_row = np.full((B_CAP, T_CAP), U, dtype=np.int32)
    for b, (f, n) in enumerate(zip(first, lengths)):
        x_row[b, :n] = f + np.arange(n)
    label = np.zeros(N_CAP, dtype=np.int64)
    rows = x_row[x_row < U]
    label[:len(rows)] = store_lab.numpy()[rows]
    o = _meta_out()
    capi.dag_meta_cap(None, None, 0, 0, 1, None, desc, store_spk.to(DEV), store_lab.to(DEV), U, B_CAP, T_CAP, N_CAP, o["spk"],
                      o["pred"], o["node_off"], o["node_row"], o["x_row"], o["label"], o["counts"])
    for name, w in zip(("spk", "pred", "node_off", "node_row", "counts"), want):
        np.testing.assert_array_equal(o[name].cpu().numpy(), w, err_msg=name)
    np.testing.assert_array_equal(o["x_row"].cpu().numpy(), x_row.reshape(-1))
    np.testing.assert_array_equal(o["label"].cpu().numpy(), label)


def test_meta_cap_refuses_mixed_forms_and_a_t_beyond_the_recurrence():
    from erc_amd import capi
    o = _meta_out()
    out = (o["spk"], o["pred"], o["node_off"], o["node_row"])
    lens = torch.zeros(B_CAP, dtype=torch.int64, device=DEV)
    ids = torch.zeros(B_CAP, T_CAP, dtype=torch.int64, device=DEV)
    desc = torch.zeros(2 * B_CAP, dtype=torch.int32, device=DEV)
    with pytest.raises(capi.ErcGraftError, match="resident form"):
        capi.dag_meta_cap(None, ids, T_CAP, 1, 2, None, desc, ids.view(-1), ids.view(-1), 5, B_CAP, T_CAP, N_CAP, *out, o["x_row"],
                          o["label"], o["counts"])
    with pytest.raises(capi.ErcGraftError, match="bucket form"):
        capi.dag_meta_cap(None, None, T_CAP, 1, 2, lens, None, None, None, 0, B_CAP, T_CAP, N_CAP, *out, None, None, o["counts"])
    with pytest.raises(capi.ErcGraftError, match="T <= 1021"):
        capi.dag_meta_cap(None, ids, T_CAP, 1, 2, lens, None, None, None, 0, B_CAP, 1022, N_CAP, *out, None, None, o["counts"])


# ------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("n_cap,rows", [(40, 52), (600, 640)], ids=["one-workgroup", "three-workgroups"])
def test_cross_entropy_cap_against_float64(n_cap, rows, weighted):
    """n in {0, 1, n_cap - 1, n_cap} through a permuted row map.  Samples at or beyond n map to one row of NaN logits: reading
    it would turn the loss into NaN, writing its gradient would replace the sentinel.  Bounds: loss 1e-5 (the project's), the
    gradient 1e-6 absolute (entries are at most 1 / n; fp32 exp / log carry a few 1e-7 relative)."""
    from erc_amd import capi
    C = 6
    g = torch.Generator().manual_seed(13)
    logits = 2.0 * torch.randn(rows, C, generator=g)
    nan_row = rows - 1
    logits[nan_row] = float("nan")
    perm = torch.randperm(rows - 1, generator=g)[:n_cap].to(torch.int32)
    labels = torch.randint(0, C, (n_cap, ), generator=g)
    weight = (0.5 + torch.rand(C, generator=g)) if weighted else None
    logits_d, stats = logits.to(DEV), torch.zeros(256, device=DEV)
    n_dev = torch.zeros(2, dtype=torch.int32, device=DEV)
    for n in (0, 1, n_cap - 1, n_cap):
        row_map = perm.clone()
        row_map[n:] = nan_row
        dl = torch.full((rows, C), 7.0, device=DEV)
        n_dev[0] = n
        capi.cross_entropy_cap(logits_d, C, C, n_cap, n_dev, row_map.to(DEV), labels.to(DEV), weight.to(DEV) if weighted else None,
                               1.0, dl, C, stats)
        st, dl = stats.cpu(), dl.cpu()
        z = logits[row_map[:n].long()].double()
        y = labels[:n]
        w = weight.double()[y] if weighted else torch.ones(n, dtype=torch.float64)
        lse = torch.logsumexp(z, 1)
        want_loss = float((w * (lse - z[torch.arange(n), y])).sum() / w.sum()) if n else 0.0
        assert abs(float(st[0]) - want_loss) < 1e-5, n
        assert float(st[1]) == float((z.argmax(1) == y).sum()) and abs(float(st[2]) - float(w.sum() if n else 0.0)) < 1e-4, n
        assert int(st[4:5].view(torch.int32)[0]) == 0                    # the arrival counter is back at zero
        want_d = torch.full((rows, C), 7.0, dtype=torch.float64)
        if n:
            d = torch.softmax(z, 1)
            d[torch.arange(n), y] -= 1.0
            want_d[row_map[:n].long()] = d * (w / w.sum())[:, None]
        assert float((dl.double() - want_d).abs().max()) < 1e-6, n      # (untouched rows keep the sentinel exactly)
        assert bool(torch.isfinite(st[:3]).all())


# ------------------------------------------------------------------------------------------------------- the step
@pytest.mark.parametrize("lengths,S,C", [(l, 2, 6) for l in LENGTH_SETS] + [(LENGTH_SETS[0], 9, 7)], ids=str)
def test_capacity_step_against_the_oracle(lengths, S, C):
    batch, want = _reference(tuple(lengths), S, C)
    mine = _module(C)
    static = _place(_static(S), lengths, batch)
    mine.dynamic_n = True
    stats = mine.loss_and_grads(static).cpu()
    mine.dynamic_n = False
    assert mine._last_ws["logits"].shape == (N_CAP, C) and mine._last_ws["node_row"].shape == (N_CAP, )
    _check_step(mine, stats, lengths, want)
    mine.check_cluster()


def test_all_node_counts_share_one_workspace_and_stale_data_does_not_leak():
    """a full batch, then [0, 0, 0, 5] through the SAME static buffers (the full batch's features, speakers and labels stay in
    the slots and rows the small one does not own) and the same workspace: each against its own oracle"""
    S, C = 2, 6
    mine = _module(C)
    static = _static(S)
    mine.dynamic_n = True
    seen = set()
    for lengths in ([13, 13, 13, 13], [0, 0, 0, 5], [13, 1, 0, 7]):
        batch, want = _reference(tuple(lengths), S, C)
        _place(static, lengths, batch)
        stats = mine.loss_and_grads(static).cpu()
        _check_step(mine, stats, lengths, want, str(lengths))
        seen.add(id(mine._last_ws))
    mine.dynamic_n = False
    assert len(seen) == 1 and len(mine._ws) == 1
    mine.check_cluster()


def _trainer(extra=(), lr=None):
    from erc_amd.dagerc import DAGERCTrainer
    from track_mm.dagerc import DAGERCParams
    p = DAGERCParams().from_args(["--dataset=iemocap-cogmen-6", "--train.batch_size=4", "--test.batch_size=4", "--gnn_layers=2",
                                  "--capacity_buckets=True"] + list(extra))
    p.hidden_audio = p.hidden_text = p.hidden_visual = 8            # (the features of this file: D = 24)
    p.hidden_all = D
    tr = DAGERCTrainer(p, DEV)
    if lr is not None:
        tr.optim.lr = lr
    return tr, p


def test_three_optimizer_steps_through_stepgraphs():
    """StepGraphs on the trainer: one eager step on the bucket's static buffers, its capture, two replays.  Before each step the
    module's parameters go into the oracle, so every step is compared on its own."""
    from erc_amd.trainer import StepGraphs
    S, C = 2, 6
    tr, p = _trainer()
    assert tr.model.emb_dim == D and tr.model.gnn_layers == L and tr.model.drop_p == 0.0
    tr.t_cap = T_CAP
    ref = _oracle_copy(C)
    graphs = StepGraphs(tr)
    for step, lengths in enumerate(([13, 1, 7], [5], [13, 13, 13, 12])):
        batch = _exact_batch(_dialogues(lengths, S, C, seed=20 + step), S, C)
        ref.load_state_dict({k: v.cpu() for k, v in tr.model.state_dict().items()})
        want = _oracle_step(ref, batch)
        before = tr.model.flat.data.clone()
        stats = graphs.step(tr.prepare_batch(batch)).cpu()
        _check_step(tr.model, stats, lengths, want, "step %d" % step)
        assert not torch.equal(tr.model.flat.data, before) and int(tr.optim.state[0]) == step + 1
    assert (graphs.captures, graphs.eager, graphs.replays) == (1, 1, 2)
    assert list(graphs.cache) == [("capacity", B_CAP, T_CAP, N_CAP)] and tr.model.dynamic_n is False
    tr.model.check_cluster()


def _oracle_copy(C):
    from oracle.dagerc import DAGERCOracle
    return DAGERCOracle(emb_dim=D, dropout=0.0, n_classes=C, gnn_layers=L).train()


def test_graph_replay_is_bit_identical_to_the_eager_capacity_step():
    """lr = 0 keeps the parameters: the eager step and the replay on the same static buffers must agree bit for bit in the
    statistics, the logits and the whole gradient buffer, for every batch put into the buffers"""
    S, C = 2, 6
    tr, p = _trainer(lr=0.0)
    tr.t_cap = T_CAP
    probe = tr.prepare_batch(_reference((13, 1, 0, 7), S, C)[0])
    key, make, fill = tr.capacity_bucket(probe)
    static = make()
    fill(static, probe)
    tr.model.dynamic_n = True
    tr.train_step(static)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tr.train_step(static)
    grab = lambda st: (st.clone(), tr.model._last_ws["logits"].clone(), tr.model.flat.grad.clone())
    for lengths in ((13, 13, 13, 13), (0, 0, 0, 5), (13, 1, 0, 7)):
        fill(static, tr.prepare_batch(_reference(lengths, S, C)[0]))
        eager = grab(tr.train_step(static))
        tr.model.flat.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, grab(out)):
            assert torch.equal(a, b), lengths
    tr.model.dynamic_n = False
    tr.model.check_cluster()


# ------------------------------------------------------------------------------------------------------- resident
STORE_LENGTHS = (13, 1, 7, 5, 2, 9, 13, 4, 11, 6)


def _store(p, S, C, dtype=torch.float32):
    from erc_amd.datasets import DeviceDialogueStore
    dialogues = _dialogues(STORE_LENGTHS, S, C, seed=31)
    return dialogues, DeviceDialogueStore(dialogues, p, torch.device(DEV), dtype)


def _resident_step(tr, store, pick):
    """one resident training step on the dialogues ``pick`` (None: an empty slot); returns (stats, lengths)"""
    lengths = [int(store.lengths[d]) if d is not None else 0 for d in pick]
    first = [int(store.offsets[d]) if d is not None else 0 for d in pick]
    desc = torch.tensor(lengths + first, dtype=torch.int32, device=DEV)
    batch = tr.resident_batch(store, desc, B_CAP, T_CAP, N_CAP)
    assert batch is not None and batch["input_tensor"].shape[0] == int(store.fused.shape[0]) + 1
    tr.model.dynamic_n = True
    stats = tr.model.loss_and_grads(batch).cpu()
    tr.model.dynamic_n = False
    return stats, lengths


def test_resident_step_against_the_oracle_on_the_same_dialogues():
    S, C = 2, 6
    tr, p = _trainer(extra=["--device_collate", "--resident"])
    dialogues, store = _store(p, S, C)
    ref = _oracle_copy(C)
    ref.load_state_dict({k: v.cpu() for k, v in tr.model.state_dict().items()})
    for pick in ([4, 0, None, 2], [None, None, None, 3], [0, 6, 6, 0]):
        stats, lengths = _resident_step(tr, store, pick)
        want = _oracle_step(ref, _exact_batch([dialogues[d] for d in pick if d is not None], S, C))
        _check_step(tr.model, stats, lengths, want, str(pick))
    assert len(tr.model._ws) == 1
    tr.model.check_cluster()


def test_resident_step_bf16_features_against_the_rounded_oracle():
    """``--compute=bf16``: the store is bf16 and fc1 / the raw-feature block of out_mlp.0 / their weight gradients read it
    through x_row with the gathering bf16 kernels.  The oracle gets the same rounded operands; tolerances are the MODE's, from
    test_dagerc_bf16_feature_mode_vs_rounded_oracle: logits and loss 1e-3, gradients 2 % (3 % for the two bf16-side ones)."""
    from erc_amd.dagerc import HID
    S, C = 2, 6
    tr, p = _trainer(extra=["--device_collate", "--resident", "--compute=bf16"])
    dialogues, store = _store(p, S, C, torch.bfloat16)
    ref = _oracle_copy(C)
    ref.load_state_dict({k: v.cpu() for k, v in tr.model.state_dict().items()})
    W5 = HID * (L + 1)
    with torch.no_grad():
        ref.fc1.weight.copy_(ref.fc1.weight.to(torch.bfloat16).float())
        ref.out_mlp[0].weight[:, W5:] = ref.out_mlp[0].weight[:, W5:].to(torch.bfloat16).float()
    tr.model.load_state_dict(ref.state_dict())
    pick = [4, 0, None, 2]
    stats, lengths = _resident_step(tr, store, pick)
    batch = _exact_batch([dialogues[d] for d in pick if d is not None], S, C)
    batch["input_tensor"] = batch["input_tensor"].to(torch.bfloat16).float()
    loss, sel, grads = _oracle_step(ref, batch)
    ws, n = tr.model._last_ws, sum(lengths)
    got = ws["logits"][ws["node_row"][:n].long()].cpu()
    assert float((got - sel).abs().max()) < 1e-3 and abs(float(stats[0]) - loss) < 1e-3
    errs = {name: rel_err(tr.model.flat.g(name).cpu(), grads[name]) for name in tr.model.flat.params}
    for name, e in errs.items():
        assert e < (3e-2 if name in ("fc1.weight", "out_mlp.0.weight") else 2e-2), sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    tr.model.check_cluster()


def test_resident_epoch_is_one_capture_and_replays():
    """one ResidentEpochs epoch over the 10-dialogue store at B = 4: three steps, ONE capture, the others replays; the epoch's
    loss sum is finite and no recurrence exchange timed out"""
    from erc_amd.trainer import ResidentEpochs
    S, C = 2, 6
    tr, p = _trainer(extra=["--device_collate", "--resident"])
    _, store = _store(p, S, C)
    res = ResidentEpochs(tr, store, B_CAP, seed=3)
    assert res.supported() and res.N_BUCKET == N_CAP
    n_utt, n_steps = res.epoch()
    torch.cuda.synchronize()
    assert (n_utt, n_steps) == (sum(STORE_LENGTHS), 3)
    assert (res.captures, res.eager, res.replays) == (1, 1, 2) and list(res.graphs) == [N_CAP]
    acc = res.acc.cpu()
    assert bool(torch.isfinite(acc).all()) and float(acc[0]) > 0 and int(tr.optim.state[0]) == 3
    tr.model.check_cluster()
