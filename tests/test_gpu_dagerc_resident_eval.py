"""GPU: DAG-ERC ``--resident_eval`` -- erc_rows_score through the C-ABI against numpy, the ResidentEval test epoch against the
default host loop's confusion matrix (exact: the oracle's smallest top-2 logit gap over the test utterances is asserted to be
above ten times the logit tolerance first), the training state across test epochs, and ``train_mm.py --module=dagerc
--device_collate --resident --resident_eval`` as a child process."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, L = 24, 2
TEST_LENGTHS = (1, 2, 13, 5, 13, 13, 13, 13, 7, 11, 3)      # B = 4: the second batch fills its bucket, the last has an empty slot
TRAIN_LENGTHS = (12, 3, 13, 7, 10, 9, 2, 8)
SEED = 5               # --seed of the trainer, chosen on the CPU with _min_gap(): 1.07e-1 here (seed 6 would give 5.2e-4)
GAP = 1e-3             # ten times the logit tolerance of tests/test_gpu_dagerc.py


# ----------------------------------------------------------------------------------------------------- erc_rows_score
def _cm_numpy(logits, row_map, labels, n, C):
    cm = np.zeros((C, C), dtype=np.int64)
    for i in range(n):
        z = logits[row_map[i]]
        if np.all(np.isnan(z)) or not 0 <= labels[i] < C:
            continue
        cm[labels[i], int(np.nanargmax(z))] += 1          # (the first index of the maximum; a NaN never wins)
    return cm


@pytest.mark.parametrize("C,n_cap,rows", [(6, 52, 52), (7, 700, 900), (16, 300, 300)], ids=["c6", "c7-three-workgroups", "c16"])
def test_rows_score_against_numpy(C, n_cap, rows):
    """constructed ties (the first index wins), labels outside [0, C), a permuted row map, NaN logits, n in {0, k, n_cap}; cm is
    added to.  Samples at or beyond n map to a row whose maximum is class C - 1 and carry label C - 1: counting any of them
    would show in that cell."""
    from erc_amd import capi
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(rows, C, generator=g)
    logits[0] = 1.5                                        # all equal: class 0
    logits[1, 2:] = logits[1, 2]                           # ties among the upper classes
    logits[2, 1], logits[2, C - 1] = 9.0, 9.0              # two equal maxima: the lower index
    logits[3, 0] = float("nan")                            # a NaN never wins
    logits[4] = float("nan")                               # nothing but NaN: not counted
    logits[5, C - 1] = 50.0                                # the row the uncounted samples map to
    perm = torch.randperm(rows, generator=g)[:n_cap]
    perm[:6] = torch.tensor([3, 0, 2, 1, 4, 0])            # the constructed rows come first, so every n > 0 meets some
    labels = torch.randint(0, C, (n_cap, ), generator=g)
    labels[7], labels[8] = -1, C                           # out of range: not counted
    logits_d = logits.to(DEV)
    n_dev = torch.zeros(2, dtype=torch.int32, device=DEV)
    cm = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    want = np.zeros((C, C), dtype=np.int64)
    for n in (0, 11, n_cap, 11):
        row_map, lab = perm.clone(), labels.clone()
        row_map[n:], lab[n:] = 5, C - 1
        n_dev[0] = n
        capi.rows_score(logits_d, C, rows, C, n_cap, n_dev, row_map.to(torch.int32).to(DEV), lab.to(DEV), cm)
        want += _cm_numpy(logits.numpy(), row_map.numpy(), lab.numpy(), n, C)
        np.testing.assert_array_equal(cm.cpu().numpy(), want, err_msg="n = %d" % n)      # (added to: ``want`` accumulates too)
    assert 0 < int(want.sum()) < 22 + n_cap                 # (the all-NaN row and the two labels out of range are missing)
    assert torch.equal(logits_d.cpu().isnan(), logits.isnan())      # the launch writes nothing but cm
    with pytest.raises(capi.ErcGraftError, match="C <= 16"):
        capi.rows_score(logits_d, C, rows, 17, n_cap, n_dev, None, labels.to(DEV), cm)


def test_rows_score_without_a_row_map_and_with_rows_outside_the_logits():
    from erc_amd import capi
    C, rows = 6, 40
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(rows, C, generator=g)
    labels = torch.randint(0, C, (rows, ), generator=g)
    n_dev = torch.tensor([33, 0], dtype=torch.int32, device=DEV)
    cm = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    capi.rows_score(logits.to(DEV), C, rows, C, rows, n_dev, None, labels.to(DEV), cm)
    np.testing.assert_array_equal(cm.cpu().numpy(), _cm_numpy(logits.numpy(), np.arange(rows), labels.numpy(), 33, C))
    # a row index outside [0, n_logit_rows) is neither read nor counted; a count above n_cap is clamped
    row_map = torch.arange(rows, dtype=torch.int32)
    row_map[0], row_map[1] = -1, rows
    n_dev[0] = rows + 100
    cm.zero_()
    capi.rows_score(logits.to(DEV), C, rows, C, rows, n_dev, row_map.to(DEV), labels.to(DEV), cm)
    want = _cm_numpy(logits.numpy(), np.arange(rows), labels.numpy(), rows, C) - _cm_numpy(logits.numpy(), np.arange(rows), labels.numpy(), 2, C)
    np.testing.assert_array_equal(cm.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------- the whole path
def _params(extra=()):
    from track_mm.dagerc import DAGERCParams
    p = DAGERCParams().from_args(["--dataset=iemocap-cogmen-6", "--train.batch_size=4", "--test.batch_size=4", "--gnn_layers=2",
                                  "--device_collate", "--resident", "--seed=%d" % SEED] + list(extra))
    p.hidden_audio = p.hidden_text = p.hidden_visual = 8            # D = 24
    p.hidden_all = D
    return p


def _dialogues(p, lengths, seed=11):
    from erc_amd.synthetic import make_dialogues
    return [make_dialogues(1, p.dims(), n_speakers=p.n_speakers, n_classes=p.n_classes, min_len=n, max_len=n, seed=seed * 100 + i)[0]
            for i, n in enumerate(lengths)]


def _dress(model):
    """a wider logit spread (fewer near-ties among an untrained model's logits): out_mlp.5.weight = 8 * randn with zero row
    mean, its bias 0.1 * randn, from a CPU generator: the same on the oracle and on the device"""
    g = torch.Generator().manual_seed(77)
    lin = model.out_mlp[5]
    W = 8.0 * torch.randn(lin.weight.shape, generator=g)
    W -= W.mean(1, keepdim=True)
    b = 0.1 * torch.randn(lin.bias.shape, generator=g)
    with torch.no_grad():
        lin.weight.copy_(W.to(lin.weight.device))
        lin.bias.copy_(b.to(lin.bias.device))


def _trainer(device=DEV, dropout=0.0):
    from erc_amd.dagerc import DAGERCTrainer
    p = _params(["--dropout=%g" % dropout])
    tr = DAGERCTrainer(p, device)
    _dress(tr.model)
    return tr, p


def _store(p, dialogues, device=DEV):
    from erc_amd.datasets import DeviceDialogueStore
    return DeviceDialogueStore(dialogues, p, torch.device(device), torch.float32)


@functools.lru_cache(maxsize=None)
def _min_gap():
    """the oracle (CPU, the trainer's initial parameters) on the test dialogues, batch by batch as the test loop visits them:
    the smallest difference between the two largest logits of an utterance"""
    from erc_amd.trainer import StoreLoader
    from oracle.dagerc import DAGERCOracle
    tr, p = _trainer("cpu")
    ref = DAGERCOracle(emb_dim=D, dropout=0.0, n_classes=p.n_classes, gnn_layers=L).eval()
    ref.load_state_dict(tr.model.state_dict())
    store = _store(p, _dialogues(p, TEST_LENGTHS), "cpu")
    gap = float("inf")
    torch.set_num_threads(8)
    with torch.no_grad():
        for batch in StoreLoader(store, 4, False, 0):
            logits = ref(**batch)[0][batch["attention_mask"].bool()]
            top = logits.double().topk(2, dim=-1).values
            gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
    return gap


def _host_cm(tr, store, C):
    """the default test loop of trainer.run on this trainer: its confusion matrix (true x predicted)"""
    from erc_amd.trainer import StoreLoader, test_epoch_loader
    tr.model.eval()
    true, pred, _, _ = test_epoch_loader(tr, StoreLoader(store, 4, False, 0), False)
    cm = torch.zeros(C, C, dtype=torch.int64)
    for t, q in zip(true, pred):
        cm[t, q] += 1
    return cm


def test_resident_eval_epoch_equals_the_default_test_loop_exactly():
    from erc_amd.trainer import ResidentEval
    gap = _min_gap()
    print("oracle's smallest top-2 logit gap over the %d test utterances: %.3e" % (sum(TEST_LENGTHS), gap))
    assert gap > GAP                                        # precondition: no argmax can flip within the logit tolerance
    tr, p = _trainer()
    store = _store(p, _dialogues(p, TEST_LENGTHS))
    C, n_all = p.n_classes, sum(TEST_LENGTHS)
    want = _host_cm(tr, store, C)
    assert int(want.sum()) == n_all
    ev = ResidentEval(tr, store, 4)
    assert ev.supported() and ev.T == 13 and ev.caps == [52] * 3 and ev.counts == [21, 52, 21]
    cm1 = ev.epoch()
    assert int(cm1.sum()) == n_all                          # no utterance left out
    assert torch.equal(cm1, want)
    assert (ev.eager, ev.captures, ev.replays) == (1, 1, 2)
    for k in (2, 3):                                        # replays only, the same matrix
        assert torch.equal(ev.epoch(), want)
        assert (ev.eager, ev.captures, ev.replays) == (1, 1, 2 + 3 * (k - 1))
    tr.model.check_cluster()


def test_eval_scores_takes_a_capacity_sized_static_batch():
    """the bucket layout of DAGERCTrainer.capacity_bucket (more slots than dialogues, a longer T, label [N_cap]); neither
    ``dynamic_n`` nor ``eval()`` is set by the caller, and the step runs in a workspace of its own"""
    from tests.util_cases import make_batch_lengths
    tr, p = _trainer(dropout=0.3)
    b = tr.prepare_batch(make_batch_lengths([9, 1, 12], p.dims(), n_speakers=2, n_classes=6, seed=4, speaker_onehot=True))
    n = int(b["label"].shape[0])
    tr.t_cap = 13
    key, make, fill = tr.capacity_bucket(b)
    assert key == ("capacity", 4, 13, 52)
    static = make()
    fill(static, b)
    static["label"][n:] = 5
    tr.model.train()
    tr.train_step(b)                                        # a training workspace exists and is the last one
    last, rng = tr.model._last_ws, tr.optim.state.clone()
    cm = torch.zeros(6, 6, dtype=torch.int64, device=DEV)
    ws = tr.model.eval_scores(static, cm)
    assert ws is not last and tr.model._last_ws is last and torch.equal(tr.optim.state, rng) and tr.model.training
    assert not tr.model.dynamic_n and "dHall" not in ws
    tr.model.eval()
    want = tr.to_logits(b)[b["attention_mask"].bool()].cpu()
    got = ws["logits"][ws["node_row"][:n].long()].cpu()
    assert float((got - want).abs().max()) < 1e-4          # eval mode: no dropout although the module was in train()
    assert int(cm.sum()) == n
    assert torch.equal(cm.cpu(), torch.from_numpy(_cm_numpy(got.numpy(), np.arange(n), b["label"].cpu().numpy(), n, 6)))


def test_test_epochs_leave_the_training_state_untouched():
    """three resident training epochs (dropout on) with a test epoch after each, and three without: parameters, Adam moments,
    the optimizer's step count and RNG offset, the health word and the running loss sums are bit-identical"""
    from erc_amd.trainer import ResidentEpochs, ResidentEval
    states = []
    for with_eval in (True, False):
        tr, p = _trainer(dropout=0.2)
        train = _store(p, _dialogues(p, TRAIN_LENGTHS, seed=21))
        test = _store(p, _dialogues(p, TEST_LENGTHS[:9]))
        res = ResidentEpochs(tr, train, 4, seed=3)
        assert res.supported()
        ev = ResidentEval(tr, test, 4)
        cms = []
        for epoch in range(3):
            tr.model.train()
            assert res.epoch() == (sum(TRAIN_LENGTHS), 2)
            if with_eval:
                tr.model.eval()
                before = [t.clone() for t in (tr.model.flat.data, tr.model.flat.exp_avg, tr.model.flat.exp_avg_sq, tr.optim.state,
                                              tr.model.flat.grad_full)]
                cms.append(ev.epoch())
                after = (tr.model.flat.data, tr.model.flat.exp_avg, tr.model.flat.exp_avg_sq, tr.optim.state, tr.model.flat.grad_full)
                assert all(torch.equal(a, b) for a, b in zip(before, after))      # (grad_full ends in the health word)
        torch.cuda.synchronize()
        if with_eval:
            assert all(int(c.sum()) == sum(TEST_LENGTHS[:9]) for c in cms) and ev.captures == 1
        fl = tr.model.flat
        states.append(dict(data=fl.data.clone(), exp_avg=fl.exp_avg.clone(), exp_avg_sq=fl.exp_avg_sq.clone(),
                           state=tr.optim.state.clone(), health=fl.health.clone(), acc=res.acc.clone()))
        tr.model.check_cluster()
    a, b = states
    assert int(a["state"][0]) == 6 and int(a["state"][1]) > 0 and int(a["health"][0]) == 0
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_train_mm_cli_resident_eval():
    """``train_mm.py --module=dagerc --device_collate --resident --resident_eval``, two epochs on short synthetic dialogues,
    as a child process: every epoch line carries all seven metrics and ``test_s``, and the metrics equal those of the same run
    without ``--resident_eval`` (the host loop over the same parameters)"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = ["--module=dagerc", "--dataset=iemocap-cogmen-6", "--modality=a", "--epoch=2", "--n_train=10", "--n_test=6",
            "--train.batch_size=4", "--test.batch_size=4", "--syn_min_len=2", "--syn_max_len=12", "--gnn_layers=2",
            "--device_collate", "--resident"]
    runs = {}
    for tag, extra in (("device", ["--resident_eval"]), ("host", [])):
        res = subprocess.run([sys.executable, "train_mm.py"] + args + extra, cwd=repo, capture_output=True, text=True, timeout=240)
        assert res.returncode == 0, res.stderr[-2000:]
        runs[tag] = [l for l in (json.loads(s) for s in res.stdout.splitlines() if s.startswith("{")) if "test" in l]
        assert len(runs[tag]) == 2
    for e, (d, h) in enumerate(zip(runs["device"], runs["host"])):
        assert set(d["test"]) == {"acc", "wa", "pre", "rec", "f1", "mif1", "maf1"} == set(h["test"])
        assert d["test_s"] > 0 and "test_s" not in h
        assert d["graphs_captured"] == h["graphs_captured"] == 1 and d["graph_replays"] == h["graph_replays"] == 3 * (e + 1) - 1
        print("epoch %d: test %s (device) %s (host), test_s %.4f" % (e, d["test"], h["test"], d["test_s"]))
        for k in d["test"]:
            assert abs(d["test"][k] - h["test"][k]) < 1e-9, (e, k, d["test"], h["test"])
