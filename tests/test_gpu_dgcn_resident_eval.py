"""GPU: ``--module=dgcn --resident --resident_eval`` -- the evaluation tail (csrc/dgcn_tail_eval.hip, erc_dgcn_tail_eval)
through the C-ABI against a float64 evaluation of its five formulas, DialogueGCN's forward-only step under
``trainer.ResidentEval`` against the default test loop of ``trainer.run`` (``store.batch`` -> ``to_logits`` -> host argmax:
the reference here), a capacity-sized static batch, graph replay, the training state, and the command line."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util_cases import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 256                     # capacity of the launches: 16 workgroups of 16 rows
GAP = 1e-3                    # rows compared with float64's argmax: float64 top-two logit gap at least this
TOL = 2e-5                    # logits, relative (rel_err): the fused tail's bound against separate kernels (test_gpu_dgcn.py)
NS = (0, 1, 15, 16, 17, 33, 250, 256)      # no row, one row, around a tile (= workgroup) edge, many workgroups, full capacity
# dialogue lengths, 256 utterances: the first tile (rows 0 .. 15) holds dialogues 0, 1 and the start of 2; dialogue 2 (rows
# 3 .. 42) lies in the tiles 0, 1 and 2; the last dialogue (42 utterances) is longer than a tile plus both windows
DLG = (1, 2, 40, 5, 13, 7, 3, 30, 9, 21, 16, 11, 4, 25, 8, 19, 42)
assert sum(DLG) == CAP


# ------------------------------------------------------------------------------------------------- the tail kernel alone
def _adjacency(n, wp, wf):
    """dense in-adjacency of the first n utterances of DLG: A[i, j] = 1 when j -> i, i.e. j in i's dialogue and
    i - wp <= j <= i + wf (the window graph, its own row included); both below n"""
    dlg = np.repeat(np.arange(len(DLG)), DLG)
    i, j = np.arange(CAP)[:, None], np.arange(CAP)[None, :]
    return ((dlg[:, None] == dlg[None, :]) & (j >= i - wp) & (j <= i + wf) & (i < n) & (j < n)).astype(np.float64)


def _csr(A):
    """in-CSR over CAP rows of a dense adjacency: (in_ptr int32 [CAP + 1], in_src int32 [>= 1]); empty rows stay empty"""
    ptr = np.zeros(CAP + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(A.sum(1).astype(np.int64))
    src = np.nonzero(A)[1].astype(np.int32)
    return torch.from_numpy(ptr), torch.from_numpy(src if src.size else np.zeros(1, dtype=np.int32))


def _tail_f64(case, A):
    """the five formulas of erc_dgcn_tail_eval in float64 with the dense adjacency: (logits, first index of the maximum)"""
    d = lambda k: case[k].double()
    Hc = d("slabs").sum(0) + d("rgcn_bias")
    agg = torch.from_numpy(A) @ Hc
    gout = agg @ d("W_rel").T + d("b_rel") + Hc @ d("W_root").T
    z = torch.relu(torch.cat([d("X"), gout], 1) @ d("W1").T + d("b1"))
    logits = z @ d("W2").T + d("b2")
    return logits, logits.argmax(-1)


WINDOWS = ((10, 10), (2, 4), (0, 0))


def _draw_case(C, n_slabs, tie, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    case = dict(C=C, n_slabs=n_slabs, slabs=rnd(n_slabs, CAP, 100) / n_slabs ** 0.5, rgcn_bias=0.1 * rnd(100), X=rnd(CAP, 200),
                W_rel=rnd(100, 100) / 30.0, b_rel=0.1 * rnd(100), W_root=rnd(100, 100) / 10.0, W1=rnd(100, 300) / 300 ** 0.5,
                b1=0.1 * rnd(100), W2=rnd(C, 100) / 2.0, b2=0.1 * rnd(C), labels=torch.randint(0, C, (CAP, ), generator=g))
    case["W2"] -= case["W2"].mean(1, keepdim=True)      # (Zc >= 0: rows with a common offset would let one class win every row)
    if tie:
        case["W2"][1], case["b2"][1] = case["W2"][0], case["b2"][0]
    return case


def _enough_clear_rows(case):
    """the float64 top-two gap is at least GAP on 98 % of the rows, for every window and every n the tests use (a property of
    the drawn inputs and the float64 formulas alone)"""
    for window in WINDOWS:
        for n in NS[1:]:
            top = _tail_f64(case, _adjacency(n, *window))[0][:n].topk(2, dim=-1).values
            if int(((top[:, 0] - top[:, 1]) >= GAP).sum()) < 0.98 * n:
                return False
    return True


@functools.lru_cache(maxsize=None)
def _tail_case(C, n_slabs, tie=False):
    """Parameters and CAP rows of inputs, drawn once per (C, n_slabs) on the CPU and never changed: the first seed whose
    float64 logits leave at most 2 % of the rows within GAP of a tie (with n = 1 .. 17 that is: none of the first rows).
    ``tie``: classes 0 and 1 share their W2 row and bias (no gap condition: the test compares with the kernel's own logits)."""
    base = 2000 + 100 * C + 10 * n_slabs + (5000 if tie else 0)
    for seed in range(base, base + 10):
        case = _draw_case(C, n_slabs, tie, seed)
        if tie or _enough_clear_rows(case):
            return case
    raise AssertionError("no seed in [%d, %d) draws a case with 98 %% of its rows clear of a tie" % (base, base + 10))


@functools.lru_cache(maxsize=None)
def _reference(C, n_slabs, window, n, tie=False):
    """float64 (logits, predictions, in_ptr, in_src) of the first n rows under the window (wp, wf)"""
    A = _adjacency(n, *window)
    return _tail_f64(_tail_case(C, n_slabs, tie), A) + _csr(A)


def _cm_of(true, pred, C):
    cm = torch.zeros(C, C, dtype=torch.int64)
    cm.index_put_((true, pred), torch.ones_like(true), accumulate=True)
    return cm


@functools.lru_cache(maxsize=None)
def _device_case(C, n_slabs, tie=False):
    case = _tail_case(C, n_slabs, tie)
    return {k: v.to(DEV).contiguous() for k, v in case.items() if torch.is_tensor(v) and k not in ("slabs", "X", "labels")}


def _launch(C, n_slabs, window, n, cm, use_n_dev=True, label_rows=False, logits=None, tie=False, n_classes=None, win=None):
    """one erc_dgcn_tail_eval launch on the first n rows of the case: rows [n, CAP) hold NaN in the slabs and in Xc, their
    labels are 99 and their CSR ranges empty.  Returns Xc before and after (the graph_out columns hold a sentinel)."""
    from erc_amd import capi
    case, W = _tail_case(C, n_slabs, tie), _device_case(C, n_slabs, tie)
    _, _, in_ptr, in_src = _reference(C, n_slabs, window, n, tie)
    slabs = torch.full((n_slabs, CAP, 100), float("nan"))
    slabs[:, :n] = case["slabs"][:, :n]
    Xc = torch.full((CAP, 300), float("nan"))
    Xc[:n, :200] = case["X"][:n]
    Xc[:, 200:] = 555.0
    labels = torch.full((CAP, ), 99, dtype=torch.int64)
    labels[:n] = case["labels"][:n]
    rows = None
    if label_rows:      # a permutation into a longer label array (a resident store's labels); the other entries are out of range
        perm = torch.randperm(400, generator=torch.Generator().manual_seed(n))[:CAP]
        long = torch.full((400, ), -5, dtype=torch.int64)
        long[perm] = labels
        labels, rows = long, perm.to(torch.int32).to(DEV)
    n_dev = torch.tensor([n, 12345], dtype=torch.int32, device=DEV) if use_n_dev else None
    Xd = Xc.to(DEV)
    g = dict(in_ptr=in_ptr.to(DEV), in_src=in_src.to(DEV))
    capi.dgcn_tail_eval(slabs.to(DEV), n_slabs, CAP * 100, W["rgcn_bias"], g, max(window) if win is None else win, W["W_rel"],
                        W["b_rel"], W["W_root"], W["W1"], W["b1"], W["W2"], W["b2"], labels.to(DEV), n_classes or C,
                        CAP if use_n_dev else n, Xd, 300, cm, logits=logits, n_dev=n_dev, label_rows=rows)
    torch.cuda.synchronize()
    return Xc, Xd.cpu()


def _check_case(C, n_slabs, window):
    case = _tail_case(C, n_slabs)
    for n in NS:
        ref_logits, ref_pred, _, _ = _reference(C, n_slabs, window, n)
        true = case["labels"][:n]
        top = ref_logits[:n].topk(2, dim=-1).values
        keep = (top[:, 0] - top[:, 1]) >= GAP
        assert int(keep.sum()) >= 0.98 * n, (C, n, int(keep.sum()))
        want_kept = _cm_of(true[keep], ref_pred[:n][keep], C)
        first = None
        for use_n_dev in (True, False):
            for label_rows in (False, True):
                cm = torch.zeros(C, C, dtype=torch.int64, device=DEV)
                logits = torch.full((CAP, C), -7777.0, device=DEV)
                x_before, x_after = _launch(C, n_slabs, window, n, cm, use_n_dev, label_rows, logits)
                tag = (C, n_slabs, window, n, use_n_dev, label_rows)
                got, cm = logits.cpu(), cm.cpu()
                err = rel_err(got[:n], ref_logits[:n]) if n else 0.0
                print("dgcn_tail_eval C=%d slabs=%d window=%s n=%d n_dev=%s label_rows=%s rel err %.3e, %d rows under the gap"
                      % (tag + (err, n - int(keep.sum()))))
                assert err < TOL, tag
                assert bool((got[n:] == -7777.0).all()), tag                              # nothing written beyond the count
                assert torch.equal(x_before.view(torch.int32), x_after.view(torch.int32)), tag      # Xc is read-only
                assert int(cm.sum()) == n, (tag, cm)
                assert torch.equal(cm, _cm_of(true, got[:n].argmax(-1), C)), tag          # the first maxima of its own logits
                assert torch.equal(_cm_of(true[keep], got[:n].argmax(-1)[keep], C), want_kept), tag
                first = cm if first is None else first
                assert torch.equal(cm, first), tag                                       # the four ways count alike
        # a second launch adds; a launch with no rows changes nothing
        cm = torch.full((C, C), 3, dtype=torch.int64, device=DEV)
        _launch(C, n_slabs, window, n, cm)
        _launch(C, n_slabs, window, n, cm, label_rows=True)
        assert torch.equal(cm.cpu(), 2 * first + 3), (C, n)
        _launch(C, n_slabs, window, 0, cm)
        assert torch.equal(cm.cpu(), 2 * first + 3), (C, n)


def _many_slabs():
    from erc_amd import capi
    return capi.brgcn_fwd_tile_slabs()


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("many", [False, True], ids=["1-slab", "tile-slabs"])
@pytest.mark.parametrize("C", [4, 6, 7])
def test_tail_eval_counts_equal_the_float64_confusion_matrix(C, many, window):
    """erc_dgcn_tail_eval alone, 256 rows in 17 dialogues (a tile that spans three dialogues, a dialogue that spans three
    tiles), for every n of NS, with the count on the device and with n_dev = NULL, with and without label_rows: the logits
    of the counted rows are within 2e-5 (relative) of float64, nothing is written past n, cm sums to n and IS the matrix
    of the first maxima of the kernel's own logits; on the rows whose float64 top-two gap is at least 1e-3 (at least 98 % of
    n) it equals the float64 matrix.  A second launch adds to cm, n = 0 leaves it untouched.  Rows [n, 256) hold NaN in the
    slabs and in Xc and labels of 99: reading any of them would show in the logits or in the counts."""
    _check_case(C, _many_slabs() if many else 1, window)


def test_tail_eval_sums_more_slabs_than_one_pass_holds():
    """nine partial outputs: the first eight are requested at once, the ninth is added by the loop behind them"""
    _check_case(6, 9, (2, 4))


def test_tail_eval_on_poisoned_lds(monkeypatch):
    """every CU's LDS holds NaN when the kernel starts: a tail that reads LDS it never wrote (K padding of the A tiles, the
    window rows outside the batch, rows of a partial tile) fails the same assertions"""
    from tests.util_cases import poison_lds_before
    poison_lds_before(monkeypatch, "dgcn_tail_eval")
    _check_case(6, _many_slabs(), (2, 4))
    _check_case(7, 1, (10, 10))


def test_tail_eval_scores_equal_logits_as_the_lower_index():
    """classes 0 and 1 with identical W2 rows and biases: torch.argmax returns the first index of the maximum, so nothing is
    ever predicted as class 1"""
    C, window = 6, (10, 10)
    case = _tail_case(C, 1, tie=True)
    for n in (17, 256):
        _, ref_pred, _, _ = _reference(C, 1, window, n, True)
        assert int((ref_pred[:n] == 1).sum()) == 0 and int((ref_pred[:n] == 0).sum()) >= 3
        cm = torch.zeros(C, C, dtype=torch.int64, device=DEV)
        logits = torch.zeros(CAP, C, device=DEV)
        _launch(C, 1, window, n, cm, logits=logits, tie=True)
        assert torch.equal(logits[:n, 0], logits[:n, 1])
        assert int(cm[:, 1].sum()) == 0 and int(cm[:, 0].sum()) >= 3
        assert torch.equal(cm.cpu(), _cm_of(case["labels"][:n], logits[:n].argmax(-1).cpu(), C))


def test_tail_eval_refuses_what_it_cannot_run():
    from erc_amd import capi
    with pytest.raises(capi.ErcGraftError, match="n_classes=9"):
        _launch(4, 1, (10, 10), 16, torch.zeros(9, 9, dtype=torch.int64, device=DEV), n_classes=9)
    with pytest.raises(capi.ErcGraftError, match="int64"):
        _launch(4, 1, (10, 10), 16, torch.zeros(4, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(capi.ErcGraftError, match="window 11"):
        _launch(4, 1, (10, 10), 16, torch.zeros(4, 4, dtype=torch.int64, device=DEV), win=11)
    with pytest.raises(capi.ErcGraftError, match="null pointer"):
        capi._call("erc_dgcn_tail_eval", None, 1, 0, None, None, None, 10, None, None, None, None, None, None, None, None, None, 4,
                   16, None, None, 300, torch.zeros(4, 4, dtype=torch.int64, device=DEV), None)


# ------------------------------------------------------------------------------------------------------- the whole path
LENGTHS = (1, 2, 23, 5, 23, 23, 23, 23, 7, 11, 16, 3, 19, 13, 9)      # B = 4: 4 steps, the second fills its bucket (4 x 23 = B * T),
CONFIGS = [("meld-mmgcn-7", "bf16"), ("iemocap-cogmen-6", "f32")]     # the last has 3 dialogues; 201 utterances


def _params(dataset, compute, extra=()):
    from erc_amd.params import ERCParams
    return ERCParams().from_args(["--dataset=" + dataset, "--loss_weights=False", "--compute=" + compute, "--train.batch_size=4",
                                  "--test.batch_size=4", "--device_collate", "--seed=5"] + list(extra))


def _dialogues(p, lengths=LENGTHS, seed=11):
    from erc_amd.synthetic import make_dialogues
    return [make_dialogues(1, p.dims(), n_speakers=p.n_speakers, n_classes=p.n_classes, min_len=L, max_len=L, seed=seed * 100 + i)[0]
            for i, L in enumerate(lengths)]


def _dress(model):
    """a wider logit spread (fewer near-ties among the untrained model's logits): clf.lin2.weight = 8 * randn with zero row
    mean, clf.lin2.bias = 0.1 * randn, from a CPU generator: the same on the oracle and on the device"""
    g = torch.Generator().manual_seed(77)
    C = model.clf.lin2.weight.shape[0]
    W = 8.0 * torch.randn(C, 100, generator=g)
    W -= W.mean(1, keepdim=True)
    b = 0.1 * torch.randn(C, generator=g)
    with torch.no_grad():
        model.clf.lin2.weight.copy_(W.to(model.clf.lin2.weight.device))
        model.clf.lin2.bias.copy_(b.to(model.clf.lin2.bias.device))


def _trainer(dataset, compute, device=DEV):
    from erc_amd.dgcn import DGCNTrainer
    p = _params(dataset, compute)
    tr = DGCNTrainer(p, device)
    tr.model.relation_space = False      # (two speakers default to relation space, which has no capacity mode)
    _dress(tr.model)
    return tr, p


def _store(p, dialogues, device=DEV):
    from erc_amd.datasets import DeviceDialogueStore
    return DeviceDialogueStore(dialogues, p, torch.device(device), torch.bfloat16 if p.compute == "bf16" else torch.float32)


def _default_test_loop(tr, store, B):
    """the test loop of trainer.run on this trainer: (logits [n, C], labels [n]) on the host"""
    from erc_amd.trainer import StoreLoader
    tr.model.eval()
    logits, true = [], []
    for batch in StoreLoader(store, B, False, 0):
        logits.append(tr.to_logits(tr.prepare_batch(batch)).float().cpu().clone())
        true.append(batch["label"].cpu())
    return torch.cat(logits), torch.cat(true)


@pytest.mark.parametrize("dataset,compute", CONFIGS)
def test_resident_eval_epoch_equals_the_default_test_loop(dataset, compute):
    """ResidentEval.epoch() against the default test loop on the same trainer state, B = 4, dialogues of 1 .. 23 utterances
    (one batch fills its bucket exactly, the last has an empty slot).  Every utterance is counted; the per-row logits of the
    eval step are within 2e-5 (relative) of the eager ones; the confusion matrices are equal once the rows whose REFERENCE
    top-two gap is under 1e-3 are taken out of both, and those are at most 2 % of the rows.  Share measured with
    oracle/dgcn.py in float64 on the CPU for these seeds (trainer seed 5, dialogue seed 11, lin2 seed 77): 0 of 201 rows
    under the gap for meld-mmgcn-7 (smallest gap 8.9e-3; features rounded to bf16: 0 of 201, 1.05e-2) and 1 of 201 for
    iemocap-cogmen-6 (smallest gap 4.8e-4, the next 2.3e-3), every class predicted in both.  Epochs two and three replay the bucket's graph
    and return the same matrix, bit for bit."""
    from erc_amd.trainer import ResidentEval
    tr, p = _trainer(dataset, compute)
    store = _store(p, _dialogues(p))
    C, n_all = p.n_classes, sum(LENGTHS)
    ref_logits, true = _default_test_loop(tr, store, 4)
    assert ref_logits.shape == (n_all, C)
    ev = ResidentEval(tr, store, 4)
    assert ev.supported() and ev.T == 23 and ev.caps == [92] * 4 and ev.counts[1] == 92
    cm1 = ev.epoch()
    assert int(cm1.sum()) == n_all
    assert (ev.eager, ev.captures, ev.replays) == (1, 1, 3)
    # per-row scores of the forward-only step: each step once more, eagerly, on the epoch's own table
    rows, cm_rows = [], torch.zeros(C, C, dtype=torch.int64, device=DEV)
    for s in range(ev.steps):
        ev.cur_desc.copy_(ev.table_dev[s])
        ws = tr.resident_eval_step(tr.resident_eval_batch(store, ev.cur_desc, 4, ev.T, ev.caps[s]), cm_rows)
        rows.append(ws["logits"][:ev.counts[s]].cpu().clone())
    got_logits = torch.cat(rows)
    assert torch.equal(cm_rows.cpu(), cm1)                          # the same launches, counted the same
    assert torch.equal(_cm_of(true, got_logits.argmax(-1), C), cm1)      # and cm IS the matrix of these rows' first maxima
    err = rel_err(got_logits, ref_logits)
    top = ref_logits.double().topk(2, dim=-1).values
    keep = (top[:, 0] - top[:, 1]) >= GAP
    out = n_all - int(keep.sum())
    print("dgcn resident eval %s %s: rel err vs the eager loop %.3e, %d of %d rows within %g of a tie, min gap %.3e, classes "
          "predicted %s" % (dataset, compute, err, out, n_all, GAP, float((top[:, 0] - top[:, 1]).min()),
                            sorted(set(ref_logits.argmax(-1).tolist()))))
    assert out <= 0.02 * n_all
    assert torch.equal(_cm_of(true[keep], got_logits.argmax(-1)[keep], C), _cm_of(true[keep], ref_logits.argmax(-1)[keep], C))
    assert err < TOL
    # replay: no new capture, the same matrix
    for k in (2, 3):
        cm_k = ev.epoch()
        assert ev.captures == 1 and ev.eager == 1 and ev.replays == 3 + 4 * (k - 1)
        assert torch.equal(cm_k, cm1)


def test_eval_scores_takes_a_capacity_sized_static_batch():
    """the same step on a padded static batch (more dialogue slots than dialogues, a longer T, a label buffer of N_cap > N
    entries filled with 99 past N: the bucket layout of DGCNTrainer.capacity_bucket) counts exactly the batch's utterances
    and scores them like the exact-shape eager forward; neither ``dynamic_n`` nor ``eval()`` is set by the caller"""
    tr, p = _trainer("meld-mmgcn-7", "bf16")
    from tests.util_cases import make_batch_lengths
    b = tr.prepare_batch(make_batch_lengths([9, 1, 14], p.dims(), n_speakers=p.n_speakers, n_classes=p.n_classes, seed=4))
    n = int(b["label"].shape[0])
    tr.t_cap = 20
    key, make, fill = tr.capacity_bucket(b)
    assert key == ("capacity", 4, 20, 80)                           # min(128, B_cap * T_cap)
    static = make()
    static["label"].fill_(99)
    fill(static, b)
    tr.model.train()
    assert not tr.model.dynamic_n
    rng = tr.optim.state.clone()
    cm = torch.zeros(7, 7, dtype=torch.int64, device=DEV)
    ws = tr.model.eval_scores(static, cm)
    assert ws is not tr.model._last_ws and torch.equal(tr.optim.state, rng) and tr.model.training
    got = ws["logits"][:n].cpu().clone()
    tr.model.eval()
    want = tr.to_logits(b).float().cpu()
    assert int(cm.sum()) == n
    print("dgcn eval_scores on a static bucket: rel err %.3e" % rel_err(got, want))
    assert rel_err(got, want) < TOL
    assert torch.equal(cm.cpu(), _cm_of(b["label"].cpu(), got.argmax(-1), 7))


@pytest.mark.parametrize("dataset,compute", CONFIGS)
def test_test_epochs_leave_the_training_state_untouched(dataset, compute):
    """six resident training steps (dropout on) with a test epoch after each pair, and six without: parameters, Adam
    moments, the optimizer's step count and RNG offset and the running loss sums are bit-identical"""
    from erc_amd.trainer import ResidentEpochs, ResidentEval
    states = []
    for with_eval in (True, False):
        tr, p = _trainer(dataset, compute)
        train = _store(p, _dialogues(p, (12, 3, 20, 7, 15, 9, 2, 18), seed=21))
        test = _store(p, _dialogues(p, LENGTHS[:9]))
        res = ResidentEpochs(tr, train, 4, seed=3)
        assert res.supported()
        ev = ResidentEval(tr, test, 4)
        cms = []
        for epoch in range(3):
            tr.model.train()
            assert res.epoch() == (86, 2)
            if with_eval:
                tr.model.eval()
                cms.append(ev.epoch())
        torch.cuda.synchronize()
        if with_eval:
            assert all(int(c.sum()) == sum(LENGTHS[:9]) for c in cms) and ev.captures == 1
        fl = tr.model.flat
        states.append(dict(data=fl.data.clone(), exp_avg=fl.exp_avg.clone(), exp_avg_sq=fl.exp_avg_sq.clone(),
                           state=tr.optim.state.clone(), acc=res.acc.clone()))
    a, b = states
    assert int(a["state"][0]) == 6 and int(a["state"][1]) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_train_mm_cli_resident_eval():
    """``train_mm.py --module=dgcn --dataset=meld-mmgcn-7 --loss_weights=False --compute=bf16 --device_collate --resident
    --resident_eval``, two epochs on synthetic data, as a child process: every epoch line carries ``test`` with all seven
    metrics and ``test_s``; ``acc`` equals the same run's without the flag to within 2 % of the test utterances (a logit pair
    closer than the two paths' rounding may flip its argmax); the training side replays the same number of graphs."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = ["--module=dgcn", "--dataset=meld-mmgcn-7", "--loss_weights=False", "--epoch=2", "--n_train=20", "--n_test=6",
            "--train.batch_size=8", "--test.batch_size=4", "--compute=bf16", "--device_collate", "--resident"]
    runs = {}
    for tag, extra in (("device", ["--resident_eval"]), ("host", [])):
        res = subprocess.run([sys.executable, "train_mm.py"] + args + extra, cwd=repo, capture_output=True, text=True, timeout=240)
        assert res.returncode == 0, res.stderr[-2000:]
        runs[tag] = [l for l in (json.loads(s) for s in res.stdout.splitlines() if s.startswith("{")) if "test" in l]
        assert len(runs[tag]) == 2
    for e, (d, h) in enumerate(zip(runs["device"], runs["host"])):
        assert set(d["test"]) == {"acc", "wa", "pre", "rec", "f1", "mif1", "maf1"} == set(h["test"])
        assert d["test_s"] > 0 and "test_s" not in h
        assert d["train_utt_per_s"] > 0 and d["graph_replays"] == h["graph_replays"]
        print("epoch %d: acc %.6f (device) %.6f (host), test_s %.4f" % (e, d["test"]["acc"], h["test"]["acc"], d["test_s"]))
        assert abs(d["test"]["acc"] - h["test"]["acc"]) <= 0.02, (e, d["test"], h["test"])
        assert d["test"]["mif1"] == d["test"]["acc"]
