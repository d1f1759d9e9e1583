"""GPU: ``--resident_eval`` -- the evaluation head (csrc/head.hip, erc_head_eval) through the C-ABI against a float64
evaluation of its three formulas, COGMEN's forward-only step under ``trainer.ResidentEval`` against the default test loop of
``trainer.run`` (``store.batch`` -> ``to_logits`` -> host argmax: the reference here), graph replay, the training state, and
the command line."""
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
F = 100
CAP = 256                     # capacity of the head launches: 16 workgroups of 16 rows
GAP = 1e-3                    # rows kept: float64 top-two logit gap >= ten times the 1e-4 logit bound
NS = (0, 1, 15, 16, 17, 33, 250, 256)      # no row, one row, around a tile (= workgroup) edge, many workgroups, full capacity


# ------------------------------------------------------------------------------------------------- the head kernel alone
def _head_f64(H2, P):
    """the three formulas of erc_head_eval in float64: (logits, first index of the maximum)"""
    d = lambda k: P[k].double()
    y = (H2.double() - d("rm")) * d("gamma") / torch.sqrt(d("rv") + P["eps"]) + d("beta")
    h3 = torch.where(y > 0, y, 0.01 * y)
    z = torch.relu(h3 @ d("W0").T + d("b0"))
    logits = z @ d("W3").T + d("b3")
    return logits, logits.argmax(-1)


@functools.lru_cache(maxsize=None)
def _head_case(C, tie=False):
    """Parameters, a pool of CAP rows whose float64 top-two gap is at least GAP (drawn twice as many; rows are independent
    in eval mode) with labels, and their float64 logits / predictions.  Computed once per C, never changed.
    ``tie``: classes 0 and 1 share their W3 row and bias -- the gap is then taken with class 1 left out."""
    g = torch.Generator().manual_seed(1000 + C + (50 if tie else 0))
    rnd = lambda *s: torch.randn(*s, generator=g)
    P = dict(gamma=0.5 + torch.rand(F, generator=g), beta=0.3 * rnd(F), rm=0.2 * rnd(F), rv=0.5 + torch.rand(F, generator=g),
             W0=rnd(F, F) / F ** 0.5, b0=0.1 * rnd(F), W3=rnd(C, F) / 4.0, b3=0.1 * rnd(C), eps=1e-5)
    P["W3"] -= P["W3"].mean(1, keepdim=True)      # (Z >= 0: rows with a common offset would let one class win every row)
    if tie:
        P["W3"][1], P["b3"][1] = P["W3"][0], P["b3"][0]
    H2 = 1.5 * rnd(2 * CAP, F)
    logits, pred = _head_f64(H2, P)
    lg = torch.cat([logits[:, :1], logits[:, 2:]], 1) if tie else logits
    top = lg.topk(2, dim=-1).values
    keep = (top[:, 0] - top[:, 1]) >= GAP
    assert int(keep.sum()) >= CAP, "fewer than half of the drawn rows have a top-two gap of %g: %d of %d" % (GAP, int(keep.sum()), 2 * CAP)
    H2, logits, pred = H2[keep][:CAP].contiguous(), logits[keep][:CAP], pred[keep][:CAP]
    labels = torch.randint(0, C, (CAP, ), generator=g)
    return dict(P=P, H2=H2, logits=logits, pred=pred, labels=labels, C=C)


def _cm_of(true, pred, C):
    cm = torch.zeros(C, C, dtype=torch.int64)
    cm.index_put_((true, pred), torch.ones_like(true), accumulate=True)
    return cm


def _launch(case, n, cm, use_n_dev=True, label_rows=False, logits=None):
    """one erc_head_eval launch on the first n rows of the case: rows [n, CAP) of H2 are NaN and their labels out of range"""
    from erc_amd import capi
    P, C = case["P"], case["C"]
    dev = lambda t: t.to(DEV).contiguous()
    H2 = torch.full((CAP, F), float("nan"))
    H2[:n] = case["H2"][:n]
    labels = torch.full((CAP, ), 99, dtype=torch.int64)
    labels[:n] = case["labels"][:n]
    rows = None
    if label_rows:      # a permutation into a longer label array (a resident store's labels); the other entries are out of range
        perm = torch.randperm(400, generator=torch.Generator().manual_seed(n))[:CAP]
        long = torch.full((400, ), -5, dtype=torch.int64)
        long[perm] = labels
        labels, rows = long, dev(perm.to(torch.int32))
    n_dev = torch.tensor([n, 12345], dtype=torch.int32, device=DEV) if use_n_dev else None
    capi.head_eval(dev(H2), F, CAP if use_n_dev else n, F, C, dev(P["gamma"]), dev(P["beta"]), dev(P["rm"]), dev(P["rv"]), P["eps"], 0.01,
                   dev(P["W0"]), dev(P["b0"]), dev(P["W3"]), dev(P["b3"]), dev(labels), cm, logits=logits, n_dev=n_dev, label_rows=rows)
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [4, 6, 7])
def test_head_eval_counts_equal_the_float64_confusion_matrix(C):
    """erc_head_eval alone: for every n the logits of the counted rows are within 1e-4 (the project's fp32 parity bound) of
    float64, the confusion matrix EQUALS the float64 one, rows [n, 256) (NaN, labels out of range) are neither read nor
    counted -- with the count taken from the device, with n_dev = NULL, with and without label_rows -- a second launch adds
    to cm and n = 0 leaves it untouched."""
    case = _head_case(C)
    for n in NS:
        want = _cm_of(case["labels"][:n], case["pred"][:n], C)
        assert int(want.sum()) == n
        for use_n_dev in (True, False):
            if n == 0 and not use_n_dev:
                continue                       # (n_rows = 0 is no launch: the count 0 exists only on the device)
            for label_rows in (False, True):
                cm = torch.zeros(C, C, dtype=torch.int64, device=DEV)
                logits = torch.full((CAP, C), -7777.0, device=DEV)
                _launch(case, n, cm, use_n_dev, label_rows, logits)
                tag = (C, n, use_n_dev, label_rows)
                got = logits.cpu()
                err = float((got[:n].double() - case["logits"][:n]).abs().max()) if n else 0.0
                print("head_eval C=%d n=%d n_dev=%s label_rows=%s max|dlogit| %.3e" % (tag + (err, )))
                assert err < 1e-4, tag
                assert bool((got[n:] == -7777.0).all()), tag              # nothing written beyond the count
                assert int(cm.sum()) == n and torch.equal(cm.cpu(), want), (tag, cm.cpu(), want)
        # a second launch adds; a launch with no rows changes nothing
        cm = torch.full((C, C), 3, dtype=torch.int64, device=DEV)
        _launch(case, n, cm)
        _launch(case, n, cm, label_rows=True)
        assert torch.equal(cm.cpu(), 2 * want + 3), (C, n)
        _launch(case, 0, cm)
        assert torch.equal(cm.cpu(), 2 * want + 3), (C, n)


def test_head_eval_scores_equal_logits_as_the_lower_index():
    """classes 0 and 1 with identical W3 rows and biases: torch.argmax returns the first index of the maximum, so nothing is
    ever predicted as class 1"""
    case = _head_case(6, tie=True)
    assert int((case["pred"] == 1).sum()) == 0 and int((case["pred"][:17] == 0).sum()) >= 3
    for n in (17, 256):
        cm = torch.zeros(6, 6, dtype=torch.int64, device=DEV)
        logits = torch.zeros(CAP, 6, device=DEV)
        _launch(case, n, cm, logits=logits)
        assert torch.equal(logits[:n, 0], logits[:n, 1])
        assert int(cm[:, 1].sum()) == 0 and int(cm[:, 0].sum()) >= 3 and torch.equal(cm.cpu(), _cm_of(case["labels"][:n], case["pred"][:n], 6))


def test_head_eval_refuses_what_it_cannot_run():
    from erc_amd import capi
    case = _head_case(4)
    with pytest.raises(capi.ErcGraftError):
        capi.head_eval(None, F, CAP, F, 4, None, None, None, None, 1e-5, 0.01, None, None, None, None, None,
                       torch.zeros(4, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(capi.ErcGraftError):
        _launch(dict(case, C=9), 16, torch.zeros(9, 9, dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------------------- the whole path
LENGTHS = (1, 2, 23, 5, 23, 23, 23, 23, 7, 11, 16, 3, 19, 13, 9)      # B = 4: 4 steps, the second fills its bucket (4 x 23 = B * T),
W3_SCALE = 4.0                                                        # the last has 3 dialogues; 201 utterances


def _params(compute, extra=()):
    from erc_amd.params import ERCParams
    return ERCParams().from_args(["--dataset=iemocap-cogmen-6", "--compute=" + compute, "--train.batch_size=4",
                                  "--test.batch_size=4", "--device_collate", "--seed=5"] + list(extra))


def _dialogues(p, lengths=LENGTHS, seed=11):
    from erc_amd.synthetic import make_dialogues
    return [make_dialogues(1, p.dims(), n_speakers=p.n_speakers, n_classes=p.n_classes, min_len=L, max_len=L, seed=seed * 100 + i)[0]
            for i, L in enumerate(lengths)]


def _dress(model):
    """non-trivial BatchNorm affine / running statistics and a wider logit spread (cls.3.weight x W3_SCALE: fewer near-ties
    among the untrained model's logits), from a CPU generator: the same on the oracle and on the device"""
    g = torch.Generator().manual_seed(77)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(F, generator=g)
    with torch.no_grad():
        bn = model.gcn.bn
        for t, v in ((bn.weight, u(0.5, 1.5)), (bn.bias, u(-0.3, 0.3)), (bn.running_mean, u(-0.2, 0.2)), (bn.running_var, u(0.5, 1.5))):
            t.copy_(v.to(t.device))
        model.cls[3].weight.mul_(W3_SCALE)


def _trainer(compute):
    from erc_amd.cogmen import COGMENTrainer
    p = _params(compute)
    tr = COGMENTrainer(p, DEV)
    _dress(tr.model)
    tr.model.refresh_shadows()
    return tr, p


def _store(p, dialogues):
    from erc_amd.datasets import DeviceDialogueStore
    return DeviceDialogueStore(dialogues, p, torch.device(DEV), torch.bfloat16 if p.compute == "bf16" else torch.float32)


def _default_test_loop(tr, store, B):
    """the test loop of trainer.run on this trainer: (logits [n, C], labels [n]) on the host"""
    from erc_amd.trainer import StoreLoader
    tr.model.eval()
    logits, true = [], []
    for batch in StoreLoader(store, B, False, 0):
        logits.append(tr.to_logits(tr.prepare_batch(batch)).float().cpu().clone())
        true.append(batch["label"].cpu())
    return torch.cat(logits), torch.cat(true)


@pytest.mark.parametrize("compute", ["bf16", "f32x32"])
def test_resident_eval_epoch_equals_the_default_test_loop(compute):
    """ResidentEval.epoch() against the default test loop on the same trainer state, B = 4, dialogues of 1 .. 23 utterances
    (one batch fills its bucket exactly, the last has an empty slot).  Every utterance is counted; the confusion matrices are
    equal once the rows whose REFERENCE top-two gap is under 1e-3 are taken out of both, and those are at most 2 % of the rows.
    Share measured with oracle/cogmen.py on the CPU for this seed and W3_SCALE = 4: 0 of 201 rows, smallest gap 2.4e-3 (fp32
    features); 0 of 201, smallest gap 3.2e-3 (features rounded to bf16); with W3_SCALE = 1 it is 2 of 201, smallest gap 1e-5.
    On the MI355X the default loop's own logits had 1 of 201 rows under the gap in bf16 (smallest gap 2.3e-4) and 0 in f32x32
    (2.4e-3); eval step against eager loop 4.8e-7 (bf16) and 5.1e-7 (f32x32).  The eval step's logits are within 1e-4 (f32x32: the fp32 parity bound) /
    1e-5 (bf16: the bound of the capacity-mode test, test_gpu_cogmen.test_capacity_mode_step_equals_exact_step) of the
    eager ones.  Epochs two and three replay the bucket's graph and return the same matrix, bit for bit."""
    from erc_amd.trainer import ResidentEval
    tr, p = _trainer(compute)
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
    err = float((got_logits - ref_logits).abs().max())
    top = ref_logits.double().topk(2, dim=-1).values
    keep = (top[:, 0] - top[:, 1]) >= GAP
    out = n_all - int(keep.sum())
    print("resident eval %s: max|dlogit| vs the eager loop %.3e, %d of %d rows within %g of a tie, min gap %.3e"
          % (compute, err, out, n_all, GAP, float((top[:, 0] - top[:, 1]).min())))
    assert out <= 0.02 * n_all
    assert torch.equal(_cm_of(true[keep], got_logits.argmax(-1)[keep], C), _cm_of(true[keep], ref_logits.argmax(-1)[keep], C))
    assert err < (1e-4 if compute == "f32x32" else 1e-5)
    # replay: no new capture, the same matrix
    for k in (2, 3):
        cm_k = ev.epoch()
        assert ev.captures == 1 and ev.eager == 1 and ev.replays == 3 + 4 * (k - 1)
        assert torch.equal(cm_k, cm1)


def test_eval_scores_takes_a_capacity_sized_static_batch():
    """the same step on a padded static batch (more dialogue slots than dialogues, a longer T, a label buffer of N_cap > N
    entries: the bucket layout of COGMENTrainer.capacity_bucket) counts exactly the batch's utterances and scores them like
    the exact-shape eager forward"""
    tr, p = _trainer("bf16")
    from tests.util_cases import make_batch_lengths
    b = tr.prepare_batch(make_batch_lengths([9, 1, 14], p.dims(), seed=4))
    n = int(b["label"].shape[0])
    tr.t_cap = 20
    key, make, fill = tr.capacity_bucket(b)
    assert key == ("capacity", 4, 20, 80)                           # min(256, B_cap * T_cap)
    static = make()
    static["label"].fill_(99)
    fill(static, b)
    cm = torch.zeros(6, 6, dtype=torch.int64, device=DEV)
    ws = tr.model.eval_scores(static, cm)
    tr.model.eval()
    want = tr.to_logits(b).float()
    assert int(cm.sum()) == n
    assert float((ws["logits"][:n] - want).abs().max()) < 1e-5
    assert torch.equal(cm.cpu(), _cm_of(b["label"].cpu(), ws["logits"][:n].argmax(-1).cpu(), 6))


@pytest.mark.parametrize("compute", ["bf16", "f32x32"])
def test_test_epochs_leave_the_training_state_untouched(compute):
    """six resident training steps (dropout on, the optimizer inside the weight-gradient launch) with a test epoch after
    each pair, and six without: parameters, Adam moments, BatchNorm's running statistics, the optimizer's step count and
    RNG offset and the bf16 weight copies are bit-identical"""
    from erc_amd.trainer import ResidentEpochs, ResidentEval
    states = []
    for with_eval in (True, False):
        tr, p = _trainer(compute)
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
        tr.model.check_cluster()
        if with_eval:
            assert all(int(c.sum()) == sum(LENGTHS[:9]) for c in cms) and ev.captures == 1
        fl, bn = tr.model.flat, tr.model.gcn.bn
        states.append(dict(data=fl.data.clone(), exp_avg=fl.exp_avg.clone(), exp_avg_sq=fl.exp_avg_sq.clone(),
                           rmean=bn.running_mean.clone(), rvar=bn.running_var.clone(), state=tr.optim.state.clone(),
                           shadows=tr.model._sh["catT"].clone(), acc=res.acc.clone()))
    a, b = states
    assert int(a["state"][0]) == 6 and int(a["state"][1]) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_train_mm_cli_resident_eval():
    """``train_mm.py --module=cogmen --compute=bf16 --device_collate --resident --resident_eval``, two epochs on synthetic
    data, as a child process: every epoch line carries ``test`` with all seven metrics and ``test_s``; ``acc`` equals the
    same run's without the flag to within 2 % of the test utterances (a logit pair closer than the two paths' rounding may
    flip its argmax).  Observed on the MI355X: no difference (acc 0.176329 / 0.181159 in both runs; test_s 0.8 ms for the
    epoch that captures, 0.1 ms for the replayed one)."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = ["--module=cogmen", "--dataset=iemocap-cogmen-6", "--epoch=2", "--n_train=20", "--n_test=6", "--train.batch_size=8",
            "--test.batch_size=4", "--compute=bf16", "--device_collate", "--resident"]
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
