"""CPU: the host side of ``--resident_eval`` -- ``report_from_cm`` against the sklearn metric set of the default test loop,
``ResidentEval``'s planning (table, order, padding, capacities, T) and its epoch loop under a recorder in place of the HIP
runtime, and the flag handling of ``trainer.run``."""
import types

import numpy as np
import pytest
import torch

KEYS = ("acc", "wa", "pre", "rec", "f1", "mif1", "maf1")


def _cm(true, pred, C):
    cm = np.zeros((C, C), dtype=np.int64)
    np.add.at(cm, (np.asarray(true), np.asarray(pred)), 1)
    return cm


def _cases(C):
    rng = np.random.RandomState(100 + C)
    n = 257
    out = {}
    true, pred = rng.randint(0, C, n), rng.randint(0, C, n)
    true[:C], pred[:C] = np.arange(C), np.arange(C)[::-1]                # every class in both
    out["all classes present"] = (true, pred)
    t2 = rng.randint(0, C - 1, n)                                        # class C-1 never a label ...
    p2 = rng.randint(0, C, n)
    p2[:3] = C - 1                                                       # ... but predicted
    out["absent from the labels, predicted"] = (t2, p2)
    out["absent from both"] = (rng.randint(1, C, n), rng.randint(1, C, n))
    out["n = 1, right"] = (np.array([C - 2]), np.array([C - 2]))
    out["n = 1, wrong"] = (np.array([1]), np.array([0]))
    t5 = rng.randint(0, C, n)
    out["all predictions wrong"] = (t5, (t5 + 1 + rng.randint(0, C - 1, n)) % C)
    out["five samples"] = (rng.randint(0, C, 5), rng.randint(0, C, 5))
    return out


@pytest.mark.parametrize("C", [4, 6, 7])
def test_report_from_cm_equals_the_sklearn_metric_set(C):
    import warnings
    from erc_amd.trainer import classification_report, report_from_cm
    for name, (true, pred) in _cases(C).items():
        if name == "all predictions wrong":
            assert not (true == pred).any()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                              # (sklearn warns about labels that never occur)
            want = classification_report(true.tolist(), pred.tolist(), C)
        got = report_from_cm(_cm(true, pred, C))
        assert set(got) == set(want), name
        assert got["cm"] == want["cm"], name
        for k in KEYS:
            assert abs(got[k] - want[k]) <= 1e-12, (name, k, got[k], want[k])


def test_report_from_cm_takes_lists_and_tensors():
    from erc_amd.trainer import report_from_cm
    cm = [[3, 1], [0, 4]]
    a, b = report_from_cm(cm), report_from_cm(torch.tensor(cm).numpy())
    assert a == b and a["acc"] == 7 / 8 and a["mif1"] == a["acc"] and a["wa"] == (3 / 4 + 1.0) / 2


# ----------------------------------------------------------------------------------------------------------- planning
class _Store:
    DESC_INTS = 2

    def __init__(self, lengths):
        self.lengths = torch.tensor(lengths, dtype=torch.int64)
        self.t_max = max(lengths)
        self.offsets = torch.zeros(len(lengths) + 1, dtype=torch.int64)
        self.offsets[1:] = torch.cumsum(self.lengths, 0)
        self.device = "cpu"

    def __len__(self):
        return int(self.lengths.numel())


class _Trainer:
    """what ResidentEval asks of a trainer: ``resident_eval_batch`` and ``resident_eval_step``"""

    def __init__(self, C=4, refuse_above=None):
        self.params = types.SimpleNamespace(n_classes=C)
        self.t_cap = 999                       # the TRAINING store's longest dialogue: not what the test buckets use
        self.refuse_above = refuse_above
        self.steps = []

    def resident_eval_batch(self, store, cur_desc, B_cap, T_cap, N_cap):
        if self.refuse_above is not None and N_cap > self.refuse_above:
            return None
        return dict(desc=cur_desc, caps=(B_cap, T_cap, N_cap))

    def resident_eval_step(self, batch, cm):
        self.steps.append((batch["caps"], batch["desc"].tolist()))
        cm[0, 1] += int(batch["desc"][:batch["caps"][0]].sum())          # "scores" every node of the batch
        return {"buffers": batch["caps"]}


def _recorder(ev, calls):
    """a capture records and does not execute, like the real one"""
    ev._capture = lambda fn: types.SimpleNamespace(replay=lambda: calls.append("replay"))
    return ev


def test_plan_is_sequential_padded_and_bucketed_by_the_test_stores_own_t():
    from erc_amd.trainer import ResidentEval
    lengths = [40, 3, 50, 7, 1, 60, 60, 60, 60, 2]                       # n = 10, B = 4 -> 3 steps, the last with 2 dialogues
    st = _Store(lengths)
    ev = ResidentEval(_Trainer(), st, 4)
    assert ev.steps == 3 == -(-len(lengths) // 4) and ev.table.shape == (3, 8) and ev.table.dtype == np.int32
    assert ev.T == 60                                                    # not the trainer's t_cap
    offs = st.offsets[:-1].tolist()
    for s in range(3):
        ids = list(range(4 * s, min(4 * s + 4, 10)))                     # the store's order, nothing shuffled
        pad = [0] * (4 - len(ids))
        assert ev.table[s, :4].tolist() == [lengths[i] for i in ids] + pad
        assert ev.table[s, 4:].tolist() == [offs[i] for i in ids] + pad
    assert ev.counts == [100, 181, 62]
    assert ev.N_BUCKET == 128
    assert ev.caps == [128, 240, 128]                                    # 181 -> 256, capped at B * T = 240
    assert torch.equal(ev.table_dev, torch.from_numpy(ev.table)) and ev.cur_desc.shape == (8, ) and ev.cur_desc.dtype == torch.int32
    assert ev.cm.shape == (4, 4) and ev.cm.dtype == torch.int64
    # a batch that fills its bucket exactly keeps that bucket
    assert ResidentEval(_Trainer(), _Store([64, 64, 5]), 2).caps == [128, 128]
    assert ResidentEval(_Trainer(), _Store([64, 64, 64, 1]), 2).caps == [128, 128]      # 65 -> 128 = B * T


def test_supported_asks_for_every_bucket_of_the_table():
    from erc_amd.trainer import ResidentEval
    st = _Store([40, 3, 50, 7, 1, 60, 60, 60, 60, 2])
    assert ResidentEval(_Trainer(), st, 4).supported()
    assert not ResidentEval(_Trainer(refuse_above=128), st, 4).supported()
    assert ResidentEval(_Trainer(refuse_above=240), st, 4).supported()


def test_epoch_runs_a_bucket_eagerly_once_then_replays_it():
    from erc_amd.trainer import ResidentEval
    lengths = [40, 3, 50, 7, 1, 60, 60, 60, 60, 2]
    tr, calls = _Trainer(), []
    ev = _recorder(ResidentEval(tr, _Store(lengths), 4), calls)
    cm = ev.epoch()
    # steps 0 and 1 open the buckets 128 and 240 (one eager run each; the capture records, it does not run); step 2 replays 128
    assert (ev.eager, ev.captures, ev.replays) == (2, 2, 1) and calls == ["replay"]
    assert [c for c, _ in tr.steps] == [(4, 60, 128), (4, 60, 240)]
    assert tr.steps[0][1] == ev.table[0].tolist() and tr.steps[1][1] == ev.table[1].tolist()
    assert int(cm[0, 1]) == 100 + 181 and cm.device.type == "cpu"
    assert sorted(ev.graphs) == [128, 240] and ev.graphs[128][2] == {"buffers": (4, 60, 128)}
    assert ev.cur_desc.tolist() == ev.table[2].tolist()                  # the last step's description is in place for the replay
    ev.epoch()
    assert (ev.eager, ev.captures, ev.replays) == (2, 2, 4) and len(tr.steps) == 2
    assert int(ev.cm.sum()) == 0                                         # zeroed at the start; replays are recorded, not run


def test_epoch_without_capture_stays_eager():
    from erc_amd.trainer import ResidentEval
    tr = _Trainer()
    ev = ResidentEval(tr, _Store([5, 6, 7]), 2, capture=False)
    assert ev.epoch()[0, 1] == 18 and ev.epoch()[0, 1] == 18
    assert (ev.eager, ev.captures, ev.replays) == (4, 0, 0)


# ---------------------------------------------------------------------------------------------------------- trainer.run
ARGV = ["--dataset=meld-mmgcn-7", "--loss_weights=False", "--device=cpu", "--epoch=0", "--n_train=12", "--n_test=4",
        "--train.batch_size=4", "--test.batch_size=3", "--device_collate"]


def _patched_run(monkeypatch, argv, cls, params_cls=None):
    from erc_amd import trainer as trainer_mod
    from track_mm.bclstm import BcRnnParams
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "manual_seed_all", lambda s: None)
    built = []
    orig = trainer_mod.ResidentEval.__init__

    def init(self, *a, **k):
        orig(self, *a, **k)
        built.append(self)
    monkeypatch.setattr(trainer_mod.ResidentEval, "__init__", init)
    return trainer_mod.run(cls, params_cls or BcRnnParams, argv), built


def _with_eval_step():
    from erc_amd.bcrnn import BcGruTrainer

    class T(BcGruTrainer):
        def resident_eval_batch(self, store, cur_desc, B_cap, T_cap, N_cap):
            return self.resident_batch(store, cur_desc, B_cap, T_cap, N_cap)

        def resident_eval_step(self, batch, cm):
            raise AssertionError("no epoch runs in this test")
    return T


def test_resident_eval_needs_resident(monkeypatch):
    with pytest.raises(SystemExit) as exc:
        _patched_run(monkeypatch, ARGV + ["--resident_eval"], _with_eval_step())
    assert str(exc.value) == "--resident_eval needs --resident (the test epoch then runs from the HBM-resident test store)"


def test_resident_eval_needs_a_trainer_with_the_step(monkeypatch):
    from erc_amd.bcrnn import BcGruTrainer
    with pytest.raises(SystemExit) as exc:
        _patched_run(monkeypatch, ARGV + ["--resident", "--resident_eval"], BcGruTrainer)
    assert str(exc.value) == "--resident_eval: this module's trainer has no resident_eval_step (--module=cogmen has one)"


def test_resident_eval_refuses_the_multi_label_metrics(monkeypatch):
    from track_mm.bclstm import BcRnnParams

    class P(BcRnnParams):
        def iparams(self):
            super().iparams()
            self.mosei_metric = "multiemo"
            return self
    with pytest.raises(SystemExit) as exc:
        _patched_run(monkeypatch, ARGV + ["--resident", "--resident_eval"], _with_eval_step(), P)
    assert str(exc.value).startswith("--resident_eval: mosei_metric=multiemo")


def test_the_flag_builds_one_resident_eval_over_the_test_store(monkeypatch):
    out, built = _patched_run(monkeypatch, ARGV + ["--resident", "--resident_eval"], _with_eval_step())
    assert out == {} and len(built) == 1
    ev = built[0]
    assert len(ev.store) == 4 and ev.B == 3 and ev.steps == 2 and ev.supported()
    assert ev.T == int(ev.store.lengths.max())


@pytest.mark.parametrize("extra", [[], ["--resident"]])
def test_without_the_flag_no_resident_eval_is_built(monkeypatch, extra):
    out, built = _patched_run(monkeypatch, ARGV + extra, _with_eval_step())
    assert out == {} and built == []
