"""CPU: the host side of --module=mmin_base from HBM -- the collate restatement (tests/mmin_cap_ref.py) against
``mmin.mmin_collate``, an epoch's descriptor tables against a DataLoader on the same generator, the trainer's buckets and their
fill, the resident loops under a recorder in place of the HIP runtime (their ``_capture`` seam), and the flags.  No library is
loaded: there is no GPU here."""
import types

import pytest
import torch
from torch.utils.data import DataLoader

from erc_amd import capi, mmin
from erc_amd.datasets import MMIN_T_BUCKET, MMINDeviceStore, index_batches, mmin_t_cap
from tests import mmin_cap_ref as R

TV, TT = 4, 6


def _samples(n=11, frames=(3, 150), seed=5):
    return R.small_samples(n, frames, seed=seed, tv=TV, tt=TT)


# ---------------------------------------------------------------------------------------------------------------- collate
@pytest.mark.parametrize("idx, B_cap, T_cap", [((4, 0, 9), 4, 192), ((2, ), 1, 150), ((7, 1), 2, 64 * 3), ((3, 5, 6, 8, 10), 5, 150)])
def test_collate_restatement_equals_mmin_collate_at_capacity_pitch(idx, B_cap, T_cap):
    samples = _samples()
    store = R.host_store(samples)
    host = mmin.mmin_collate([samples[i] for i in idx])
    B, Ta = host["audio_feature"].shape[:2]
    assert Ta <= T_cap
    desc = store.desc(idx, B_cap)
    assert desc.dtype.name == "int32" and desc.shape == (3 * B_cap, )
    audio, visual, text, label, counts = R.collate_ref(store, desc, B_cap, T_cap)
    assert torch.equal(audio[:B, :Ta], host["audio_feature"]) and not audio[:B, Ta:].any() and not audio[B:].any()
    assert torch.equal(visual[:B], host["visual_feature"]) and not visual[B:].any()
    assert torch.equal(text[:B], host["text_feature"]) and not text[B:].any()
    assert torch.equal(label[:B], host["label"]) and not label[B:].any()
    assert counts.tolist() == [B, Ta] and counts.dtype == torch.int32


def test_store_layout():
    samples = _samples()
    st = MMINDeviceStore(samples, None)
    lens = [s["audio_feature"].shape[0] for s in samples]
    assert len(st) == 11 and st.lengths.tolist() == lens and st.t_max == max(lens)
    assert st.offsets.tolist() == [sum(lens[:i]) for i in range(12)]
    assert st.audio.shape == (sum(lens), 130) and st.visual.shape == (11, TV, 342) and st.text.shape == (11, TT, 1024)
    assert st.label.dtype == torch.int64 and st.label.tolist() == [s["label"] for s in samples]
    for i in (0, 5, 10):
        assert torch.equal(st.audio[st.offsets[i]:st.offsets[i + 1]], torch.from_numpy(samples[i]["audio_feature"]))
    with pytest.raises(ValueError):
        st.desc(range(5), 4)


def test_t_capacity_rule():
    assert MMIN_T_BUCKET == 64
    assert [mmin_t_cap(t, 400) for t in (1, 63, 64, 65, 128, 129, 384, 385, 400)] == [64, 64, 64, 128, 128, 192, 384, 400, 400]
    assert mmin_t_cap(30, 40) == 40 and mmin_t_cap(40, 40) == 40          # never longer than the split's longest utterance
    assert mmin_t_cap(65, 0) == 128 and mmin_t_cap(65, None) == 128


# ----------------------------------------------------------------------------------------------------------------- tables
def test_epoch_tables_follow_the_dataloader():
    """every sample once, a short last batch, empty slots last, T_cap by the rule, and the order of a DataLoader on a generator
    in the same state -- over two epochs (the second draw continues the generator like the loader's second epoch)"""
    samples = _samples(n=11)
    store, B = R.host_store(samples), 4
    loader = DataLoader(samples, batch_size=B, shuffle=True, collate_fn=mmin.mmin_collate, generator=torch.Generator().manual_seed(9))
    gen = torch.Generator().manual_seed(9)
    for _ in range(2):
        names = [b["name"] for b in loader]
        batches = index_batches(len(store), B, True, gen)
        assert [[samples[i]["name"] for i in b] for b in batches] == names
        assert sorted(i for b in batches for i in b) == list(range(11)) and [len(b) for b in batches] == [4, 4, 3]
        table, caps = store.table(batches, B)
        assert table.shape == (3, 3 * B) and table.dtype.name == "int32"
        for row, idx, cap in zip(table, batches, caps):
            fr, first, sid = row.reshape(3, B).tolist()
            pad = [0] * (B - len(idx))
            assert fr == [int(store.lengths[i]) for i in idx] + pad and first == [int(store.offsets[i]) for i in idx] + pad
            assert sid == list(idx) + pad
            assert cap == mmin_t_cap(max(fr), store.t_max) and cap >= max(fr) and (cap % 64 == 0 or cap == store.t_max)
    assert index_batches(5, 2, False) == [[0, 1], [2, 3], [4]]


# ---------------------------------------------------------------------------------------------------------------- trainer
def _trainer(*argv):
    from track_mm.mmin_base import MMINBaseParams
    p = MMINBaseParams().from_args(["--train.batch_size=4", "--val.batch_size=4", "--test.batch_size=4"] + list(argv))
    return mmin.MMINBaseTrainer(p, "cpu")


def _loop(*argv):
    """the epoch loop on the CPU over real tiny splits -> (loop, trainer)"""
    t = _trainer("--n_train=5", "--n_val=5", "--n_test=5", "--mmin_frames=3,150", *argv)
    return mmin.MMINEpochLoop(t.params, t, torch.device("cpu")), t


def test_flags():
    from track_mm.mmin_base import MMINBaseParams
    p = MMINBaseParams().from_args([])
    assert not any(p.get(k) for k in mmin.CAPACITY_FLAGS)
    assert mmin.CAPACITY_FLAGS == ("capacity_buckets", "device_collate", "resident", "resident_eval")
    tr = _trainer()
    assert tr.capacity is False and tr.model.dynamic_n is False and tr.CAPACITY_MODES
    assert tr.capacity_bucket(mmin.mmin_collate(_samples(3))) is None
    assert _trainer("--capacity_buckets=True").capacity and _trainer("--device_collate", "--resident").capacity
    from erc_amd.trainer import epoch_loop_class
    from erc_amd.mmin_miss import MMINMissTrainer
    assert epoch_loop_class(mmin.MMINBaseTrainer) is epoch_loop_class(MMINMissTrainer) is mmin.MMINEpochLoop
    none, t = _loop()
    assert (none.graphs, none.fixed, none.resident, none.res_val, none.res_eval) == (None, ) * 5 and none.counters is None
    assert t.t_cap == 0 and none.n_steps == 2 and tuple(none.ring.shape) == (2, 4)
    assert [len(ld.dataset) for ld in (none.train_loader, none.val_loader, none.test_loader)] == [5, 5, 5]
    both = "--module=mmin_base: --resident runs from the device store of --device_collate; give both or neither"
    needs = "--module=mmin_base: --resident_eval needs --device_collate --resident"
    for argv, wording in ((("--resident", ), both), (("--device_collate", ), both), (("--resident_eval", ), needs),
                          (("--resident_eval", "--capacity_buckets=True"), needs)):
        t = _trainer("--n_train=5", "--n_val=5", "--n_test=5", "--mmin_frames=3,150", *argv)      # the trainer takes the flags ...
        with pytest.raises(SystemExit) as exc:                                                    # ... the loop refuses them
            mmin.MMINEpochLoop(t.params, t, torch.device("cpu"))
        assert str(exc.value) == wording
    loops, t = _loop("--capacity_buckets=True")
    assert loops.graphs is not None and loops.resident is None
    assert t.t_cap == max(s["audio_feature"].shape[0] for s in loops.train_loader.dataset) > 0


def test_data_parallel_runs_stay_refused(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    for flag in ("--capacity_buckets=True", "--resident", "--device_collate", "--resident_eval"):
        with pytest.raises(capi.ErcGraftError, match="one rank"):
            _trainer(flag)
    assert _trainer().capacity is False        # the default loop is what it was


def test_mmin_miss_keeps_its_refusals():
    from erc_amd.mmin_miss import MMINMissTrainer
    from track_mm.mmin_miss import MMINMissParams
    assert MMINMissTrainer.CAPACITY_MODES is False
    for flag in ("--capacity_buckets=True", "--resident", "--resident_eval"):
        with pytest.raises(capi.ErcGraftError, match="not built"):
            MMINMissTrainer(MMINMissParams().from_args([flag]), "cpu")


def test_bucket_key_buffers_and_fill():
    tr = _trainer("--capacity_buckets=True")
    tr.t_cap = 150
    samples = _samples()
    big, small = mmin.mmin_collate(samples[:4]), mmin.mmin_collate([samples[2], samples[7]])
    key, make, fill = tr.capacity_bucket(big)
    Ta = big["audio_feature"].shape[1]
    assert key == ("capacity", 4, mmin_t_cap(Ta, 150), TV, TT)
    assert tr.capacity_bucket(mmin.mmin_collate(samples[:5])) is None             # more samples than train.batch_size
    static = make()
    T_cap = key[2]
    assert static["audio_feature"].shape == (4, T_cap, 130) and static["visual_feature"].shape == (4, TV, 342)
    assert static["text_feature"].shape == (4, TT, 1024) and static["label"].dtype == torch.int64 and static["counts"].dtype == torch.int32
    fill(static, big)
    assert static["counts"].tolist() == [4, Ta] and torch.equal(static["audio_feature"][:, :Ta], big["audio_feature"])
    fill(static, small)                                                            # a long batch, then a short one: nothing stale
    st = R.host_store(samples)
    ref = R.collate_ref(st, st.desc([2, 7], 4), 4, T_cap)
    for k, r in zip(("audio_feature", "visual_feature", "text_feature", "label", "counts"), ref):
        assert torch.equal(static[k], r), k


# ------------------------------------------------------------------------------------------------------------------ loops
class _Model:
    dynamic_n = False
    _last_ws = "ws"


class _Trainer:
    """records what a step would run on; a resident batch is the descriptor buffer and its T capacity"""
    use_ema = True

    def __init__(self):
        self.model, self.steps, self.evals, self.ema_passes = _Model(), [], [], 0
        self.params = types.SimpleNamespace(n_classes=4)

    def resident_batch(self, store, cur_desc, B_cap, T_cap):
        return dict(desc=cur_desc, T_cap=T_cap, B_cap=B_cap)

    def train_step(self, batch):
        self.steps.append((batch["T_cap"], batch["desc"].tolist(), self.model.dynamic_n))
        return torch.ones(4)

    def resident_eval_step(self, batch, cm, loss_sum):
        self.evals.append((batch["T_cap"], batch["desc"].tolist(), self.model.dynamic_n))
        cm[0, 0] += 1
        loss_sum += 0.5
        return "ws"

    def ema_weights(self):
        import contextlib
        self.ema_passes += 1
        return contextlib.nullcontext()


def _recorder(loop, calls):
    """a capture records and does not execute, like the real one; a replay notes the descriptor it would run on"""
    loop._capture = lambda fn: types.SimpleNamespace(replay=lambda: calls.append(("replay", loop.cur_desc.tolist())))
    return loop


def test_resident_epochs_one_eager_visit_per_t_cap_then_replays_and_recapture_after_lr_change():
    samples = _samples(n=11, frames=(3, 150))
    store, B, tr, calls = R.host_store(samples), 4, _Trainer(), []
    res = _recorder(mmin.MMINResidentEpochs(tr, store, B, torch.Generator().manual_seed(9)), calls)
    assert res.cur_desc.shape == (3 * B, ) and res.cur_desc.dtype == torch.int32 and res.T == store.t_max
    expect = torch.Generator().manual_seed(9)
    seen, n_steps = set(), 0
    for epoch in range(3):
        table, caps = store.table(index_batches(11, B, True, expect), B)
        before = len(tr.steps), len(calls)
        assert res.epoch() == [4, 4, 3]
        new_steps, new_calls = tr.steps[before[0]:], calls[before[1]:]
        fresh = [c for i, c in enumerate(caps) if c not in seen and c not in caps[:i]]
        assert [s[0] for s in new_steps] == fresh                      # one eager step per T capacity not seen before
        assert all(s[2] for s in new_steps) and tr.model.dynamic_n is False
        assert len(new_calls) == 3 - len(fresh)
        rows = [s[1] for s in new_steps] + [c[1] for c in new_calls]
        assert sorted(rows) == sorted(r.tolist() for r in table)       # every step ran on its own row of the table
        seen |= set(caps)
        n_steps += 3
    assert res.eager == res.captures == len(seen) and res.replays == n_steps - len(seen)
    assert float(res.acc[0]) == res.eager                               # replays add nothing under the recorder
    # a learning-rate change drops the graphs and keeps the buffers: one more eager step and capture per capacity that comes up
    batches = {cap: ent[1] for cap, ent in res.graphs.items()}
    res.drop_graphs()
    assert all(ent[0] is None and ent[1] is batches[cap] for cap, ent in res.graphs.items())
    eager, captures = res.eager, res.captures
    table, caps = store.table(index_batches(11, B, True, expect), B)
    res.epoch()
    assert res.eager - eager == res.captures - captures == len(set(caps))
    # without capture every step stays eager
    plain = mmin.MMINResidentEpochs(_Trainer(), store, B, torch.Generator().manual_seed(9), capture=False)
    plain.epoch()
    assert (plain.eager, plain.captures, plain.replays) == (3, 0, 0)


def test_capacity_loops_drop_the_graphs_when_the_learning_rate_changes():
    """``test_epoch`` with the trainer's two evaluation hooks replaced (no library here): validation, the scheduler, the test
    epoch, in this order; the graphs go exactly when ``on_eval_end`` reports a change"""
    from erc_amd.trainer import GraphEntry
    loops, tr = _loop("--capacity_buckets=True")
    log, changed = [], [False]
    tr.eval_epoch = lambda loader: log.append(loader) or {"Lall": float(len(log))}
    tr.on_eval_end = lambda rec: log.append(rec) or changed[0]
    graph, out = object(), object()
    ent = loops.graphs.cache["k"] = GraphEntry({}, None, True, seen=3, graph=graph, out=out, workspace="ws")
    assert loops.test_epoch() == ({"Lall": 1.0}, {"Lall": 3.0})
    assert log == [loops.val_loader, {"Lall": 1.0}, loops.test_loader]
    assert ent.graph is graph and ent.out is out                      # the learning rate stayed: nothing is dropped
    changed[0] = True
    loops.test_epoch()
    assert ent.graph is None and ent.out is None and loops.graphs.cache["k"] is ent
    assert (ent.static, ent.seen, ent.workspace) == ({}, 3, "ws")     # the static buffers and the workspace stay
    c = loops.counters
    assert (c.replays, c.eager, c.captures) == (0, 0, 0)
    loops.graphs.replays, loops.graphs.eager, loops.graphs.captures = 5, 2, 1
    assert (c.replays, c.eager, c.captures) == (5, 2, 1)


def test_resident_eval_fixed_order_two_passes_one_result():
    samples = _samples(n=7, frames=(3, 150))
    store, B, tr, calls = R.host_store(samples), 4, _Trainer(), []
    ev = _recorder(mmin.MMINResidentEval(tr, store, B), calls)
    assert ev.cur_desc.shape == (3 * B, ) and ev.cur_desc.dtype == torch.int32 and ev.T == store.t_max
    table, caps = store.table([[0, 1, 2, 3], [4, 5, 6]], B)
    assert ev.table_dev.tolist() == table.tolist() and ev.caps == caps
    out = ev.epoch()
    assert tr.ema_passes == 1 and [e[0] for e in tr.evals] == sorted(set(caps), key=caps.index)
    assert all(e[2] for e in tr.evals) and tr.model.dynamic_n is False
    # pass 1 ran every capacity eagerly (the recorder's replays add nothing): its matrix and sum are those steps'; pass 2 replays
    n = len(set(caps))
    assert out["cm"][0, 0] == n and out["Lall"] == 0.5 * n and out["C"] == n and out["Acc"] == 1.0
    assert out["cm2"].sum() == 0 and out["Acc2"] == 0.0
    assert len(calls) == (2 - n) + 2 and ev.replays == len(calls) and ev.eager == ev.captures == n
    tr.use_ema = False
    assert "Acc2" not in ev.epoch() and tr.ema_passes == 1
