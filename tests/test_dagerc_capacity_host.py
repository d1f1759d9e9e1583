"""CPU: DAG-ERC's capacity buckets (DAGERCTrainer.capacity_bucket / all_capacity_buckets / resident_batch /
resident_eval_batch) -- the single node capacity per (B_cap, T_cap), the opt-in flag, every leg of the gate, the static
buffers' fill -- and ``--resident`` / ``--resident_eval`` reaching a DAGERCTrainer through ``trainer.run``.  The HIP runtime
is replaced by recorders that do not execute what they record: there is no GPU here."""
import types

import numpy as np
import pytest
import torch

from erc_amd import capi

BASE = ["--dataset=iemocap-cogmen-6", "--modality=a", "--device=cpu"]


def _trainer(batch_size=4, extra=("--capacity_buckets=True", )):
    from erc_amd.dagerc import DAGERCTrainer
    from track_mm.dagerc import DAGERCParams
    p = DAGERCParams().from_args(BASE + ["--train.batch_size=%d" % batch_size] + list(extra))
    return DAGERCTrainer(p, "cpu")


def _batch(lengths, tr, T=None, dtype=torch.float32, onehot=True):
    B, T, N, D = len(lengths), T or max(lengths), sum(lengths), tr.model.emb_dim
    ids = torch.randint(0, 2, (B, T))
    spk = torch.nn.functional.one_hot(ids, 2).float() if onehot else ids
    return dict(input_tensor=torch.randn(B, T, D).to(dtype), speaker_tensor=spk,
                text_length=torch.tensor(lengths, dtype=torch.int64), label=torch.randint(0, 6, (N, )))


def _store(tr, dtype=torch.float32, rows=10, width=None):
    return types.SimpleNamespace(fused=torch.ones(rows, width or tr.model.emb_dim, dtype=dtype),
                                 speaker=torch.zeros(rows, dtype=torch.int64), label=torch.zeros(rows, dtype=torch.int64))


def test_the_flag_is_off_by_default_and_resident_implies_it():
    from track_mm.dagerc import DAGERCParams
    assert DAGERCParams().capacity_buckets is False
    off = _trainer(extra=())
    off.t_cap = 20
    assert off.capacity is False and off.capacity_bucket(_batch([5, 7, 9], off)) is None
    assert off.all_capacity_buckets(_batch([5, 7, 9], off)) == []
    assert off.resident_batch(_store(off), torch.zeros(8, dtype=torch.int32), 4, 20, 80) is None
    assert _trainer(extra=("--capacity_buckets=True", )).capacity is True
    assert _trainer(extra=("--resident", "--device_collate")).capacity is True


def test_one_node_capacity_per_b_cap_t_cap():
    tr = _trainer(batch_size=4)
    tr.t_cap = 13
    keys = {tr.capacity_bucket(_batch(l, tr))[0] for l in ([13, 1, 7], [1], [5, 5, 5, 5], [13, 13, 13, 12])}
    assert keys == {("capacity", 4, 13, 52)}                       # N_cap = B_cap * T_cap whatever the batch's N
    # a batch larger than train.batch_size or longer than t_cap widens its own bucket
    assert tr.capacity_bucket(_batch([3] * 6, tr, T=20))[0] == ("capacity", 6, 20, 120)
    # a batch of exactly its bucket's shape has nothing to pad: the exact-shape path
    assert tr.capacity_bucket(_batch([13] * 4, tr)) is None
    # integer speaker ids are taken too
    key, make, _ = tr.capacity_bucket(_batch([4, 2], tr, onehot=False))
    assert key == ("capacity", 4, 13, 52) and make()["speaker_tensor"].shape == (4, 13)


def test_every_leg_of_the_gate(monkeypatch):
    from erc_amd.dagerc import MAX_B, MAX_T
    tr = _trainer(batch_size=4)
    tr.t_cap = 13
    ok = _batch([5, 7, 9], tr)
    assert tr.capacity_bucket(ok) is not None and len(tr.all_capacity_buckets(ok)) == 1
    # the recurrence's limits: T_cap <= 1021, B_cap <= 4096
    assert MAX_T == 1021 and MAX_B == 4096
    assert tr._capacity_ok(4, MAX_T, 4 * MAX_T) and not tr._capacity_ok(4, MAX_T + 1, 4 * (MAX_T + 1))
    assert tr._capacity_ok(MAX_B, 13, MAX_B * 13) and not tr._capacity_ok(MAX_B + 1, 13, (MAX_B + 1) * 13)
    assert not tr._capacity_ok(4, 13, 53) and not tr._capacity_ok(4, 13, 0)          # more labels than padded rows / none
    tr.t_cap = MAX_T + 1
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    tr.t_cap = 13
    # the batch's dtype must be the compute mode's, the lengths int64
    assert tr.capacity_bucket(dict(ok, input_tensor=ok["input_tensor"].to(torch.bfloat16))) is None
    assert tr.capacity_bucket(dict(ok, text_length=ok["text_length"].to(torch.int32))) is None
    bf = _trainer(batch_size=4, extra=("--capacity_buckets=True", "--compute=bf16"))
    bf.t_cap = 13
    assert bf.capacity_bucket(ok) is None
    assert bf.capacity_bucket(dict(ok, input_tensor=ok["input_tensor"].to(torch.bfloat16))) is not None
    # the class count must fit the scoring kernel
    lim = capi.rows_score_max_classes()
    assert lim == 16
    tr.model.n_classes = lim + 1
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    tr.model.n_classes = lim
    assert tr.capacity_bucket(ok) is not None
    tr.model.n_classes = 6
    # no bucket with the peer-to-peer exchange
    monkeypatch.setenv("ERC_DP_P2P", "1")
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    monkeypatch.delenv("ERC_DP_P2P")
    tr.model.flat.p2p = object()
    assert tr.capacity_bucket(ok) is None
    assert tr.resident_batch(_store(tr), torch.zeros(8, dtype=torch.int32), 4, 13, 52) is None
    del tr.model.flat.p2p
    assert tr.capacity_bucket(ok) is not None


def test_fill_clears_what_the_previous_batch_left():
    tr = _trainer(batch_size=5)
    tr.t_cap = 10
    big, small = _batch([9, 8, 10, 7, 6], tr), _batch([3, 4, 2], tr)
    key, make, fill = tr.capacity_bucket(big)
    assert key == ("capacity", 5, 10, 50)
    static = make()
    assert static["input_tensor"].shape == (5, 10, tr.model.emb_dim) and static["speaker_tensor"].shape == (5, 10, 2)
    assert static["label"].shape == (50, ) and static["text_length"].dtype == torch.int64
    fill(static, big)
    assert static["extent"] == [5, 10, 40]
    fill(static, small)
    assert static["text_length"].tolist() == [3, 4, 2, 0, 0]
    n = int(small["label"].shape[0])
    assert torch.equal(static["label"][:n], small["label"]) and int(static["label"][n:].abs().sum()) == 0
    for k in ("input_tensor", "speaker_tensor"):
        assert torch.equal(static[k][:3, :4], small[k])
        rest = static[k].clone()
        rest[:3, :4] = 0
        assert float(rest.abs().sum()) == 0.0, k            # nothing of the big batch is left
    fill(static, big)                                       # and back: the big batch in full
    assert torch.equal(static["input_tensor"], big["input_tensor"]) and static["text_length"].tolist() == [9, 8, 10, 7, 6]


@pytest.mark.parametrize("onehot", [True, False])
def test_fill_after_any_sequence_of_batches_equals_a_fresh_buffer(onehot):
    from tests.util_capacity import FILL_SEQ, assert_fill_equals_a_fresh_buffer
    tr = _trainer(batch_size=4)
    tr.t_cap = 12
    batches = [_batch(lens, tr, onehot=onehot) for lens in FILL_SEQ]
    assert_fill_equals_a_fresh_buffer(tr, batches, "input_tensor")
    assert tr.capacity_bucket(batches[0])[1]()["speaker_tensor"].shape == ((4, 12, 2) if onehot else (4, 12))


def test_precapture_list_is_the_single_bucket_with_full_synthetic_lengths():
    tr = _trainer(batch_size=8)
    tr.t_cap = 33
    buckets = tr.all_capacity_buckets(_batch([5, 9, 20], tr))       # (the probe's own shape does not enter)
    assert [b[0] for b in buckets] == [("capacity", 8, 33, 8 * 33)]
    key, make, fill, synth = buckets[0]
    static = make()
    synth(static)
    assert static["text_length"].tolist() == [33] * 8


def test_stepgraphs_replays_the_one_dagerc_bucket():
    from erc_amd.trainer import StepGraphs
    tr = _trainer(batch_size=4)
    tr.t_cap = 30
    calls = []
    tr.train_step = lambda batch: calls.append((int(batch["label"].shape[0]), tr.model.dynamic_n)) or torch.zeros(4)

    class Graphs(StepGraphs):
        def _capture(self, fn):
            fn()
            return types.SimpleNamespace(replay=lambda: calls.append("replay")), torch.zeros(4)

        def _sync(self):
            pass

    g = Graphs(tr)
    for lens in ([10, 20, 30, 4], [3, 4], [30, 30, 30, 29], [1]):
        g.step(_batch(lens, tr))
    # one eager step on the bucket's static buffers + its capture, both under dynamic_n; then replays only
    assert calls == [(120, True), (120, True), "replay", "replay", "replay"]
    assert g.captures == 1 and g.replays == 3 and g.eager == 1 and list(g.cache) == [("capacity", 4, 30, 120)]
    assert tr.model.dynamic_n is False


def test_resident_batch_and_resident_eval_batch_conditions():
    tr = _trainer(batch_size=4)
    desc = torch.zeros(8, dtype=torch.int32)
    store = _store(tr)
    a, b = tr.resident_batch(store, desc, 4, 13, 52), tr.resident_eval_batch(store, desc, 4, 13, 52)
    assert a is not None and b is not None and set(a) == set(b)
    assert a["caps"] == b["caps"] == (4, 13, 52) and a["desc"] is desc and a["text_length"] is None
    assert a["label"] is store.label and a["speaker_tensor"] is store.speaker
    # the features are handed over with one zero row appended, cached per store
    x = a["input_tensor"]
    assert x.shape == (11, tr.model.emb_dim) and torch.equal(x[:10], store.fused) and float(x[10].abs().sum()) == 0.0
    assert b["input_tensor"] is x and tr.resident_batch(store, desc, 4, 13, 52)["input_tensor"] is x
    other = _store(tr)
    assert tr.resident_batch(other, desc, 4, 13, 52)["input_tensor"] is not x
    # refusals: another dtype than the compute mode's, another width, beyond the gate
    assert tr.resident_batch(_store(tr, torch.bfloat16), desc, 4, 13, 52) is None
    assert tr.resident_eval_batch(_store(tr, torch.bfloat16), desc, 4, 13, 52) is None
    assert tr.resident_batch(_store(tr, width=tr.model.emb_dim + 1), desc, 4, 13, 52) is None
    assert tr.resident_batch(store, desc, 4, 1022, 4 * 1022) is None
    assert tr.resident_batch(store, desc, 4, 13, 53) is None
    bf = _trainer(batch_size=4, extra=("--resident", "--device_collate", "--compute=bf16"))
    assert bf.resident_batch(_store(bf), desc, 4, 13, 52) is None
    xb = bf.resident_batch(_store(bf, torch.bfloat16), desc, 4, 13, 52)["input_tensor"]
    assert xb.dtype == torch.bfloat16 and xb.shape[0] == 11


def test_eval_scores_and_a_resident_step_refuse_before_any_launch():
    tr = _trainer(batch_size=4)
    store, desc = _store(tr), torch.zeros(8, dtype=torch.int32)
    b = tr.resident_batch(store, desc, 4, 13, 52)
    with pytest.raises(capi.ErcGraftError, match="capacity mode"):
        tr.model.loss_and_grads(b)                           # outside dynamic_n
    tr.model.n_classes = 17
    with pytest.raises(capi.ErcGraftError, match="supports_capacity"):
        tr.model.eval_scores(b, torch.zeros(17, 17, dtype=torch.int64))


def _patched_run(monkeypatch, argv):
    """the run believes a GPU is there; every ResidentEpochs / ResidentEval it builds is recorded"""
    from erc_amd import trainer as trainer_mod
    from erc_amd.dagerc import DAGERCTrainer
    from track_mm.dagerc import DAGERCParams
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "manual_seed_all", lambda s: None)
    built = []
    for cls in (trainer_mod.ResidentEpochs, trainer_mod.ResidentEval):
        def init(self, *a, _orig=cls.__init__, **k):
            _orig(self, *a, **k)
            built.append(self)
        monkeypatch.setattr(cls, "__init__", init)
    return trainer_mod.run(DAGERCTrainer, DAGERCParams, argv), built


ARGV = BASE + ["--epoch=0", "--n_train=12", "--n_test=5", "--train.batch_size=4", "--test.batch_size=3", "--device_collate"]


def test_resident_and_resident_eval_reach_a_dagerc_trainer(monkeypatch):
    from erc_amd.dagerc import DAGERCTrainer
    from erc_amd.trainer import ResidentEpochs, ResidentEval
    out, built = _patched_run(monkeypatch, ARGV + ["--resident", "--resident_eval"])
    assert out == {} and [type(b) for b in built] == [ResidentEpochs, ResidentEval]
    res, ev = built
    assert isinstance(res.trainer, DAGERCTrainer) and res.trainer.capacity and res.supported() and ev.supported()
    # ONE node capacity each: B * T of the loop's own store
    assert res.N_BUCKET == res.B * res.T == 4 * int(res.store.lengths.max())
    assert ev.N_BUCKET == ev.B * ev.T == 3 * int(ev.store.lengths.max())
    assert set(ev.caps) == {ev.B * ev.T} and ev.steps == 2
    assert ev.cm.shape == (6, 6) and ev.cm.dtype == torch.int64


def test_without_the_flags_the_run_builds_neither(monkeypatch):
    out, built = _patched_run(monkeypatch, ARGV)
    assert out == {} and built == []
    with pytest.raises(SystemExit, match="--resident_eval needs --resident"):
        _patched_run(monkeypatch, ARGV + ["--resident_eval"])
    with pytest.raises(SystemExit, match="--resident needs --device_collate"):
        _patched_run(monkeypatch, [a for a in ARGV if a != "--device_collate"] + ["--resident"])


class _LenStore(types.SimpleNamespace):
    """what the resident loops read of a DeviceDialogueStore"""
    DESC_INTS = 2
    t_max = property(lambda self: int(self.lengths.max()))

    def __len__(self):
        return int(self.lengths.numel())


def test_a_resident_epoch_is_one_capture_and_otherwise_replays():
    """ResidentEpochs / ResidentEval over a DAGERCTrainer with recorders in place of the step and of the capture"""
    from erc_amd.trainer import ResidentEpochs, ResidentEval
    tr = _trainer(batch_size=4, extra=("--resident", "--device_collate"))
    lens = torch.tensor([5, 9, 3, 7, 9, 2, 6, 4, 8, 1], dtype=torch.int64)
    offs = torch.zeros(11, dtype=torch.int64)
    offs[1:] = torch.cumsum(lens, 0)
    U = int(lens.sum())
    store = _LenStore(fused=torch.zeros(U, tr.model.emb_dim), speaker=torch.zeros(U, dtype=torch.int64),
                      label=torch.zeros(U, dtype=torch.int64), lengths=lens, offsets=offs, device="cpu")
    log = []
    tr.train_step = lambda b: log.append(("step", b["caps"], tr.model.dynamic_n)) or torch.zeros(4)
    tr.resident_eval_step = lambda b, cm: log.append(("eval", b["caps"])) or {}

    class Train(ResidentEpochs):
        def _capture(self, fn):
            fn()
            return types.SimpleNamespace(replay=lambda: log.append("replay"))

    class Eval(ResidentEval):
        def _capture(self, fn):
            fn()
            return types.SimpleNamespace(replay=lambda: log.append("replay"))

    res = Train(tr, store, 4, seed=3)
    assert res.supported() and res.N_BUCKET == 36
    n_utt, n_steps = res.epoch()
    assert (n_utt, n_steps) == (U, 3)
    assert log == [("step", (4, 9, 36), True), ("step", (4, 9, 36), True), "replay", "replay"]
    assert (res.captures, res.eager, res.replays) == (1, 1, 2) and list(res.graphs) == [36]
    res.epoch()
    assert (res.captures, res.eager, res.replays) == (1, 1, 5)
    del log[:]
    ev = Eval(tr, store, 3, n_classes=6)
    assert ev.supported() and ev.caps == [27] * 4
    cm = ev.epoch()
    assert log == [("eval", (3, 9, 27)), ("eval", (3, 9, 27)), "replay", "replay", "replay"] and cm.shape == (6, 6)
    assert np.array_equal(ev.table[:, :3].sum(1), [17, 18, 18, 1])


def test_resident_loop_takes_the_trainers_node_bucket_and_keeps_128_otherwise():
    from erc_amd.trainer import ResidentLoop
    lens = torch.tensor([50, 60, 70], dtype=torch.int64)
    store = types.SimpleNamespace(lengths=lens, t_max=70, DESC_INTS=2, device="cpu")
    plain = ResidentLoop(types.SimpleNamespace(), store, 4)
    assert plain.N_BUCKET == 128 and plain._caps_of([1, 128, 129, 280]) == [128, 128, 256, 280]
    named = ResidentLoop(types.SimpleNamespace(RESIDENT_N_BUCKET=64), store, 4)
    assert named.N_BUCKET == 64 and named._caps_of([1, 65]) == [64, 128]
    dag = ResidentLoop(_trainer(), store, 4)
    assert dag.N_BUCKET == 280 and dag._caps_of([1, 128, 129, 280]) == [280] * 4
    assert ResidentLoop.N_BUCKET == 128                      # (the class default is untouched)
    for mod, name in (("dgcn", "DGCNTrainer"), ("cogmen", "COGMENTrainer"), ("bcrnn", "BcLstmTrainer")):
        cls = getattr(__import__("erc_amd." + mod, fromlist=[name]), name)
        assert getattr(cls, "RESIDENT_N_BUCKET", None) is None, name
