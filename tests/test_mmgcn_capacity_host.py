"""CPU: MMGCN's capacity buckets (MMGCNTrainer.capacity_bucket / all_capacity_buckets / resident_batch /
resident_eval_batch) -- the bucket keys, the time-major static buffers and their fill, every refusal of the gate, the
precapture list -- and ``--resident`` / ``--resident_eval`` reaching an unmodified MMGCNTrainer through ``trainer.run``.
The HIP runtime is replaced by recorders that do not execute what they record, and erc_gcnii_chain_config (which asks the
device for its CU count) by its arithmetic for a 256-CU device: there is no GPU here."""
import types

import pytest
import torch

from erc_amd import capi

BASE = ["--dataset=iemocap-cogmen-6", "--modality=atv", "--device=cpu"]
DIMS = dict(a=100, t=100, v=512)
KEYS = dict(a="audio_feature", t="text_feature", v="visual_feature")


def _chain_config_256(B, T, Mo, P):
    """what erc_gcnii_chain_config answers on a device of 256 CUs (csrc/gcnii_chain.hip)"""
    if not (B > 0 and 0 < T <= 128 and 2 <= Mo <= 3 and P >= T):
        raise capi.ErcGraftError("gcnii_chain_config: B=%d T=%d modalities=%d (T <= 128)" % (B, T, Mo))
    worst = Mo * ((T + 31) // 32)
    return (T + 15) // 16, 256, min(256 // worst, B)


@pytest.fixture(autouse=True)
def chain_config(monkeypatch):
    monkeypatch.setattr(capi, "gcnii_chain_config", _chain_config_256)
    monkeypatch.delenv("ERC_MM_CHAIN", raising=False)
    monkeypatch.delenv("ERC_DP_P2P", raising=False)


def _trainer(batch_size=4, extra=("--capacity_buckets=True", ), modality="atv"):
    from erc_amd.mmgcn import MMGCNTrainer
    from track_mm.mmgcn import MMGCNParams
    p = MMGCNParams().from_args([a for a in BASE if not a.startswith("--modality")] + ["--modality=" + modality] +
                                ["--train.batch_size=%d" % batch_size] + list(extra))
    return MMGCNTrainer(p, "cpu")


def _batch(lengths, tr, T=None, S=2):
    """the plugin's collated batch: time-major blocks per modality, one-hot speakers, zero padding"""
    B, T, N = len(lengths), T or max(lengths), sum(lengths)
    mask = (torch.arange(T)[:, None] < torch.tensor(lengths)[None, :]).float()[..., None]
    b = {k: None for k in KEYS.values()}
    for m in tr.model.order:
        b[KEYS[m]] = torch.randn(T, B, DIMS[m]) * mask
    b.update(speaker_tensor=torch.nn.functional.one_hot(torch.randint(0, S, (T, B)), S).float() * mask,
             text_length=torch.tensor(lengths, dtype=torch.int64), label=torch.randint(0, 6, (N, )))
    return b


def _store(tr, rows=10, dtype=torch.float32, widths=None):
    widths = widths or DIMS
    return types.SimpleNamespace(feats={m: torch.ones(rows, widths[m], dtype=dtype) for m in tr.model.order},
                                 speaker=torch.zeros(rows, dtype=torch.int64), label=torch.zeros(rows, dtype=torch.int64))


def test_the_flag_is_off_by_default_and_resident_implies_it():
    from track_mm.mmgcn import MMGCNParams
    assert MMGCNParams().capacity_buckets is False
    off = _trainer(extra=())
    off.t_cap = 40
    assert off.capacity is False and off.capacity_bucket(_batch([5, 7, 9], off)) is None
    assert off.all_capacity_buckets(_batch([5, 7, 9], off)) == []
    assert off.resident_batch(_store(off), torch.zeros(8, dtype=torch.int32), 4, 40, 128) is None
    assert _trainer().capacity is True
    assert _trainer(extra=("--resident", "--device_collate")).capacity is True


def test_bucket_keys_round_the_node_count_up_to_128():
    from erc_amd.mmgcn import MMGCNTrainer
    assert MMGCNTrainer.N_BUCKET == 128 and MMGCNTrainer.TIME_MAJOR is True
    tr = _trainer(batch_size=4)
    tr.t_cap = 40
    key = lambda lens, **k: tr.capacity_bucket(_batch(lens, tr, **k))[0]
    assert key([17, 1, 33]) == ("capacity", 4, 40, 128)
    assert key([1]) == ("capacity", 4, 40, 128)
    assert key([40, 40, 40, 9]) == ("capacity", 4, 40, 160)           # 129 -> 256, clipped to B_cap * T_cap
    assert key([32, 32, 32, 32]) == ("capacity", 4, 40, 128)          # a full node count in a longer T_cap still pads
    # a batch larger than train.batch_size or longer than t_cap widens its own bucket
    assert key([3] * 6, T=50) == ("capacity", 6, 50, 128)
    # a batch of exactly its bucket's shape has nothing to pad: the exact-shape path
    assert tr.capacity_bucket(_batch([40, 40, 40, 40], tr)) is None


def test_make_and_fill_are_time_major_and_empty_slots_get_length_zero():
    tr = _trainer(batch_size=5)
    tr.t_cap = 10
    big, small = _batch([9, 8, 10, 7, 6], tr), _batch([3, 4, 2], tr)
    key, make, fill = tr.capacity_bucket(big)
    assert key == ("capacity", 5, 10, 50)
    static = make()
    for m in "atv":
        assert static[KEYS[m]].shape == (10, 5, DIMS[m]) and static[KEYS[m]].dtype == torch.float32
    assert static["speaker_tensor"].shape == (10, 5, 2) and static["label"].shape == (50, )
    assert static["text_length"].shape == (5, ) and static["text_length"].dtype == torch.int64
    fill(static, big)
    assert static["extent"] == [10, 5, 40]
    fill(static, small)
    assert static["text_length"].tolist() == [3, 4, 2, 0, 0]
    n = int(small["label"].shape[0])
    assert torch.equal(static["label"][:n], small["label"]) and int(static["label"][n:].abs().sum()) == 0
    for k in list(KEYS.values()) + ["speaker_tensor"]:
        assert torch.equal(static[k][:4, :3], small[k]), k            # [T, B, .]: time first
        rest = static[k].clone()
        rest[:4, :3] = 0
        assert float(rest.abs().sum()) == 0.0, k                      # nothing of the big batch is left
    fill(static, big)                                                 # and back: the big batch in full
    assert torch.equal(static["audio_feature"], big["audio_feature"]) and static["text_length"].tolist() == [9, 8, 10, 7, 6]


@pytest.mark.parametrize("modality", ["atv", "av"])
def test_fill_after_any_sequence_of_batches_equals_a_fresh_buffer(modality):
    from tests.util_capacity import FILL_SEQ, assert_fill_equals_a_fresh_buffer
    tr = _trainer(batch_size=4, modality=modality)
    tr.t_cap = 12
    batches = [_batch(lens, tr) for lens in FILL_SEQ]
    assert_fill_equals_a_fresh_buffer(tr, batches, "audio_feature")
    assert (tr.capacity_bucket(batches[0])[1]()["text_feature"] is None) == (modality == "av")


def test_a_two_modality_bucket_holds_only_its_modalities():
    tr = _trainer(batch_size=4, modality="av")
    tr.t_cap = 12
    b = _batch([5, 12, 1], tr)
    key, make, fill = tr.capacity_bucket(b)
    static = make()
    assert key == ("capacity", 4, 12, 48) and static["text_feature"] is None
    assert static["audio_feature"].shape == (12, 4, 100) and static["visual_feature"].shape == (12, 4, 512)
    fill(static, b)
    assert static["text_length"].tolist() == [5, 12, 1, 0]


def test_the_three_refusals_of_the_gate(monkeypatch):
    tr = _trainer(batch_size=4)
    tr.t_cap = 40
    ok = _batch([17, 1, 33], tr)
    assert tr.capacity_bucket(ok) is not None and tr._capacity_ok(4, 40, 128)
    # 1. the chain form is off: by the environment, or beyond its T
    monkeypatch.setenv("ERC_MM_CHAIN", "0")
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == [] and not tr._capacity_ok(4, 40, 128)
    monkeypatch.delenv("ERC_MM_CHAIN")
    assert tr._capacity_ok(4, 128, 128) and not tr._capacity_ok(4, 129, 128)
    tr.t_cap = 129
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    tr.t_cap = 40
    # 2. the peer-to-peer exchange is on
    monkeypatch.setenv("ERC_DP_P2P", "1")
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    monkeypatch.delenv("ERC_DP_P2P")
    tr.model.flat.p2p = object()
    assert tr.capacity_bucket(ok) is None
    assert tr.resident_batch(_store(tr), torch.zeros(8, dtype=torch.int32), 4, 40, 128) is None
    del tr.model.flat.p2p
    assert tr.capacity_bucket(ok) is not None
    # 3. erc_gcnii_chain_config finds no residency for B_cap * Mo parts (here: a device with fewer CUs than one dialogue needs);
    #    the device is asked once per (B_cap, T_cap) and trainer, so each answer gets a trainer of its own
    def refuse(B, T, Mo, P):
        raise capi.ErcGraftError("gcnii_chain_config: a dialogue does not fit the device")
    asked = []
    for answer in (refuse, lambda B, T, Mo, P: (3, 4, 0)):      # (the second: a grid cap below one launch's share)
        monkeypatch.setattr(capi, "gcnii_chain_config", lambda *a, _f=answer: asked.append(a) or _f(*a))
        no = _trainer(batch_size=4)
        no.t_cap = 40
        assert no.capacity_bucket(ok) is None and no.all_capacity_buckets(ok) == [] and no.capacity_bucket(ok) is None
        assert no.resident_batch(_store(no), torch.zeros(8, dtype=torch.int32), 4, 40, 128) is None
    assert asked == [(4, 40, 3, 40)] * 2
    monkeypatch.setattr(capi, "gcnii_chain_config", _chain_config_256)
    assert tr.capacity_bucket(ok) is not None
    # and what every trainer's gate has: N_cap within the padded block, the plugin's dtypes, a class count rows_score takes
    assert not tr._capacity_ok(4, 40, 161) and not tr._capacity_ok(4, 40, 0)
    assert tr.capacity_bucket(dict(ok, text_length=ok["text_length"].to(torch.int32))) is None
    assert tr.capacity_bucket(dict(ok, audio_feature=ok["audio_feature"].double())) is None
    tr.model.n_classes = capi.rows_score_max_classes() + 1
    assert tr.capacity_bucket(ok) is None
    tr.model.n_classes = 6


def test_precapture_list_and_its_order():
    tr = _trainer(batch_size=4)
    tr.t_cap = 100
    buckets = tr.all_capacity_buckets(_batch([5, 9, 20], tr))        # (the probe's own shape does not enter)
    assert [b[0] for b in buckets] == [("capacity", 4, 100, n) for n in (128, 256, 384, 400)]
    assert tr._precapture_caps(None) == (4, 100, [128, 256, 384, 400])
    for (key, make, fill, synth), n in zip(buckets, (128, 256, 384, 400)):
        static = make()
        synth(static)
        lens = static["text_length"].tolist()
        assert sum(lens) == n and min(lens) > 0 and max(lens) <= 100 and static["label"].shape == (n, )
    tr.t_cap = 20                                                    # B_cap * T_cap below one N_BUCKET: the clipped bucket alone
    assert [b[0] for b in tr.all_capacity_buckets(_batch([5], tr))] == [("capacity", 4, 20, 80)]


def test_stepgraphs_replays_the_mmgcn_buckets():
    from erc_amd.trainer import StepGraphs
    tr = _trainer(batch_size=4)
    tr.t_cap = 60
    calls = []
    tr.train_step = lambda batch: calls.append((int(batch["label"].shape[0]), tuple(batch["audio_feature"].shape[:2]),
                                                tr.model.dynamic_n)) or torch.zeros(4)

    class Graphs(StepGraphs):
        def _capture(self, fn):
            fn()
            return types.SimpleNamespace(replay=lambda: calls.append("replay")), torch.zeros(4)

        def _sync(self):
            pass

    g = Graphs(tr)
    for lens in ([10, 20, 30, 4], [3, 4], [60, 60, 9, 1], [1]):
        g.step(tr.prepare_batch(_batch(lens, tr)))
    assert calls == [(128, (60, 4), True), (128, (60, 4), True), "replay", (240, (60, 4), True), (240, (60, 4), True), "replay"]
    assert (g.captures, g.replays, g.eager) == (2, 2, 2)
    assert list(g.cache) == [("capacity", 4, 60, 240), ("capacity", 4, 60, 128)] and tr.model.dynamic_n is False


def test_resident_batch_and_resident_eval_batch_conditions():
    tr = _trainer(batch_size=4)
    desc = torch.zeros(8, dtype=torch.int32)
    store = _store(tr)
    a, b = tr.resident_batch(store, desc, 4, 40, 128), tr.resident_eval_batch(store, desc, 4, 40, 128)
    assert a is not None and b is not None and set(a) == set(b)
    assert a["caps"] == b["caps"] == (4, 40, 128) and a["desc"] is desc and a["text_length"] is None
    assert a["label"] is store.label and a["speaker_tensor"] is store.speaker
    # each modality's features are handed over with one zero row appended, cached per store
    for m in "atv":
        x = a[KEYS[m]]
        assert x.shape == (11, DIMS[m]) and torch.equal(x[:10], store.feats[m]) and float(x[10].abs().sum()) == 0.0
        assert b[KEYS[m]] is x and tr.resident_batch(store, desc, 4, 40, 256 - 96)[KEYS[m]] is x
    other = _store(tr)
    assert tr.resident_batch(other, desc, 4, 40, 128)["audio_feature"] is not a["audio_feature"]
    assert tr.resident_batch(store, desc, 4, 40, 128)["audio_feature"] is a["audio_feature"]      # both stores stay cached
    # None when it must: another dtype, another width, a missing modality, beyond the gate
    assert tr.resident_batch(_store(tr, dtype=torch.bfloat16), desc, 4, 40, 128) is None
    assert tr.resident_eval_batch(_store(tr, dtype=torch.bfloat16), desc, 4, 40, 128) is None
    assert tr.resident_batch(_store(tr, widths=dict(DIMS, v=100)), desc, 4, 40, 128) is None
    short = _store(tr)
    del short.feats["t"]
    assert tr.resident_batch(short, desc, 4, 40, 128) is None
    assert tr.resident_batch(store, desc, 4, 129, 128) is None
    assert tr.resident_batch(store, desc, 4, 40, 161) is None
    av = _trainer(batch_size=4, modality="av", extra=("--resident", "--device_collate"))
    got = av.resident_batch(_store(av), desc, 4, 40, 128)
    assert got["text_feature"] is None and got["visual_feature"].shape == (11, 512)


def test_a_resident_step_and_eval_scores_refuse_before_any_launch():
    tr = _trainer(batch_size=4)
    b = tr.resident_batch(_store(tr), torch.zeros(8, dtype=torch.int32), 4, 40, 128)
    with pytest.raises(capi.ErcGraftError, match="capacity mode"):
        tr.model.loss_and_grads(b)                           # outside dynamic_n
    tr.model.n_classes = 17
    with pytest.raises(capi.ErcGraftError, match="at most 16 classes"):
        tr.model.eval_scores(b, torch.zeros(17, 17, dtype=torch.int64))


def _patched_run(monkeypatch, argv):
    """(the pattern of test_dgcn_resident_eval_host._patched_run: the run believes a GPU is there; every StepGraphs,
    ResidentEpochs and ResidentEval it builds is recorded)"""
    from erc_amd import trainer as trainer_mod
    from erc_amd.mmgcn import MMGCNTrainer
    from track_mm.mmgcn import MMGCNParams
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "manual_seed_all", lambda s: None)
    built = []
    for cls in (trainer_mod.StepGraphs, trainer_mod.ResidentEpochs, trainer_mod.ResidentEval):
        def init(self, *a, _orig=cls.__init__, **k):
            _orig(self, *a, **k)
            built.append(self)
        monkeypatch.setattr(cls, "__init__", init)
    return trainer_mod.run(MMGCNTrainer, MMGCNParams, argv), built


ARGV = BASE + ["--epoch=0", "--n_train=12", "--n_test=5", "--train.batch_size=4", "--test.batch_size=3", "--device_collate"]


def test_run_builds_stepgraphs_resident_epochs_and_resident_eval_for_an_unmodified_trainer(monkeypatch):
    from erc_amd.mmgcn import MMGCNTrainer
    from erc_amd.trainer import ResidentEpochs, ResidentEval, StepGraphs
    out, built = _patched_run(monkeypatch, ARGV + ["--resident", "--resident_eval"])
    assert out == {} and [type(b) for b in built] == [StepGraphs, ResidentEpochs, ResidentEval]
    graphs, res, ev = built
    assert isinstance(res.trainer, MMGCNTrainer) and res.trainer is graphs.trainer and res.trainer.capacity
    assert res.trainer.t_cap == int(res.store.lengths.max())
    assert res.supported() and ev.supported()
    assert res.N_BUCKET == ev.N_BUCKET == 128 and res.B == 4 and ev.B == 3 and ev.steps == 2
    assert ev.T == int(ev.store.lengths.max()) and all(c % 128 == 0 or c == ev.B * ev.T for c in ev.caps)
    assert ev.cm.shape == (6, 6) and ev.cm.dtype == torch.int64


def test_without_the_flags_the_run_builds_the_exact_shape_graphs_alone(monkeypatch):
    from erc_amd.trainer import StepGraphs
    out, built = _patched_run(monkeypatch, ARGV)
    assert out == {} and [type(b) for b in built] == [StepGraphs] and built[0].trainer.capacity is False
    with pytest.raises(SystemExit, match="--resident_eval needs --resident"):
        _patched_run(monkeypatch, ARGV + ["--resident_eval"])
    with pytest.raises(SystemExit, match="--resident needs --device_collate"):
        _patched_run(monkeypatch, [a for a in ARGV if a != "--device_collate"] + ["--resident"])
    # a split whose longest dialogue is beyond the chain's T: refused before the first epoch, not in the middle of one
    with pytest.raises(SystemExit, match="capacity mode"):
        _patched_run(monkeypatch, ARGV + ["--resident", "--syn_min_len=129", "--syn_max_len=130"])
