"""CPU: DialogueGCN's capacity buckets (DGCNTrainer.capacity_bucket / all_capacity_buckets / resident_batch) -- keys and
rounding, the paths that stay exact-shape, the static buffers' fill, the data-parallel precapture order -- and
``--resident`` reaching a DialogueGCN trainer."""
import types

import pytest
import torch

from erc_amd import capi


def _trainer(batch_size=8, dataset="meld-mmgcn-7", extra=()):
    from erc_amd.dgcn import DGCNTrainer
    from erc_amd.params import ERCParams
    p = ERCParams().from_args(["--dataset=" + dataset, "--loss_weights=False", "--device=cpu",
                               "--train.batch_size=%d" % batch_size] + list(extra))
    tr = DGCNTrainer(p, "cpu")
    tr.model.relation_space = False
    return tr


def _batch(lengths, T=None, D=4, dtype=torch.float32):
    B, T = len(lengths), T or max(lengths)
    N = sum(lengths)
    return dict(input_tensor=torch.randn(B, T, D).to(dtype), speaker_tensor=torch.randint(0, 9, (B, T)),
                text_length=torch.tensor(lengths, dtype=torch.int64), label=torch.randint(0, 7, (N, )))


def test_bucket_keys_round_n_up_to_the_bucket_edge():
    tr = _trainer(batch_size=8)
    tr.t_cap = 40
    assert tr.N_BUCKET == 128
    assert tr.capacity_bucket(_batch([5, 7, 9]))[0] == ("capacity", 8, 40, 128)
    assert tr.capacity_bucket(_batch([40, 40, 40, 9]))[0] == ("capacity", 8, 40, 256)          # N = 129
    assert tr.capacity_bucket(_batch([30] * 8))[0] == ("capacity", 8, 40, 256)
    # a batch larger than train.batch_size or longer than t_cap widens its own bucket
    assert tr.capacity_bucket(_batch([3] * 10, T=50))[0] == ("capacity", 10, 50, 128)
    # the rounded count never exceeds the B_cap x T_cap block
    tr.t_cap = 12
    assert tr.capacity_bucket(_batch([12] * 7 + [11]))[0] == ("capacity", 8, 12, 96)


def test_a_batch_of_its_buckets_shape_stays_exact():
    tr = _trainer(batch_size=4)
    tr.t_cap = 12
    assert tr.capacity_bucket(_batch([12] * 4)) is None                 # B, T, N == B_cap, T_cap, N_cap = 48
    assert tr.capacity_bucket(_batch([12] * 3 + [11]))[0] == ("capacity", 4, 12, 48)


def test_no_bucket_above_the_tail_limit_on_other_paths_and_with_p2p(monkeypatch):
    tr = _trainer(batch_size=32)
    tr.t_cap = 300
    max_rows = capi.dgcn_tail_limits()[0]
    assert max_rows == 8192
    assert tr.capacity_bucket(_batch([256] * 32)) is not None           # N = 8192
    assert tr.capacity_bucket(_batch([256] * 31 + [257])) is None       # N = 8193 -> 8320 rows
    ok = _batch([20] * 8)
    for attr, val in (("relation_space", True), ("compact_lstm", False), ("fused_rgcn_fwd", False), ("fused_tail", False),
                      ("fused_edge_bwd", False)):
        old = getattr(tr.model, attr)
        setattr(tr.model, attr, val)
        assert tr.capacity_bucket(ok) is None, attr
        assert tr.all_capacity_buckets(ok) == [], attr
        setattr(tr.model, attr, old)
    assert tr.capacity_bucket(ok) is not None
    assert tr.capacity_bucket(dict(ok, input_tensor=ok["input_tensor"].to(torch.bfloat16))) is None   # f32 model, bf16 data
    monkeypatch.setenv("ERC_DP_P2P", "1")
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    monkeypatch.delenv("ERC_DP_P2P")
    tr.model.flat.p2p = object()
    assert tr.capacity_bucket(ok) is None
    store = types.SimpleNamespace(fused=torch.zeros(10, tr.model.input_size), speaker=torch.zeros(10, dtype=torch.int64),
                                  label=torch.zeros(10, dtype=torch.int64))
    assert tr.resident_batch(store, torch.zeros(64, dtype=torch.int32), 32, 300, 128) is None
    del tr.model.flat.p2p
    assert tr.resident_batch(store, torch.zeros(64, dtype=torch.int32), 32, 300, 128)["caps"] == (32, 300, 128)
    assert tr.resident_batch(store, torch.zeros(64, dtype=torch.int32), 32, 300, 8320) is None


def test_resident_batch_needs_the_models_feature_dtype():
    tr = _trainer(extra=["--compute=bf16"])
    desc = torch.zeros(16, dtype=torch.int32)
    mk = lambda dt: types.SimpleNamespace(fused=torch.zeros(10, tr.model.input_size, dtype=dt),
                                          speaker=torch.zeros(10, dtype=torch.int64), label=torch.zeros(10, dtype=torch.int64))
    assert tr.resident_batch(mk(torch.float32), desc, 8, 20, 128) is None
    b = tr.resident_batch(mk(torch.bfloat16), desc, 8, 20, 128)
    assert b["desc"] is desc and b["text_length"] is None and b["caps"] == (8, 20, 128)


def test_fill_zeroes_missing_dialogues_and_copies_labels():
    tr = _trainer(batch_size=5)
    tr.t_cap = 10
    big, small = _batch([9, 8, 10, 7, 6]), _batch([3, 4, 2])
    key, make, fill = tr.capacity_bucket(big)
    static = make()
    assert static["input_tensor"].shape == (5, 10, 4) and static["label"].shape == (key[3], )
    fill(static, big)
    fill(static, small)
    assert static["text_length"].tolist() == [3, 4, 2, 0, 0]
    n = int(small["label"].shape[0])
    assert torch.equal(static["label"][:n], small["label"])
    assert torch.equal(static["input_tensor"][:3, :4], small["input_tensor"])
    assert torch.equal(static["speaker_tensor"][:3, :4], small["speaker_tensor"])


def test_all_capacity_buckets_smallest_first_with_synthetic_lengths():
    tr = _trainer(batch_size=8)
    tr.t_cap = 33
    buckets = tr.all_capacity_buckets(_batch([5, 9, 33]))
    caps = [key[3] for key, _, _, _ in buckets]
    assert caps == sorted(caps) and caps[0] == 128 and caps[-1] == 8 * 33 and len(set(caps)) == len(caps)
    assert all(c % 128 == 0 for c in caps[:-1])
    for key, make, fill, synth in buckets:
        assert key[:3] == ("capacity", 8, 33)
        static = make()
        synth(static)
        lens = static["text_length"]
        assert int(lens.sum()) == key[3] and int(lens.max()) <= 33 and int(lens.min()) >= 0


def test_stepgraphs_precaptures_dgcn_buckets_in_order():
    """trainer.StepGraphs under data parallelism with DialogueGCN's buckets: every bucket is warmed up and captured up front,
    smallest first (the same order on every rank), and a later batch replays its bucket's graph; the HIP runtime is
    replaced by a recorder that does not execute what it records."""
    from erc_amd.trainer import StepGraphs
    tr = _trainer(batch_size=4)
    tr.t_cap = 80
    calls = []
    tr.train_step = lambda batch: calls.append(int(batch["label"].shape[0])) or torch.zeros(4)

    class Graphs(StepGraphs):
        def _capture(self, fn):
            return types.SimpleNamespace(replay=lambda: calls.append("replay")), torch.zeros(4)

        def _sync(self):
            pass

    g = Graphs(tr)
    probe = _batch([10, 20, 30, 40])
    g.precapture(probe)
    g.lazy = False
    want = [128, 256, 320]
    assert calls == want and [k[3] for k in g.cache] == want and g.captures == 3
    g.step(_batch([50, 60, 70, 80]))                  # N = 260 -> the 320-row bucket
    g.step(_batch([3, 4]))
    assert calls[3:] == ["replay", "replay"] and g.replays == 2 and g.eager == 0


def test_resident_flag_reaches_a_dgcn_trainer(monkeypatch):
    """``--module=dgcn --resident`` gets past the refusal that used to name COGMEN alone: the run builds its resident epochs
    (no epoch is trained here: there is no GPU)."""
    from erc_amd import trainer as trainer_mod
    from erc_amd.dgcn import DGCNTrainer
    from erc_amd.params import ERCParams
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "manual_seed_all", lambda s: None)
    built = []
    orig = trainer_mod.ResidentEpochs.__init__

    def init(self, *a, **k):
        orig(self, *a, **k)
        built.append(self)
    monkeypatch.setattr(trainer_mod.ResidentEpochs, "__init__", init)
    argv = ["--dataset=meld-mmgcn-7", "--loss_weights=False", "--device=cpu", "--epoch=0", "--n_train=12", "--n_test=4",
            "--train.batch_size=4", "--device_collate", "--resident"]
    assert trainer_mod.run(DGCNTrainer, ERCParams, argv) == {}
    assert len(built) == 1 and built[0].supported()


def test_a_bucket_carries_the_models_arguments_alone():
    """forward(**batch) runs on the static dict: no host-side bookkeeping key ("extent") may be in it"""
    tr = _trainer(batch_size=4)
    tr.t_cap = 12
    key, make, fill = tr.capacity_bucket(_batch([5, 9]))
    static = make()
    fill(static, _batch([5, 9]))
    fill(static, _batch([3]))
    assert set(static) == {"input_tensor", "speaker_tensor", "text_length", "label"}
