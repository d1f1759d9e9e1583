"""CPU: the capacity buckets of bc-LSTM / bc-GRU (BcRnnTrainer.capacity_bucket / all_capacity_buckets / resident_batch) -- the
opt-in flag, keys and rounding, the time-major static buffers' fill, a reshuffled loop over a ragged loader under a recorder in
place of the HIP runtime, the data-parallel precapture order -- and ``--resident`` reaching these trainers."""
import types

import pytest
import torch

D_M = 12


def _trainer(cell="gru", batch_size=8, extra=("--capacity_buckets=True", )):
    from erc_amd.bcrnn import BcGruTrainer, BcLstmTrainer
    from track_mm.bclstm import BcRnnParams
    p = BcRnnParams().from_args(["--dataset=meld-mmgcn-7", "--loss_weights=False", "--device=cpu",
                                 "--train.batch_size=%d" % batch_size] + list(extra))
    p.hidden_all = D_M
    return (BcGruTrainer if cell == "gru" else BcLstmTrainer)(p, "cpu")


def _batch(lengths, T=None, D=D_M, S=9, dtype=torch.float32, seed=0):
    """time-major, one-hot speakers, zero padding: the collate's layout for these models (batch_first=False)"""
    g = torch.Generator().manual_seed(seed + sum(lengths))
    B, T = len(lengths), T or max(lengths)
    N = sum(lengths)
    x = torch.randn(T, B, D, generator=g) + 3.0                  # no exact zeros among the valid rows
    spk = torch.nn.functional.one_hot(torch.randint(0, S, (T, B), generator=g), S).float()
    mask = (torch.arange(T)[:, None] < torch.tensor(lengths)[None, :])
    x, spk = x * mask[..., None], spk * mask[..., None]
    return dict(input_tensor=x.to(dtype), speaker_tensor=spk, text_length=torch.tensor(lengths, dtype=torch.int64),
                label=torch.randint(1, 7, (N, ), generator=g))


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_buckets_are_off_by_default(cell):
    tr = _trainer(cell, extra=())
    tr.t_cap = 40
    b = _batch([5, 7, 9])
    assert tr.capacity is False
    assert tr.capacity_bucket(b) is None and tr.all_capacity_buckets(b) == []


def test_resident_implies_the_buckets():
    tr = _trainer(extra=("--resident", ))
    tr.t_cap = 40
    assert tr.capacity and tr.capacity_bucket(_batch([5, 7, 9]))[0] == ("capacity", 8, 40, 128)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_bucket_keys_round_n_up_to_the_bucket_edge(cell):
    tr = _trainer(cell, batch_size=8)
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


def test_no_bucket_above_the_attention_limit_with_other_dtypes_and_with_p2p(monkeypatch):
    tr = _trainer(batch_size=4)
    ok = _batch([20] * 3)
    tr.t_cap = 110
    assert tr.capacity_bucket(ok)[0] == ("capacity", 4, 110, 128)
    tr.t_cap = 111                                                      # erc_match_att_fwd holds 110 utterances
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    tr.t_cap = 40
    assert tr.capacity_bucket(dict(ok, input_tensor=ok["input_tensor"].double())) is None
    assert tr.capacity_bucket(dict(ok, text_length=ok["text_length"].int())) is None
    monkeypatch.setenv("ERC_DP_P2P", "1")
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    monkeypatch.delenv("ERC_DP_P2P")
    assert tr.capacity_bucket(ok) is not None


def test_fill_zeroes_missing_dialogues_and_leaves_nothing_of_the_previous_batch():
    tr = _trainer(batch_size=5)
    tr.t_cap = 10
    big, small = _batch([9, 8, 10, 7, 6]), _batch([3, 4, 2])
    key, make, fill = tr.capacity_bucket(big)
    static = make()
    assert static["input_tensor"].shape == (10, 5, D_M) and static["speaker_tensor"].shape == (10, 5, 9)      # time-major
    assert static["label"].shape == (key[3], )
    fill(static, big)
    assert torch.equal(static["input_tensor"], big["input_tensor"])
    fill(static, small)
    assert static["text_length"].tolist() == [3, 4, 2, 0, 0]
    n = int(small["label"].shape[0])
    assert torch.equal(static["label"][:n], small["label"]) and int(static["label"][n:].abs().sum()) == 0
    # the unpacked RNN reads EVERY padded row of every dialogue slot: what the new lengths do not cover must be zero
    for k in ("input_tensor", "speaker_tensor"):
        assert torch.equal(static[k][:4, :3], small[k])
        assert float(static[k][4:].abs().sum()) == 0 and float(static[k][:, 3:].abs().sum()) == 0
        for b, L in enumerate([3, 4, 2]):
            assert float(static[k][L:, b].abs().sum()) == 0
            assert float(static[k][:L, b].abs().sum()) > 0


def test_fill_after_any_sequence_of_batches_equals_a_fresh_buffer():
    """fill clears only what the previous batch occupied: after every batch of a sequence with growing and shrinking B, T
    and N the static buffers equal freshly zeroed ones with that batch copied in"""
    tr = _trainer(batch_size=6)
    tr.t_cap = 12
    seq = ([9, 8, 10, 7, 6], [3, 4, 2], [12] * 5 + [11], [1], [2, 11], [5, 5, 5, 5, 5, 5], [12, 1, 1, 1], [4, 4])
    key, make, fill = tr.capacity_bucket(_batch(seq[0]))
    static = make()
    for i, lens in enumerate(seq):
        b = _batch(lens, seed=i)
        assert tr.capacity_bucket(b)[0] == key
        fill(static, b)
        fresh = make()
        T, B = b["input_tensor"].shape[:2]
        for k in ("input_tensor", "speaker_tensor"):
            fresh[k][:T, :B] = b[k]
            assert torch.equal(static[k], fresh[k]), (i, k)
        assert static["text_length"].tolist() == lens + [0] * (6 - len(lens))
        n = sum(lens)
        assert torch.equal(static["label"][:n], b["label"]) and int(static["label"][n:].abs().sum()) == 0, i


def test_all_capacity_buckets_depend_on_batch_size_and_t_cap_alone():
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
    # another probe -- more dialogues than batch_size, longer than t_cap, one that fills its bucket -- gives the same list
    for probe in (_batch([3] * 10, T=50), _batch([33] * 8), _batch([1])):
        assert [k for k, _, _, _ in tr.all_capacity_buckets(probe)] == [k for k, _, _, _ in buckets]


class _Recorder:
    """StepGraphs with the two places that touch the HIP runtime replaced: a capture records and does not execute"""

    @staticmethod
    def make(tr, calls):
        from erc_amd.trainer import StepGraphs

        class Graphs(StepGraphs):
            def _capture(self, fn):
                return types.SimpleNamespace(replay=lambda: calls.append("replay")), torch.zeros(4)

            def _sync(self):
                pass
        return Graphs(tr)


def test_a_reshuffled_ragged_loop_replays_a_handful_of_buckets():
    tr = _trainer(batch_size=8)
    gen = torch.Generator().manual_seed(5)
    lengths = torch.randint(1, 41, (30, ), generator=gen).tolist() + [40]
    tr.t_cap = max(lengths)
    calls, seen_lengths = [], []

    def train_step(batch):
        assert tr.model.dynamic_n                              # a bucket's step runs in capacity mode
        calls.append(tuple(batch["input_tensor"].shape[:2]) + (int(batch["label"].shape[0]), ))
        seen_lengths.append(batch["text_length"].tolist())
        return torch.zeros(4)
    tr.train_step = train_step
    g = _Recorder.make(tr, calls)
    keys, steps = set(), 0
    for epoch in range(3):
        order = torch.randperm(len(lengths), generator=gen).tolist()
        for i in range(0, len(order), 8):
            lens = [lengths[j] for j in order[i:i + 8]]
            b = _batch(lens)
            bucket = tr.capacity_bucket(b)
            assert bucket is not None
            keys.add(bucket[0])
            g.step(b)
            steps += 1
            assert g.cache[bucket[0]].static["text_length"].tolist() == lens + [0] * (8 - len(lens))
    n_buckets = len(tr.all_capacity_buckets(_batch([3])))
    assert 1 < len(keys) <= n_buckets == 3                    # 8 x 40 = 320 rows: 128 | 256 | 320
    assert g.captures == len(keys) and g.eager == g.captures and g.replays == steps - g.captures
    assert calls.count("replay") == g.replays
    assert all(c == "replay" or c[:2] == (40, 8) for c in calls)          # every real step ran on the static buffers
    assert not tr.model.dynamic_n


def test_stepgraphs_precaptures_the_buckets_in_order():
    tr = _trainer("lstm", batch_size=4)
    tr.t_cap = 80
    calls = []
    tr.train_step = lambda batch: calls.append(int(batch["label"].shape[0])) or torch.zeros(4)
    g = _Recorder.make(tr, calls)
    g.precapture(_batch([10, 20, 30, 40]))
    g.lazy = False
    want = [128, 256, 320]
    assert calls == want and [k[3] for k in g.cache] == want and g.captures == 3
    g.step(_batch([50, 60, 70, 80]))                  # N = 260 -> the 320-row bucket
    g.step(_batch([3, 4]))
    assert calls[3:] == ["replay", "replay"] and g.replays == 2 and g.eager == 0


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_resident_batch_needs_an_fp32_store_of_the_models_width(cell):
    tr = _trainer(cell)
    desc = torch.zeros(16, dtype=torch.int32)
    mk = lambda dt, w=D_M: types.SimpleNamespace(fused=torch.ones(10, w, dtype=dt), speaker=torch.zeros(10, dtype=torch.int64),
                                                 label=torch.zeros(10, dtype=torch.int64))
    assert tr.resident_batch(mk(torch.bfloat16), desc, 8, 20, 128) is None
    assert tr.resident_batch(mk(torch.float32, D_M + 1), desc, 8, 20, 128) is None
    assert tr.resident_batch(mk(torch.float32), desc, 8, 111, 128) is None          # above the attention's limit
    store = mk(torch.float32)
    b = tr.resident_batch(store, desc, 8, 20, 128)
    assert b["desc"] is desc and b["text_length"] is None and b["caps"] == (8, 20, 128) and b["label"] is store.label
    # the features with the zero row that padded positions read, built once per store
    x = b["input_tensor"]
    assert x.shape == (11, D_M) and torch.equal(x[:10], store.fused) and float(x[10].abs().sum()) == 0
    assert tr.resident_batch(store, desc, 8, 20, 256)["input_tensor"] is x
    # with the flag off the trainer offers no resident batch either
    assert _trainer(cell, extra=()).resident_batch(store, desc, 8, 20, 128) is None


def _patched_run(monkeypatch, argv, cls):
    from erc_amd import trainer as trainer_mod
    from track_mm.bclstm import BcRnnParams
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "manual_seed_all", lambda s: None)
    built = []
    orig = trainer_mod.ResidentEpochs.__init__

    def init(self, *a, **k):
        orig(self, *a, **k)
        built.append(self)
    monkeypatch.setattr(trainer_mod.ResidentEpochs, "__init__", init)
    return trainer_mod.run(cls, BcRnnParams, argv), built


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_resident_flag_reaches_a_bcrnn_trainer(monkeypatch, cell):
    from erc_amd.bcrnn import BcGruTrainer, BcLstmTrainer
    argv = ["--dataset=meld-mmgcn-7", "--loss_weights=False", "--device=cpu", "--epoch=0", "--n_train=12", "--n_test=4",
            "--train.batch_size=4", "--device_collate", "--resident"]
    out, built = _patched_run(monkeypatch, argv, BcGruTrainer if cell == "gru" else BcLstmTrainer)
    assert out == {}
    assert len(built) == 1 and built[0].supported() and built[0].trainer.capacity


def test_resident_without_device_collate_still_exits_with_the_existing_message(monkeypatch):
    from erc_amd.bcrnn import BcGruTrainer
    argv = ["--dataset=meld-mmgcn-7", "--loss_weights=False", "--device=cpu", "--epoch=0", "--n_train=12", "--n_test=4",
            "--train.batch_size=4", "--resident"]
    with pytest.raises(SystemExit) as exc:
        _patched_run(monkeypatch, argv, BcGruTrainer)
    assert str(exc.value) == "--resident needs --device_collate, one rank and a trainer with resident batches (capacity mode)"


def test_resident_eval_with_bclstm_still_exits_with_the_existing_message(monkeypatch):
    """trainer.run asks hasattr(trainer, "resident_eval_step"): these trainers have no scored test step and must not get one
    from a shared base"""
    from erc_amd.bcrnn import BcGruTrainer, BcLstmTrainer
    assert not hasattr(BcLstmTrainer, "resident_eval_step") and not hasattr(BcGruTrainer, "resident_eval_step")
    argv = ["--dataset=meld-mmgcn-7", "--loss_weights=False", "--device=cpu", "--epoch=0", "--n_train=12", "--n_test=4",
            "--train.batch_size=4", "--device_collate", "--resident", "--resident_eval"]
    with pytest.raises(SystemExit) as exc:
        _patched_run(monkeypatch, argv, BcLstmTrainer)
    assert str(exc.value) == "--resident_eval: this module's trainer has no resident_eval_step (--module=cogmen has one)"
