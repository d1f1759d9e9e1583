"""CPU: the capacity buckets of DialogueRNN (DialogRNNTrainer.capacity_bucket / all_capacity_buckets / resident_batch /
resident_eval_batch) -- the opt-in flag, the bucket key and the time-major static buffers' fill, every leg of the gate, the
data-parallel precapture list -- and ``--resident`` / ``--resident_eval`` reaching a DialogRNNTrainer through ``trainer.run``.
No library is loaded: there is no GPU here."""
import types

import pytest
import torch

from erc_amd import capi
from erc_amd.capacity import bucket_sizes

D, S = 24, 2
BASE = ["--dataset=iemocap-cogmen-6", "--device=cpu"]


def _trainer(batch_size=32, extra=("--capacity_buckets=True", ), t_cap=110):
    from erc_amd.dialogrnn import DialogRNNTrainer
    from track_mm.dialogrnn import DialogRNNParams
    p = DialogRNNParams().from_args(BASE + ["--train.batch_size=%d" % batch_size] + list(extra))
    p.hidden_all = D
    tr = DialogRNNTrainer(p, "cpu")
    tr.t_cap = t_cap
    return tr


def _batch(lengths, T=None, dtype=torch.float32, seed=0, n_spk=S):
    """time-major, one-hot speakers, zero padding: the collate's layout for this model (batch_first=False)"""
    g = torch.Generator().manual_seed(seed + sum(lengths))
    B, T, N = len(lengths), T or max(lengths), sum(lengths)
    x = torch.randn(T, B, D, generator=g) + 3.0                  # no exact zeros among the valid rows
    spk = torch.nn.functional.one_hot(torch.randint(0, n_spk, (T, B), generator=g), n_spk).float()
    mask = (torch.arange(T)[:, None] < torch.tensor(lengths)[None, :])
    x, spk = x * mask[..., None], spk * mask[..., None]
    return dict(input_tensor=x.to(dtype), speaker_tensor=spk, text_length=torch.tensor(lengths, dtype=torch.int64),
                label=torch.randint(1, 6, (N, ), generator=g))


def _store(dtype=torch.float32, rows=10, width=D, spk_dtype=torch.int64):
    return types.SimpleNamespace(fused=torch.ones(rows, width, dtype=dtype), speaker=torch.zeros(rows, dtype=spk_dtype),
                                 label=torch.zeros(rows, dtype=torch.int64))


SMALL = [12, 40, 3, 25]           # T = 40, B = 4, N = 80


def test_buckets_are_off_without_the_flags():
    from track_mm.dialogrnn import DialogRNNParams
    assert DialogRNNParams().capacity_buckets is False
    tr = _trainer(extra=())
    assert tr.capacity is False and not tr.model.dynamic_n
    for lens in (SMALL, [110, 3, 3, 3, 3, 2, 2, 2], [1], [110] * 32):
        assert tr.capacity_bucket(_batch(lens)) is None and tr.all_capacity_buckets(_batch(lens)) == []
    assert tr.resident_batch(_store(), torch.zeros(64, dtype=torch.int32), 32, 110, 128) is None
    assert _trainer(extra=("--resident", "--device_collate")).capacity is True


def test_bucket_key_static_buffers_and_fill_of_a_time_major_batch():
    tr = _trainer()
    assert tr.N_BUCKET == 128 and tr.TIME_MAJOR and not tr.CLEAR_STALE
    small, big = _batch(SMALL), _batch([110, 3, 3, 3, 3, 2, 2, 2])
    key, make, fill = tr.capacity_bucket(small)
    assert key == ("capacity", 32, 110, 128) and tr.capacity_bucket(big)[0] == key
    static = make()
    assert static["input_tensor"].shape == (110, 32, D) and static["speaker_tensor"].shape == (110, 32, S)
    assert static["text_length"].shape == (32, ) and static["label"].shape == (128, )
    assert "extent" not in static                       # nothing reads a padded position: nothing is cleared
    fill(static, big)
    assert torch.equal(static["input_tensor"][:, :8], big["input_tensor"])
    fill(static, small)
    for k in ("input_tensor", "speaker_tensor"):
        assert torch.equal(static[k][:40, :4], small[k]), k
    assert static["text_length"].tolist() == SMALL + [0] * 28          # dialogues the batch does not have: length 0
    assert torch.equal(static["label"][:80], small["label"])
    # a batch larger than train.batch_size or longer than t_cap widens its own bucket; N is rounded up to 128
    assert tr.capacity_bucket(_batch([3] * 40))[0] == ("capacity", 40, 110, 128)
    assert tr.capacity_bucket(_batch([110, 19]))[0] == ("capacity", 32, 110, 256)          # N = 129


def test_a_batch_of_exactly_its_buckets_shape_gets_no_bucket():
    tr = _trainer(batch_size=4, t_cap=12)
    assert tr.capacity_bucket(_batch([12] * 4)) is None                 # B, T, N == B_cap, T_cap, N_cap = 48
    assert tr.capacity_bucket(_batch([12] * 3 + [11]))[0] == ("capacity", 4, 12, 48)


def test_every_leg_of_the_gate(monkeypatch):
    tr = _trainer(batch_size=4, t_cap=110)
    ok = _batch([20] * 3)
    assert tr.capacity_bucket(ok)[0] == ("capacity", 4, 110, 128)
    tr.t_cap = 111                                                      # the scans hold 110 utterances of history in LDS
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    tr.t_cap = 70
    assert tr.capacity_bucket(dict(ok, input_tensor=ok["input_tensor"].bfloat16())) is None
    assert tr.capacity_bucket(dict(ok, input_tensor=ok["input_tensor"].double())) is None
    assert tr.capacity_bucket(dict(ok, text_length=ok["text_length"].int())) is None
    assert tr.capacity_bucket(dict(ok, input_tensor=ok["input_tensor"][..., :D - 1])) is None     # another width
    assert tr.capacity_bucket(dict(ok, speaker_tensor=ok["speaker_tensor"].argmax(-1))) is None   # speaker ids, not one-hot
    assert tr.capacity_bucket(_batch([20] * 3, n_spk=10)) is None                                  # nine party states are built
    tr.model.n_classes = 9                                              # erc_head_ce_cap holds 8
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    tr.model.n_classes = 6
    tr.params.n_speakers = 10
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    tr.params.n_speakers = 2
    monkeypatch.setenv("ERC_DP_P2P", "1")
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    monkeypatch.delenv("ERC_DP_P2P")
    assert tr.capacity_bucket(ok) is not None


def test_precapture_list_depends_on_batch_size_and_t_cap_alone():
    tr = _trainer(batch_size=4, t_cap=70)
    buckets = tr.all_capacity_buckets(_batch([12, 67, 3]))
    assert [k for k, _, _, _ in buckets] == [("capacity", 4, 70, n) for n in bucket_sizes(128, 4 * 70)]
    assert [k[3] for k, _, _, _ in buckets] == [128, 256, 280]          # smallest first, the clipped top bucket included
    for key, make, fill, synth in buckets:
        static = make()
        synth(static)
        lens = static["text_length"]
        assert int(lens.sum()) == key[3] and int(lens.max()) <= 70 and int(lens.min()) >= 0
    for probe in (_batch([3] * 10, T=90), _batch([70] * 4), _batch([1]), None):
        assert [k for k, _, _, _ in tr.all_capacity_buckets(probe)] == [k for k, _, _, _ in buckets]
    tr = _trainer()                                                     # the reference's batch size and the scans' limit
    assert [k[3] for k, _, _, _ in tr.all_capacity_buckets(None)] == bucket_sizes(128, 32 * 110)


def test_the_trainer_has_the_resident_hooks_and_its_resident_batch():
    from erc_amd.dialogrnn import DialogRNNTrainer
    for hook in ("resident_batch", "resident_eval_batch", "resident_eval_step", "capacity_bucket", "all_capacity_buckets"):
        assert hasattr(DialogRNNTrainer, hook), hook
    tr = _trainer(batch_size=4)
    desc, store = torch.zeros(8, dtype=torch.int32), _store()
    a, b = tr.resident_batch(store, desc, 4, 70, 128), tr.resident_eval_batch(store, desc, 4, 70, 128)
    assert a is not None and b is not None and set(a) == set(b)
    assert set(a) == {"input_tensor", "speaker_tensor", "text_length", "label", "desc", "caps"}
    assert a["caps"] == (4, 70, 128) and a["desc"] is desc and a["text_length"] is None
    assert a["label"] is store.label and a["speaker_tensor"] is store.speaker          # the store's own speaker ids
    x = a["input_tensor"]                                                               # one zero row appended, once per store
    assert x.shape == (11, D) and torch.equal(x[:10], store.fused) and float(x[10].abs().sum()) == 0.0
    assert b["input_tensor"] is x and tr.resident_batch(store, desc, 4, 70, 256)["input_tensor"] is x
    assert tr.resident_batch(_store(torch.bfloat16), desc, 4, 70, 128) is None
    assert tr.resident_batch(_store(width=D + 1), desc, 4, 70, 128) is None
    assert tr.resident_batch(_store(spk_dtype=torch.int32), desc, 4, 70, 128) is None
    assert tr.resident_batch(store, desc, 4, 111, 128) is None
    assert tr.resident_eval_batch(store, desc, 4, 111, 128) is None
    assert tr.model.n_speakers == 2


def test_capacity_steps_are_refused_before_any_launch():
    """no library is built or loaded here: a refusal that came after a launch would fail with another error"""
    tr = _trainer(batch_size=4, t_cap=70)
    b = tr.resident_batch(_store(), torch.zeros(8, dtype=torch.int32), 4, 70, 128)
    with pytest.raises(capi.ErcGraftError, match="capacity mode needs dynamic_n"):
        tr.model.loss_and_grads(b, None)                      # a resident batch outside dynamic_n
    tr.model.dynamic_n = True
    try:
        tr.model.n_classes = 9
        with pytest.raises(capi.ErcGraftError, match="at most 8 classes"):
            tr.model.loss_and_grads(b, None)
        tr.model.n_classes = 6
        with pytest.raises(capi.ErcGraftError, match="T_cap=111"):
            tr.model.loss_and_grads(dict(b, caps=(4, 111, 128)), None)
        with pytest.raises(capi.ErcGraftError, match="int64 speaker ids"):
            tr.model.loss_and_grads(dict(b, speaker_tensor=b["speaker_tensor"].int()), None)
        static = tr.capacity_bucket(_batch([12, 67, 3]))[1]()
        with pytest.raises(capi.ErcGraftError, match="fp32 features of width"):
            tr.model.loss_and_grads(dict(static, input_tensor=static["input_tensor"].double()), None)
        with pytest.raises(capi.ErcGraftError, match="fp32 features of width"):
            tr.model.loss_and_grads(dict(static, input_tensor=static["input_tensor"][..., :D - 1]), None)
        with pytest.raises(capi.ErcGraftError, match="int64 text_length"):
            tr.model.loss_and_grads(dict(static, text_length=static["text_length"].int()), None)
        with pytest.raises(capi.ErcGraftError, match="dynamic_n"):
            tr.model(**_batch([12, 67, 3]))                    # the plain forward is not a capacity step
    finally:
        tr.model.dynamic_n = False


def _patched_run(monkeypatch, argv):
    """the run believes a GPU is there; every ResidentEpochs / ResidentEval it builds is recorded"""
    from erc_amd import trainer as trainer_mod
    from erc_amd.dialogrnn import DialogRNNTrainer
    from track_mm.dialogrnn import DialogRNNParams
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "manual_seed_all", lambda s: None)
    built = []
    for cls in (trainer_mod.ResidentEpochs, trainer_mod.ResidentEval):
        def init(self, *a, _orig=cls.__init__, **k):
            _orig(self, *a, **k)
            built.append(self)
        monkeypatch.setattr(cls, "__init__", init)
    return trainer_mod.run(DialogRNNTrainer, DialogRNNParams, argv), built


ARGV = BASE + ["--modality=a", "--epoch=0", "--n_train=12", "--n_test=5", "--train.batch_size=4", "--test.batch_size=3",
               "--device_collate"]


def test_resident_and_resident_eval_reach_a_dialogrnn_trainer(monkeypatch):
    from erc_amd.dialogrnn import DialogRNNTrainer
    from erc_amd.trainer import ResidentEpochs, ResidentEval
    out, built = _patched_run(monkeypatch, ARGV + ["--resident", "--resident_eval"])
    assert out == {} and [type(b) for b in built] == [ResidentEpochs, ResidentEval]
    res, ev = built
    assert type(res.trainer) is DialogRNNTrainer and res.trainer.capacity and res.supported() and ev.supported()
    assert res.N_BUCKET == ev.N_BUCKET == 128
    assert ev.cm.shape == (6, 6) and ev.cm.dtype == torch.int64


def test_without_the_flags_the_run_builds_neither(monkeypatch):
    out, built = _patched_run(monkeypatch, ARGV)
    assert out == {} and built == []
