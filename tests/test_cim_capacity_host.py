"""CPU: CIM's capacity buckets (CIMTrainer.capacity_bucket / all_capacity_buckets / resident_batch / resident_eval_batch) --
the bucket keys, the batch-first static buffers with their zero row and, on CMU-MOSEI, emo_label and its tail clearing, every
refusal of the gates -- and ``--resident`` / ``--resident_eval`` reaching an unmodified CIMTrainer through ``trainer.run``.
The HIP runtime is replaced by recorders that do not execute what they record: there is no GPU here.  Last, the index
arithmetic of erc_cim_meta_cap (csrc/cim_meta.h, the functions the kernel calls) as a host program under the address and
undefined-behaviour sanitizers."""
import os
import shutil
import subprocess
import types

import pytest
import torch

from erc_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = dict(a="audio_feature", t="text_feature", v="visual_feature")
DIMS = {"iemocap-cogmen-6": dict(a=100, t=100, v=512), "mosei-cim-2": dict(a=74, t=300, v=35)}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.delenv("ERC_DP_P2P", raising=False)


def _trainer(dataset="iemocap-cogmen-6", batch_size=4, extra=("--capacity_buckets=True", )):
    from erc_amd.cim import CIMTrainer
    from track_mm.cim import CIMParams
    p = CIMParams().from_args(["--dataset=" + dataset, "--device=cpu", "--train.batch_size=%d" % batch_size] + list(extra))
    return CIMTrainer(p, "cpu")


def _batch(lengths, tr, T=None):
    """the plugin's collated batch: batch-first blocks per modality, speaker ids, zero padding"""
    B, T, N = len(lengths), T or max(lengths), sum(lengths)
    mask = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).float()[..., None]
    b = {KEYS[m]: torch.randn(B, T, d) * mask for m, d in tr.model.dims.items()}
    b.update(speaker_tensor=torch.zeros(B, T, dtype=torch.int64), text_length=torch.tensor(lengths, dtype=torch.int64),
             label=torch.randint(0, tr.model.n_classes, (N, )))
    if tr.multitask:
        b["emo_label"] = 1 + torch.randint(0, 2, (N, 7))      # (1 or 2: never 0, so that a cleared row shows)
        b["senti2_label"] = b["label"].clone()
    return b


def _store(tr, rows=10, dtype=torch.float32, widths=None, emo=True):
    widths = widths or tr.model.dims
    extra = {"emo_label": torch.ones(rows, 7, dtype=torch.int64)} if tr.multitask and emo else {}
    return types.SimpleNamespace(feats={m: torch.ones(rows, widths[m], dtype=dtype) for m in "atv"}, extra=extra,
                                 speaker=torch.zeros(rows, dtype=torch.int64), label=torch.zeros(rows, dtype=torch.int64))


DESC = torch.zeros(8, dtype=torch.int32)


def test_the_flag_is_off_by_default_and_resident_implies_it():
    from erc_amd.cim import CIMTrainer
    from erc_amd.capacity import CapacityBuckets, ResidentEvalSteps
    from track_mm.cim import CIMParams
    assert CIMParams().capacity_buckets is False and issubclass(CIMTrainer, (CapacityBuckets, ResidentEvalSteps))
    off = _trainer(extra=())
    off.t_cap = 40
    assert off.capacity is False and off.capacity_bucket(_batch([5, 7, 9], off)) is None
    assert off.all_capacity_buckets(_batch([5, 7, 9], off)) == []
    assert off.resident_batch(_store(off), DESC, 4, 40, 128) is None and off.model.dynamic_n is False
    assert _trainer().capacity is True
    assert _trainer(extra=("--resident", "--device_collate")).capacity is True


def test_bucket_keys_round_the_node_count_up_to_128():
    from erc_amd.cim import CIMTrainer
    assert (CIMTrainer.N_BUCKET, CIMTrainer.TIME_MAJOR, CIMTrainer.CLEAR_STALE) == (128, False, False)
    tr = _trainer()
    tr.t_cap = 40
    assert tr._feature_keys() == ("audio_feature", "visual_feature", "text_feature")
    key = lambda lens, **k: tr.capacity_bucket(_batch(lens, tr, **k))[0]
    assert key([17, 1, 33]) == ("capacity", 4, 40, 128)
    assert key([1]) == ("capacity", 4, 40, 128)
    assert key([40, 40, 40, 9]) == ("capacity", 4, 40, 160)           # 129 -> 256, clipped to B_cap * T_cap
    assert key([32, 32, 32, 32]) == ("capacity", 4, 40, 128)          # a full node count in a longer T_cap still pads
    assert key([3] * 6, T=50) == ("capacity", 6, 50, 128)             # a larger / longer batch widens its own bucket
    assert tr.capacity_bucket(_batch([40, 40, 40, 40], tr)) is None   # exactly its bucket's shape: nothing to pad
    assert tr._precapture_caps(None) == (4, 40, [128, 160])
    assert [b[0] for b in tr.all_capacity_buckets(_batch([5], tr))] == [("capacity", 4, 40, 128), ("capacity", 4, 40, 160)]


@pytest.mark.parametrize("dataset", list(DIMS))
def test_make_and_fill_are_batch_first_with_a_zero_row_and_emo_label(dataset):
    tr = _trainer(dataset, batch_size=5)
    tr.t_cap = 10
    dims, multi = DIMS[dataset], dataset.startswith("mosei")
    assert tr.multitask is multi and tr.model.dims == dims
    big, small = _batch([9, 8, 10, 7, 6], tr), _batch([3, 4, 2], tr)
    key, make, fill = tr.capacity_bucket(small)
    assert key == ("capacity", 5, 10, 50) and tr.capacity_bucket(big)[0] == key
    static = make()
    assert static["tail_row"] == 50 and static["label"].shape == (50, ) and static["text_length"].dtype == torch.int64
    assert ("emo_label" in static) is multi
    for m in "atv":
        x = static[KEYS[m]]
        assert x.shape == (5, 10, dims[m]) and x.dtype == torch.float32 and x.is_contiguous()
        assert x.untyped_storage().nbytes() == 51 * dims[m] * 4           # the block and ONE more row behind it
    fill(static, big)
    fill(static, small)
    assert static["text_length"].tolist() == [3, 4, 2, 0, 0]
    n = int(small["label"].shape[0])
    assert torch.equal(static["label"][:n], small["label"])
    for m in "atv":
        assert torch.equal(static[KEYS[m]][:3, :4], small[KEYS[m]])       # [B, T, .]: dialogue first
        assert torch.equal(static[KEYS[m]][3:], big[KEYS[m]][3:])         # CLEAR_STALE is off: the big batch's rows stay
        flat = torch.empty(0).set_(static[KEYS[m]].untyped_storage()).view(51, dims[m])
        assert float(flat[50].abs().sum()) == 0.0                          # no fill reaches the zero row
    if multi:
        assert static["emo_label"].shape == (50, 7) and static["emo_label"].dtype == torch.int64
        assert torch.equal(static["emo_label"][:n], small["emo_label"])
        assert int(static["emo_label"][n:].abs().sum()) == 0 and static["emo_rows"] == n      # the big batch's 40 rows: cleared
        fill(static, big)
        assert torch.equal(static["emo_label"][:40], big["emo_label"]) and int(static["emo_label"][40:].abs().sum()) == 0


def test_every_refusal_of_the_capacity_gate(monkeypatch):
    tr = _trainer()
    tr.t_cap = 40
    ok = _batch([17, 1, 33], tr)
    assert tr.capacity_bucket(ok) is not None and tr._capacity_ok(4, 40, 128)
    # the peer-to-peer exchange
    monkeypatch.setenv("ERC_DP_P2P", "1")
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    monkeypatch.delenv("ERC_DP_P2P")
    tr.model.flat.p2p = object()
    assert tr.capacity_bucket(ok) is None and tr.resident_batch(_store(tr), DESC, 4, 40, 128) is None
    del tr.model.flat.p2p
    # supports_capacity: T_cap beyond the attention's LDS, more slots than the prefix kernel takes, a class count beyond rows_score
    T = capi.cim_max_t()
    assert T == 118 and tr._capacity_ok(4, T, 128) and not tr._capacity_ok(4, T + 1, 128)
    assert tr._capacity_ok(1024, 40, 128) and not tr._capacity_ok(1025, 40, 128)
    tr.t_cap = T + 1
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    tr.t_cap = 40
    tr.model.n_classes = capi.rows_score_max_classes() + 1
    assert tr.capacity_bucket(ok) is None
    tr.model.n_classes = 6
    # N_cap within the padded block
    assert not tr._capacity_ok(4, 40, 161) and not tr._capacity_ok(4, 40, 0)
    # the plugin's dtypes, ranks and widths; all three modalities
    assert tr.capacity_bucket(dict(ok, text_length=ok["text_length"].to(torch.int32))) is None
    assert tr.capacity_bucket(dict(ok, audio_feature=ok["audio_feature"].double())) is None
    assert tr.capacity_bucket(dict(ok, visual_feature=ok["visual_feature"][..., :100].contiguous())) is None
    assert tr.capacity_bucket(dict(ok, text_feature=None)) is None
    assert tr.capacity_bucket(dict(ok, speaker_tensor=None)) is None
    assert tr.capacity_bucket(ok) is not None
    # CMU-MOSEI: the multi-task loss needs emo_label [N, 7] int64
    mo = _trainer("mosei-cim-2")
    mo.t_cap = 40
    good = _batch([17, 1, 33], mo)
    assert mo.capacity_bucket(good) is not None
    assert mo.capacity_bucket({k: v for k, v in good.items() if k != "emo_label"}) is None
    assert mo.capacity_bucket(dict(good, emo_label=good["emo_label"].float())) is None
    assert mo.capacity_bucket(dict(good, emo_label=good["emo_label"][:, :6])) is None


def test_resident_batch_and_every_refusal_of_the_resident_gate():
    tr = _trainer(extra=("--resident", "--device_collate"))
    store = _store(tr)
    a, b = tr.resident_batch(store, DESC, 4, 40, 128), tr.resident_eval_batch(store, DESC, 4, 40, 128)
    assert a is not None and b is not None and set(a) == set(b) and "emo_label" not in a
    assert a["caps"] == (4, 40, 128) and a["desc"] is DESC and a["text_length"] is None and a["label"] is store.label
    for m in "atv":                       # each modality's store with one zero row appended, cached per store
        x = a[KEYS[m]]
        assert x.shape == (11, tr.model.dims[m]) and torch.equal(x[:10], store.feats[m]) and float(x[10].abs().sum()) == 0.0
        assert b[KEYS[m]] is x and tr.resident_batch(store, DESC, 4, 40, 160)[KEYS[m]] is x
    assert tr.resident_batch(_store(tr), DESC, 4, 40, 128)["audio_feature"] is not a["audio_feature"]
    # None when it must: another dtype, another width, a missing modality, beyond the capacity gate
    assert tr.resident_batch(_store(tr, dtype=torch.bfloat16), DESC, 4, 40, 128) is None
    assert tr.resident_eval_batch(_store(tr, dtype=torch.bfloat16), DESC, 4, 40, 128) is None
    assert tr.resident_batch(_store(tr, widths=dict(tr.model.dims, v=100)), DESC, 4, 40, 128) is None
    short = _store(tr)
    del short.feats["t"]
    assert tr.resident_batch(short, DESC, 4, 40, 128) is None
    assert tr.resident_batch(store, DESC, 4, 119, 128) is None and tr.resident_batch(store, DESC, 4, 40, 161) is None
    # CMU-MOSEI: emo_label comes from the store's extras; a store without them cannot run the multi-task step
    mo = _trainer("mosei-cim-2", extra=("--resident", "--device_collate"))
    ms = _store(mo)
    got = mo.resident_batch(ms, DESC, 4, 40, 128)
    assert got["emo_label"] is ms.extra["emo_label"] and got["text_feature"].shape == (11, 300)
    assert mo.resident_batch(_store(mo, emo=False), DESC, 4, 40, 128) is None
    single = _trainer("mosei-cim-2", extra=("--resident", "--device_collate", "--apply_multi=False"))
    assert "emo_label" not in single.resident_batch(_store(single, emo=False), DESC, 4, 40, 128)


def test_a_resident_step_and_eval_scores_refuse_before_any_launch():
    tr = _trainer()
    b = tr.resident_batch(_store(tr), DESC, 4, 40, 128)
    with pytest.raises(capi.ErcGraftError, match="capacity mode"):
        tr.model.loss_and_grads(b)                           # outside dynamic_n
    tr.model.n_classes = 17
    with pytest.raises(capi.ErcGraftError, match="at most 16 classes"):
        tr.model.eval_scores(b, torch.zeros(17, 17, dtype=torch.int64))
    tr.model.n_classes = 6
    with pytest.raises(capi.ErcGraftError, match="up to 118 utterances"):
        tr.model.eval_scores(dict(b, caps=(4, 119, 128)), torch.zeros(6, 6, dtype=torch.int64))


def test_stepgraphs_replays_the_cim_buckets():
    from erc_amd.trainer import StepGraphs
    tr = _trainer("mosei-cim-2")
    tr.t_cap = 60
    calls = []
    tr.train_step = lambda batch: calls.append((int(batch["label"].shape[0]), tuple(batch["audio_feature"].shape[:2]),
                                                tuple(batch["emo_label"].shape), tr.model.dynamic_n)) or torch.zeros(4)

    class Graphs(StepGraphs):
        def _capture(self, fn):
            fn()
            return types.SimpleNamespace(replay=lambda: calls.append("replay")), torch.zeros(4)

        def _sync(self):
            pass

    g = Graphs(tr)
    for lens in ([10, 20, 30, 4], [3, 4], [60, 60, 9, 1], [1]):
        g.step(tr.prepare_batch(_batch(lens, tr)))
    small, large = (128, (4, 60), (128, 7), True), (240, (4, 60), (240, 7), True)
    assert calls == [small, small, "replay", large, large, "replay"]
    assert (g.captures, g.replays, g.eager) == (2, 2, 2) and tr.model.dynamic_n is False


def _patched_run(monkeypatch, argv):
    """(the pattern of test_mmgcn_capacity_host._patched_run: the run believes a GPU is there; every StepGraphs,
    ResidentEpochs and ResidentEval it builds is recorded)"""
    from erc_amd import trainer as trainer_mod
    from erc_amd.cim import CIMTrainer
    from track_mm.cim import CIMParams
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "manual_seed_all", lambda s: None)
    built = []
    for cls in (trainer_mod.StepGraphs, trainer_mod.ResidentEpochs, trainer_mod.ResidentEval):
        def init(self, *a, _orig=cls.__init__, **k):
            _orig(self, *a, **k)
            built.append(self)
        monkeypatch.setattr(cls, "__init__", init)
    return trainer_mod.run(CIMTrainer, CIMParams, argv), built


ARGV = ["--device=cpu", "--epoch=0", "--n_train=12", "--n_test=5", "--train.batch_size=4", "--test.batch_size=3", "--device_collate"]


def test_run_builds_stepgraphs_resident_epochs_and_resident_eval_for_an_unmodified_trainer(monkeypatch):
    from erc_amd.cim import CIMTrainer
    from erc_amd.trainer import ResidentEpochs, ResidentEval, StepGraphs
    out, built = _patched_run(monkeypatch, ["--dataset=iemocap-cogmen-6"] + ARGV + ["--resident", "--resident_eval"])
    assert out == {} and [type(b) for b in built] == [StepGraphs, ResidentEpochs, ResidentEval]
    graphs, res, ev = built
    assert type(res.trainer) is CIMTrainer and res.trainer is graphs.trainer and res.trainer.capacity
    assert res.trainer.t_cap == int(res.store.lengths.max())
    assert res.supported() and ev.supported()
    assert res.N_BUCKET == ev.N_BUCKET == 128 and res.B == 4 and ev.B == 3 and ev.steps == 2
    assert ev.T == int(ev.store.lengths.max()) and all(c % 128 == 0 or c == ev.B * ev.T for c in ev.caps)
    assert ev.cm.shape == (6, 6) and ev.cm.dtype == torch.int64


def test_on_mosei_resident_trains_from_hbm_and_resident_eval_stays_refused(monkeypatch):
    from erc_amd.trainer import ResidentEpochs, StepGraphs
    mosei = ["--dataset=mosei-cim-2"] + ARGV
    out, built = _patched_run(monkeypatch, mosei + ["--resident"])
    assert out == {} and [type(b) for b in built] == [StepGraphs, ResidentEpochs]
    res = built[1]
    assert res.trainer.multitask and res.supported()
    assert res._batch(128)["emo_label"] is res.store.extra["emo_label"]
    with pytest.raises(SystemExit, match="mosei_metric=multiemo reports multi-label metrics"):
        _patched_run(monkeypatch, mosei + ["--resident", "--resident_eval"])


def test_without_the_flags_the_run_builds_the_exact_shape_graphs_alone(monkeypatch):
    from erc_amd.trainer import StepGraphs
    iemocap = ["--dataset=iemocap-cogmen-6"] + ARGV
    out, built = _patched_run(monkeypatch, iemocap)
    assert out == {} and [type(b) for b in built] == [StepGraphs] and built[0].trainer.capacity is False
    with pytest.raises(SystemExit, match="--resident_eval needs --resident"):
        _patched_run(monkeypatch, iemocap + ["--resident_eval"])
    with pytest.raises(SystemExit, match="--resident needs --device_collate"):
        _patched_run(monkeypatch, [a for a in iemocap if a != "--device_collate"] + ["--resident"])
    # a split whose longest dialogue is beyond the attention's T: refused before the first epoch, not in the middle of one
    with pytest.raises(SystemExit, match="capacity mode"):
        _patched_run(monkeypatch, iemocap + ["--resident", "--syn_min_len=119", "--syn_max_len=120"])


def test_meta_arithmetic_under_the_address_and_undefined_sanitizers(tmp_path):
    """csrc/cim_meta.h holds the prefix sum and the row map of erc_cim_meta_cap as plain functions the kernel calls;
    tests/host/cim_meta_check.cpp runs them on the host over exactly sized heap buffers (410 cases: the GPU tests' shapes, every
    clamp, descriptor rows outside the store) and compares with a restatement"""
    # a host compiler is always there: without g++ / clang++ on the path, the clang++ next to the hipcc that builds the library
    hipcc = os.path.realpath(os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc")
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++, %s): the host memory check cannot run" % rocm_clang
    exe = str(tmp_path / "cim_meta_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", capi.CSRC, os.path.join(REPO, "tests", "host", "cim_meta_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.startswith("ok 410"), (res.stdout[-500:], res.stderr[-2000:])
