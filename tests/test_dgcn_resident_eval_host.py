"""CPU: the host side of ``--module=dgcn --resident --resident_eval`` -- ``trainer.run`` builds one ``ResidentEval`` over the
test store for the unmodified ``DGCNTrainer``, and ``DGCNTrainer.resident_eval_batch`` mirrors ``resident_batch`` (the same
dict, the same refusals).  No step runs here: there is no GPU."""
import types

import pytest
import torch

from erc_amd import capi

ARGV = ["--dataset=meld-mmgcn-7", "--loss_weights=False", "--device=cpu", "--epoch=0", "--n_train=12", "--n_test=4",
        "--train.batch_size=4", "--test.batch_size=3", "--device_collate"]


def _patched_run(monkeypatch, argv, cls, params_cls):
    """(the pattern of test_resident_eval_host._patched_run: the run believes a GPU is there, every ResidentEval it builds
    is recorded)"""
    from erc_amd import trainer as trainer_mod
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "manual_seed_all", lambda s: None)
    built = []
    orig = trainer_mod.ResidentEval.__init__

    def init(self, *a, **k):
        orig(self, *a, **k)
        built.append(self)
    monkeypatch.setattr(trainer_mod.ResidentEval, "__init__", init)
    return trainer_mod.run(cls, params_cls, argv), built


@pytest.mark.parametrize("extra", [[], ["--dataset=iemocap-cogmen-6", "--relation_space=False"]], ids=["meld-7", "iemocap-6"])
def test_the_flag_builds_one_resident_eval_for_a_dgcn_trainer(monkeypatch, extra):
    """MELD's nine speakers give 162 relations: basis space by itself; IEMOCAP's two would run in relation space, which has
    no capacity mode, hence --relation_space=False there (as for --resident)"""
    from erc_amd.dgcn import DGCNTrainer
    from track_mm.dgcn import DGCNParams
    assert hasattr(DGCNTrainer, "resident_eval_step") and hasattr(DGCNTrainer, "resident_eval_batch")
    out, built = _patched_run(monkeypatch, ARGV + extra + ["--resident", "--resident_eval"], DGCNTrainer, DGCNParams)
    assert out == {} and len(built) == 1
    ev = built[0]
    assert isinstance(ev.trainer, DGCNTrainer)
    assert len(ev.store) == 4 and ev.B == 3 and ev.steps == 2 and ev.supported()
    assert ev.T == int(ev.store.lengths.max())
    assert ev.cm.shape == (ev.trainer.params.n_classes, ) * 2 and ev.cm.dtype == torch.int64


def test_two_speakers_in_relation_space_are_refused_before_the_first_epoch(monkeypatch):
    """IEMOCAP without --relation_space=False: the run ends in _setup_resident (at --resident already: no capacity mode)"""
    from erc_amd.dgcn import DGCNTrainer
    from track_mm.dgcn import DGCNParams
    with pytest.raises(SystemExit) as exc:
        _patched_run(monkeypatch, ARGV + ["--dataset=iemocap-cogmen-6", "--resident", "--resident_eval"], DGCNTrainer, DGCNParams)
    assert "capacity mode" in str(exc.value)


def _trainer(extra=()):
    from erc_amd.dgcn import DGCNTrainer
    from erc_amd.params import ERCParams
    p = ERCParams().from_args(["--dataset=meld-mmgcn-7", "--loss_weights=False", "--device=cpu", "--train.batch_size=8"] + list(extra))
    tr = DGCNTrainer(p, "cpu")
    tr.model.relation_space = False
    return tr


def _store(tr, dtype=torch.float32):
    return types.SimpleNamespace(fused=torch.zeros(10, tr.model.input_size, dtype=dtype), speaker=torch.zeros(10, dtype=torch.int64),
                                 label=torch.zeros(10, dtype=torch.int64))


def test_resident_eval_batch_mirrors_resident_batch():
    tr = _trainer()
    store, desc = _store(tr), torch.zeros(16, dtype=torch.int32)
    max_rows = capi.dgcn_tail_limits()[0]
    for cap in (128, 256, max_rows):
        a, b = tr.resident_batch(store, desc, 8, 1100, cap), tr.resident_eval_batch(store, desc, 8, 1100, cap)
        assert a is not None and b is not None
        assert b["caps"] == a["caps"] == (8, 1100, cap)
        assert set(a) == set(b) and b["desc"] is desc and b["text_length"] is None
        assert b["input_tensor"] is store.fused and b["speaker_tensor"] is store.speaker and b["label"] is store.label
    # above the fused tail's row limit; in relation space; features of the wrong dtype
    assert tr.resident_eval_batch(store, desc, 8, 1100, max_rows + 128) is None
    assert tr.resident_eval_batch(_store(tr, torch.bfloat16), desc, 8, 1100, 128) is None
    tr.model.relation_space = True
    assert tr.resident_eval_batch(store, desc, 8, 1100, 128) is None and tr.resident_batch(store, desc, 8, 1100, 128) is None


def test_eval_scores_names_relation_space_as_the_reason():
    """(the refusal comes before any launch: it runs without a GPU)"""
    tr = _trainer()
    tr.model.relation_space = True
    store, desc = _store(tr), torch.zeros(16, dtype=torch.int32)
    b = dict(input_tensor=store.fused, speaker_tensor=store.speaker, text_length=None, label=store.label, desc=desc, caps=(8, 20, 128))
    with pytest.raises(capi.ErcGraftError, match="relation space.*--relation_space=False"):
        tr.model.eval_scores(b, torch.zeros(7, 7, dtype=torch.int64))
