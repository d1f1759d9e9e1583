"""CPU: tools/epoch_bench.py -- its presets parse with every plugin's own params class, its parent starts one child at a time
under a time limit and stops at the first failure, and its summary of the epoch times is the hand-computed one.  No child
runs here: there is no GPU."""
import importlib
import importlib.util
import json
import os
import types
from pkgutil import iter_modules

import pytest

import track_mm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("epoch_bench", os.path.join(REPO, "tools", "epoch_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


EB = _tool()
PLUGINS = sorted(m.name for m in iter_modules(track_mm.__path__))
CASES = [(m, c, mode) for m, (_, configs) in sorted(EB.PRESETS.items()) for c in configs for mode in EB.MODES
         if not EB.skipped(m, c, mode)]


def test_every_plugin_has_a_preset_and_resolves_to_trainer_and_params():
    assert sorted(EB.PRESETS) == PLUGINS
    for module in EB.PRESETS:
        trainer_cls, params_cls = EB.plugin(module)
        assert callable(getattr(trainer_cls, "train_step", None)) and hasattr(params_cls(), "from_args")
        assert (trainer_cls, params_cls) == importlib.import_module("track_mm." + module).main.args


@pytest.mark.parametrize("module,config,mode", CASES, ids=["-".join(c) for c in CASES])
def test_preset_parses_with_the_modules_own_params(module, config, mode):
    _, params_cls = EB.plugin(module)
    argv = EB.flags(module, config, mode)
    p = params_cls().from_args(argv + ["--device=cpu", "--epoch=3", "--log_every=0"])
    assert isinstance(p.dims(), dict) and all(int(v) > 0 for v in p.dims().values())        # a dataset params.dims() knows
    assert p.dataset == [f for f in argv if f.startswith("--dataset=")][-1].split("=", 1)[1]
    assert int(p.train.batch_size) == int(p.test.batch_size) == EB.PRESETS[module][0]
    assert (int(p.n_train), int(p.n_test)) in ((120, 31), (1039, 280), (2240, 672), (1024, 64))
    for flag in EB.MODES[mode]:
        key, _, value = flag[2:].partition("=")
        assert p.get(key) == {"": True, "True": True, "False": False}[value], flag


def test_skipped_cells_and_overrides():
    assert EB.skipped("cim", "mosei", "resident_eval") and not EB.skipped("cim", "iemocap", "resident_eval")
    assert EB.skipped("bcgru", "meld", "resident_eval") and EB.skipped("bclstm", "iemocap", "resident_eval")
    assert not EB.skipped("bcgru", "meld", "resident")
    assert EB.skipped("mmin_miss", "f50_400", "resident") and not EB.skipped("mmin_base", "f50_400", "resident")
    assert EB.skipped("mmin_miss", "f100_100", "exact") and EB.skipped("mmin_base", "f100_100", "exact")
    argv = EB.flags("bcgru", "iemocap", "default", sets=["n_train=10", "train.batch_size=4", "syn_min_len=1"], collate_on_device=True)
    assert argv.count("--n_train=10") == 1 and "--n_train=120" not in argv and "--n_test=31" in argv
    assert "--train.batch_size=4" in argv and "--train.batch_size=32" not in argv and "--test.batch_size=32" in argv
    assert "--syn_min_len=1" in argv and argv.count("--device_collate") == 1
    assert EB.flags("bcgru", "iemocap", "resident", collate_on_device=True).count("--device_collate") == 1


class _Recorder:
    """stands in for subprocess.run: records every argv, starts nothing, hands out the given exit statuses"""

    def __init__(self, statuses):
        self.statuses, self.calls = list(statuses), []

    def __call__(self, cmd, **kwargs):
        self.calls.append(list(cmd))
        rc = self.statuses.pop(0)
        mode = [a for a in cmd if a.startswith("--modes=")][0].split("=", 1)[1]
        rec = {"tool": "epoch_bench", "mode": mode, "train_ms_median": 2.0, "test_ms_median": 1.0, "epoch_ms_median": 3.0}
        return types.SimpleNamespace(returncode=rc, stdout=json.dumps(rec) + "\n" if rc == 0 else "")


def _lines(capsys):
    return [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]


def test_the_parent_stops_at_the_first_child_that_fails(monkeypatch, capsys):
    rec = _Recorder([0, 134, 0])
    monkeypatch.setattr(EB.subprocess, "run", rec)
    with pytest.raises(SystemExit) as exc:
        EB.main(["--module=bcgru", "--config=iemocap", "--modes=default,buckets,resident", "--timeout=77"])
    assert exc.value.code == 134
    assert len(rec.calls) == 2                                   # the third child is never started
    for cmd, mode in zip(rec.calls, ("default", "buckets")):
        assert cmd[:4] == ["timeout", "-k", "10", "77"] and cmd[5].endswith(os.path.join("tools", "epoch_bench.py"))
        assert "--child" in cmd and "--module=bcgru" in cmd and "--config=iemocap" in cmd and "--modes=" + mode in cmd
    lines = _lines(capsys)
    errors = [l for l in lines if "error" in l]
    assert len(errors) == 1 and errors[0] == {"tool": "epoch_bench", "module": "bcgru", "config": "iemocap", "mode": "buckets",
                                              "error": "exit status 134"}
    assert lines[-1] is errors[0] and len(lines) == 2           # one result line, one error line, no ratio line


def test_a_repeated_modes_list_starts_one_child_per_entry_and_ends_with_ratio_lines(monkeypatch, capsys):
    rec = _Recorder([0] * 4)
    monkeypatch.setattr(EB.subprocess, "run", rec)
    EB.main(["--module=dgcn", "--config=meld", "--modes=resident,resident_eval,resident,resident_eval", "--set", "n_train=64"])
    assert [[a for a in cmd if a.startswith("--modes=")] for cmd in rec.calls] == \
        [["--modes=resident"], ["--modes=resident_eval"]] * 2
    assert all("--set=n_train=64" in cmd for cmd in rec.calls)
    lines = _lines(capsys)
    assert len(lines) == 5 and lines[-1] == {"tool": "epoch_bench", "module": "dgcn", "config": "meld",
                                             "modes": ["resident", "resident_eval"], "train_ms_ratio": 1.0, "test_ms_ratio": 1.0,
                                             "epoch_ms_ratio": 1.0}


def test_skipped_modes_start_no_child(monkeypatch, capsys):
    rec = _Recorder([0] * 2)
    monkeypatch.setattr(EB.subprocess, "run", rec)
    EB.main(["--module=cim", "--config=mosei", "--modes=resident,resident_eval", "--steps"])
    assert [[a for a in cmd if a.startswith("--modes=")][0] for cmd in rec.calls] == ["--modes=resident", "--modes=steps"]
    rec = _Recorder([0])
    monkeypatch.setattr(EB.subprocess, "run", rec)
    EB.main(["--module=mmin_miss", "--config=f50_400", "--modes=default,resident", "--steps"])
    assert [[a for a in cmd if a.startswith("--modes=")][0] for cmd in rec.calls] == ["--modes=default"]


def test_the_summary_is_the_hand_computed_one():
    train = [50.0, 4.0, 2.0, 9.0, 3.0]
    epoch = [80.0, 5.0, 4.0, 12.0, 7.0]
    counts = [[0, 3, 3], [3, 0, 0], [3, 0, 0], [2, 1, 1], [3, 0, 0]]
    s = EB.summarise(train, epoch, counts, EB.warmup_of("default", 1))
    assert s["warmup_epochs"] == 1 and s["epochs_timed"] == 4
    assert s["train_ms"] == [4.0, 2.0, 9.0, 3.0] and (s["train_ms_median"], s["train_ms_min"], s["train_ms_max"]) == (3.5, 2.0, 9.0)
    assert s["epoch_ms"] == [5.0, 4.0, 12.0, 7.0] and (s["epoch_ms_median"], s["epoch_ms_min"], s["epoch_ms_max"]) == (6.0, 4.0, 12.0)
    assert s["test_ms"] == [1.0, 2.0, 3.0, 4.0] and s["test_ms_median"] == 2.5
    assert s["replay_share_timed"] == round(11 / 12, 3)
    assert s["replays_by_epoch"] == [0, 3, 3, 2, 3] and s["eager_steps_by_epoch"] == [3, 0, 0, 1, 0]
    assert s["captures_by_epoch"] == [3, 0, 0, 1, 0]
    # ``exact`` drops one more epoch (a shape is captured on its second visit); a warm-up of 0 still drops the first
    assert EB.warmup_of("exact", 1) == 2 and EB.warmup_of("exact", 0) == 2 and EB.warmup_of("resident", 0) == 1
    s = EB.summarise(train, epoch, counts, EB.warmup_of("exact", 1))
    assert s["warmup_epochs"] == 2 and s["epochs_timed"] == 3
    assert s["train_ms"] == [2.0, 9.0, 3.0] and s["train_ms_median"] == 3.0
    assert s["epoch_ms_median"] == 7.0 and s["test_ms_median"] == 3.0 and s["replay_share_timed"] == round(8 / 9, 3)
    assert s["replays_by_epoch"] == [0, 3, 3, 2, 3]              # the counters keep every epoch
