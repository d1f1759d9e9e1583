"""GPU: tools/epoch_bench.py end to end -- each test is one run of the tool as a subprocess, on the smallest shapes that still
have a smaller last batch, a one-utterance dialogue and more than one node capacity (the MMIN modules: more than one T capacity)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--config=iemocap", "--epochs=1", "--warmup=1", "--timeout=120", "--set", "n_train=10", "--set", "n_test=5",
         "--set", "train.batch_size=4", "--set", "test.batch_size=4", "--set", "syn_min_len=1", "--set", "syn_max_len=9"]


# the MMIN modules: 10 utterances of 5..140 audio frames in batches of 4 (a short last batch); T capacities are multiples of 64
# clipped to the split's longest utterance.  Seed 1 draws one capacity only (114 for every batch); seed 7 draws 64, 128 and the
# maximum, 131, in the first epoch and nothing new in the second (test_the_mmin_seed_draws_more_than_one_t_capacity)
MMIN_SEED = 7
MMIN_SMALL = ["--config=f50_400", "--epochs=1", "--warmup=1", "--timeout=120", "--set", "n_train=10", "--set", "n_val=5", "--set", "n_test=5",
              "--set", "train.batch_size=4", "--set", "val.batch_size=4", "--set", "test.batch_size=4", "--set", "mmin_frames=5,140",
              "--set", "seed=%d" % MMIN_SEED]


def _tool(args, small=SMALL):
    res = subprocess.run([sys.executable, os.path.join(REPO, "tools", "epoch_bench.py")] + args + small, cwd=REPO,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-1500:])
    return [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]


def test_bcgru_default_and_resident():
    """``launches_per_eager_step`` counts every C-ABI call of the step, as DESIGN.md states it ("a step is 22 C-ABI calls") and
    tools/bcrnn_bench.py counts it; 19 of them take a stream -- the nineteen launches DESIGN.md lists, batch tables ..
    ``erc_adam_step`` -- and three are host-side queries"""
    lines = _tool(["--module=bcgru", "--modes=default,resident"])
    results = {l["mode"]: l for l in lines if "train_ms_median" in l}
    assert len(lines) == 3 and sorted(results) == ["default", "resident"] and lines[-1]["modes"] == ["default", "resident"]
    for rec in results.values():
        assert rec["tool"] == "epoch_bench" and rec["module"] == "bcgru" and rec["config"] == "iemocap"
        assert rec["steps_per_epoch"] == 3 and rec["loss_finite"] is True and rec["epochs_timed"] == 1
    res = results["resident"]
    assert res["replays_by_epoch"][-1] == 3 and res["eager_steps_by_epoch"][-1] == 0 and res["captures_by_epoch"][-1] == 0
    assert res["replay_share_timed"] == 1.0                     # the timed epoch consists of replays only
    assert results["default"]["launches_per_eager_step"] == 22  # the bc-RNN step
    assert results["default"]["kernel_launches_per_eager_step"] == 19


def test_dialogrnn_resident_eval():
    lines = _tool(["--module=dialogrnn", "--modes=resident_eval"])
    assert len(lines) == 1
    rec = lines[0]
    assert rec["mode"] == "resident_eval" and rec["steps_per_epoch"] == 3 and rec["loss_finite"] is True
    assert rec["eval_captures_total"] >= 1 and rec["epoch_ms_median"] > rec["train_ms_median"]


def _mmin_train_caps(seed, epochs=2):
    """the T capacities of the first training epochs of the small MMIN split, as the resident loop draws them (host only)"""
    import torch
    from erc_amd.datasets import MMINDeviceStore, index_batches
    from erc_amd.synthetic import make_mmin_samples
    store = MMINDeviceStore(make_mmin_samples(10, "train", seed=seed, frames=(5, 140)), None)
    gen = torch.Generator().manual_seed(seed)
    return [store.table(index_batches(10, 4, True, gen), 4)[1] for _ in range(epochs)], store.t_max


def test_the_mmin_seed_draws_more_than_one_t_capacity():
    (first, second), t_max = _mmin_train_caps(MMIN_SEED)
    assert sorted(set(first)) == [64, 128, t_max] and t_max == 131      # a multiple of 64, another one, the clipped maximum
    assert set(second) <= set(first)                                     # the timed epoch meets no capacity for the first time
    assert len({c for caps in _mmin_train_caps(1)[0] for c in caps}) == 1


def test_mmin_base_default_and_resident_eval():
    """``kernel_launches_per_eager_step`` against this test's own count: one ``train_step`` of a fresh MMINBaseTrainer under
    ``capi.start_recording``, the calls for which ``capi._launches`` holds -- tools/mmin_bench.py's ``launching_calls_per_step``"""
    import torch
    from erc_amd import capi
    from erc_amd.mmin import MMINBaseTrainer, mmin_collate
    from erc_amd.synthetic import make_mmin_samples
    from track_mm.mmin_base import MMINBaseParams
    lines = _tool(["--module=mmin_base", "--modes=default,resident_eval"], MMIN_SMALL)
    results = {l["mode"]: l for l in lines if "train_ms_median" in l}
    assert len(lines) == 3 and sorted(results) == ["default", "resident_eval"] and lines[-1]["modes"] == ["default", "resident_eval"]
    for rec in results.values():
        assert rec["tool"] == "epoch_bench" and rec["module"] == "mmin_base" and rec["config"] == "f50_400"
        assert rec["steps_per_epoch"] == 3 and rec["loss_finite"] is True and rec["epochs_timed"] == 1
    res = results["resident_eval"]
    assert res["replay_share_timed"] == 1.0 and res["eager_steps_by_epoch"][-1] == 0
    assert res["eval_captures_total"] >= 2 and res["epoch_ms_median"] > res["train_ms_median"]
    # the training loop met the three T capacities the host replay of the draw finds (64, 128, 131), all in the first epoch
    assert res["captures_total"] - res["eval_captures_total"] == len(set(_mmin_train_caps(MMIN_SEED)[0][0])) == 3
    assert res["captures_by_epoch"] == [res["captures_total"], 0]
    tr = MMINBaseTrainer(MMINBaseParams().from_args(["--train.batch_size=4"]), "cuda:0")
    batch = tr.prepare_batch(mmin_collate(make_mmin_samples(4, "train", seed=MMIN_SEED, frames=(5, 140))))
    capi.start_recording()
    tr.train_step(batch)
    torch.cuda.synchronize()
    own = sum(1 for name, _ in capi.stop_recording() if capi._launches(name))
    print("mmin_base: launching calls of one eager step %d, the tool's %d of %d C-ABI calls"
          % (own, results["default"]["kernel_launches_per_eager_step"], results["default"]["launches_per_eager_step"]))
    assert own > 0 and results["default"]["kernel_launches_per_eager_step"] == own


def test_mmin_miss_runs_its_default_loop_and_starts_no_child_for_a_skipped_mode():
    lines = _tool(["--module=mmin_miss", "--modes=default,resident"], MMIN_SMALL)
    assert len(lines) == 1
    rec = lines[0]
    assert rec["module"] == "mmin_miss" and rec["mode"] == "default" and rec["steps_per_epoch"] == 3 and rec["loss_finite"] is True
