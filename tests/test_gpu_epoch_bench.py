"""GPU: tools/epoch_bench.py end to end -- each test is one run of the tool as a subprocess, on the smallest shapes that still
have a smaller last batch, a one-utterance dialogue and more than one node capacity."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--config=iemocap", "--epochs=1", "--warmup=1", "--timeout=120", "--set", "n_train=10", "--set", "n_test=5",
         "--set", "train.batch_size=4", "--set", "test.batch_size=4", "--set", "syn_min_len=1", "--set", "syn_max_len=9"]


def _tool(args):
    res = subprocess.run([sys.executable, os.path.join(REPO, "tools", "epoch_bench.py")] + args + SMALL, cwd=REPO,
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
