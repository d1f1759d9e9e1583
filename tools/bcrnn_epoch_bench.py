#!/usr/bin/env python3
"""bc-LSTM / bc-GRU (--module=bclstm, --module=bcgru) over whole reshuffled training epochs, as train_mm.py runs them:

  eager     --graph_capture=False: every step launched from Python, exact batch shapes
  default   no flag: StepGraphs keyed by the exact batch shape (a shape is captured when it shows up the second time; under
            reshuffling almost none does)
  bucketed  --capacity_buckets=True: capacity buckets, one captured HIP graph per bucket, every later batch a replay
  resident  --device_collate --resident: dialogues in HBM, a step's input is 2 B int32, one copy + one replay per step

Two configurations at B = 32: synthetic IEMOCAP-6 (120 dialogues of 20 .. 110 utterances, class-weighted loss) and a
MELD-sized set (1039 dialogues of 1 .. 33 utterances, --loss_weights=False) that is long enough for a steady state.  Every
mode runs in a fresh process; train_mm.py times an epoch between device synchronisations.  One JSON line per (cell, config,
mode): utterances/s per epoch and the mean over the epochs after the first (the first pays one eager step + capture per
bucket), steps per epoch, and the run's replay / capture / eager-step counts.  The first run that fails or runs into
--timeout ends the tool with a non-zero exit code: no further process is started on the GPU after it.

    python tools/bcrnn_epoch_bench.py [--epochs 4] [--cells gru,lstm] [--configs iemocap,meld] [--modes eager,default,bucketed,resident]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    "iemocap": ["--dataset=iemocap-cogmen-6", "--n_train=120"],
    "meld": ["--dataset=meld-mmgcn-7", "--modality=atv", "--loss_weights=False", "--n_train=1039"],
}
CONFIG_N = {"iemocap": 120, "meld": 1039}
MODES = {"eager": ["--graph_capture=False"], "default": [], "bucketed": ["--capacity_buckets=True"],
         "resident": ["--device_collate", "--resident"]}


def run(cell, config, mode, epochs, batch, timeout):
    args = [sys.executable, os.path.join(REPO, "train_mm.py"), "--module=bc" + cell, "--epoch=%d" % epochs, "--n_test=4",
            "--train.batch_size=%d" % batch, "--test.batch_size=%d" % batch] + CONFIGS[config] + MODES[mode]
    head = {"tool": "bcrnn_epoch_bench", "cell": cell, "config": config, "mode": mode, "batch": batch}
    res = subprocess.run(args, cwd=REPO, capture_output=True, text=True, timeout=timeout)      # a timeout ends the whole tool
    if res.returncode != 0:
        return dict(head, error=res.stderr[-600:], returncode=res.returncode)
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    ep = [l for l in lines if "train_utt_per_s" in l]
    later = [l["train_utt_per_s"] for l in ep[1:]] or [ep[-1]["train_utt_per_s"]]
    return dict(head, epochs=len(ep), steps_per_epoch=-(-CONFIG_N[config] // batch),
                utt_per_s_per_epoch=[round(l["train_utt_per_s"], 1) for l in ep],
                utt_per_s_mean_after_first=round(sum(later) / len(later), 1),
                graph_replays=ep[-1]["graph_replays"], graphs_captured=ep[-1]["graphs_captured"], eager_steps=ep[-1]["eager_steps"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--cells", default="gru,lstm")
    ap.add_argument("--configs", default="iemocap,meld")
    ap.add_argument("--modes", default="eager,default,bucketed,resident")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per run")
    a = ap.parse_args()
    for cell in a.cells.split(","):
        for config in a.configs.split(","):
            for mode in a.modes.split(","):
                rec = run(cell, config, mode, a.epochs, a.batch, a.timeout)
                print(json.dumps(rec), flush=True)
                if "error" in rec:
                    # a run that failed (abort, fault, refusal) may have left the card in a bad state: nothing more is
                    # started on it by this tool
                    raise SystemExit("bcrnn_epoch_bench: %s / %s / %s exited with %d; stopping"
                                     % (cell, config, mode, rec["returncode"]))


if __name__ == "__main__":
    main()
