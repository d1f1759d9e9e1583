#!/usr/bin/env python3
"""DialogueGCN (--module=dgcn) over whole reshuffled training epochs, as train_mm.py runs them, in three modes:

  eager     --graph_capture=False: every step launched from Python (capacity buckets' static buffers, no replay)
  bucketed  the default: capacity buckets, one captured HIP graph per bucket, every later batch of the bucket a replay
  resident  --device_collate --resident: dialogues in HBM, a step's input is 2 B int32, one copy + one replay per step

Two configurations at B = 32: the MELD-shaped 7-way atv bf16 config (BASELINE.json configs[4]) and IEMOCAP-6 f32 (two
speakers; --relation_space=False runs the basis-space path capacity mode covers).  Every mode runs in a fresh process;
train_mm.py times an epoch between device synchronisations.  One JSON line per (config, mode): utterances/s of the last
epoch and the mean over the epochs after the first (the first pays one eager step + capture per bucket), steps per epoch,
and the run's replay / capture / eager-step counts.

    python tools/dgcn_epoch_bench.py [--epochs 4] [--configs meld,iemocap] [--modes eager,bucketed,resident]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    "meld": ["--dataset=meld-mmgcn-7", "--modality=atv", "--compute=bf16", "--loss_weights=False", "--n_train=1039"],
    "iemocap": ["--dataset=iemocap-cogmen-6", "--compute=f32", "--relation_space=False", "--n_train=120"],
}
MODES = {"eager": ["--graph_capture=False"], "bucketed": [], "resident": ["--device_collate", "--resident"]}


def run(config, mode, epochs, batch, timeout):
    args = [sys.executable, os.path.join(REPO, "train_mm.py"), "--module=dgcn", "--epoch=%d" % epochs, "--n_test=4",
            "--train.batch_size=%d" % batch, "--test.batch_size=%d" % batch] + CONFIGS[config] + MODES[mode]
    res = subprocess.run(args, cwd=REPO, capture_output=True, text=True, timeout=timeout)
    if res.returncode != 0:
        return {"config": config, "mode": mode, "error": res.stderr[-600:]}
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    ep = [l for l in lines if "train_utt_per_s" in l]
    steps = [l for l in lines if "Lall" in l and "step" in l]
    later = [l["train_utt_per_s"] for l in ep[1:]] or [ep[-1]["train_utt_per_s"]]
    return {"tool": "dgcn_epoch_bench", "config": config, "mode": mode, "batch": batch, "epochs": len(ep),
            "steps_per_epoch": (len(steps) // len(ep)) if steps else -(-CONFIG_N[config] // batch),
            "utt_per_s_last_epoch": round(ep[-1]["train_utt_per_s"], 1), "utt_per_s_mean_after_first": round(sum(later) / len(later), 1),
            "utt_per_s_per_epoch": [round(l["train_utt_per_s"], 1) for l in ep],
            "graph_replays": ep[-1]["graph_replays"], "graphs_captured": ep[-1]["graphs_captured"], "eager_steps": ep[-1]["eager_steps"]}


CONFIG_N = {"meld": 1039, "iemocap": 120}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--configs", default="meld,iemocap")
    ap.add_argument("--modes", default="eager,bucketed,resident")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per run")
    a = ap.parse_args()
    for config in a.configs.split(","):
        for mode in a.modes.split(","):
            print(json.dumps(run(config, mode, a.epochs, a.batch, a.timeout)), flush=True)


if __name__ == "__main__":
    main()
