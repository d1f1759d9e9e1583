#!/usr/bin/env python3
"""One bc-LSTM / bc-GRU training step, replayed --steps times as a captured HIP graph, in one of two forms:

  exact    the batch at its own shape (B, T, N), as train_mm.py runs it by default
  bucket   the same batch in its capacity bucket (B_cap = 32, T_cap = 110, N rounded up to 128): static buffers, the node
           count and the longest dialogue read from the device (--capacity_buckets=True)

on synthetic iemocap-cogmen-6 dialogues (D = 712) of 20 .. --t_max utterances, the longest exactly --t_max.  Prints one JSON
line: ms per step (median, min, max of the replays, device events), utterances, the shapes.  Meant to run under
``rocprofv3 --kernel-trace --stats`` (kernel time per step = a kernel's total over warm-up + replays, divided by their
number): bucket against exact shows what the capacity rows cost, --t_max 40 against 110 in bucket mode whether the scan
launches follow the device-side step count.

    python tools/bcrnn_capacity_steps.py --cell gru --mode bucket --t_max 40 [--batch 32] [--steps 20]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", default="gru")
    ap.add_argument("--mode", default="bucket", choices=("exact", "bucket"))
    ap.add_argument("--t_max", type=int, default=110)
    ap.add_argument("--t_cap", type=int, default=110)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bcrnn_capacity_steps.py times the step on the GPU: no device found")
    from erc_amd.collate import ERCCollate
    from erc_amd.engine import GraphedStep
    from erc_amd.synthetic import make_dialogues
    plugin = importlib.import_module("track_mm.bc" + a.cell)
    extra = ["--capacity_buckets=True"] if a.mode == "bucket" else []
    params = plugin.ParamsType().from_args(["--dataset=iemocap-cogmen-6", "--train.batch_size=%d" % a.batch] + extra)
    tr = plugin.main.args[0](params, "cuda:0")
    dialogs = make_dialogues(a.batch, params.dims(), n_speakers=params.n_speakers, n_classes=params.n_classes,
                             min_len=min(20, a.t_max), max_len=a.t_max, seed=7, force_max=True)
    batch = tr.prepare_batch(ERCCollate(params)([[d] for d in dialogs]))
    n_utt, T = int(batch["text_length"].sum()), int(batch["text_length"].max())
    shape = [a.batch, T, n_utt]
    if a.mode == "bucket":
        tr.t_cap = a.t_cap
        key, make, fill = tr.capacity_bucket(batch)
        static = make()
        fill(static, batch)
        batch, shape = static, list(key[1:])
        tr.model.dynamic_n = True
    tr.model.train()
    step = GraphedStep(lambda: tr.train_step(batch), warmup=2)
    times = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    print(json.dumps({"tool": "bcrnn_capacity_steps", "module": "bc" + a.cell, "mode": a.mode, "launch_shape": shape, "n_utt": n_utt,
                      "t_dev": T, "steps": a.steps, "ms_per_step": statistics.median(times), "min_ms": min(times),
                      "max_ms": max(times), "utt_per_s": n_utt / statistics.median(times) * 1e3}), flush=True)


if __name__ == "__main__":
    main()
