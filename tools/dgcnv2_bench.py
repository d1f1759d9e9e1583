#!/usr/bin/env python3
"""conv-emotion DialogueGCN training step (--module=dgcnv2, LSTM base, iemocap-cogmen-6 atv synthetic dialogues of up to 110
utterances, D = 712) timed as a captured HIP graph with device events: warm-up replays, then the median of --replays replays.
Prints one JSON line per batch size with ms/step, utterances/s, launches per step, and the same step restated on the CPU
(tests/dgcnv2_oracle.py, autograd + Adam, 16 threads) as the baseline.

    python tools/dgcnv2_bench.py [--batch 32] [--replays 50] [--cpu_steps 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def make_batch(params, B, seed):
    from erc_amd.collate import ERCCollate
    from erc_amd.synthetic import make_dialogues
    dialogs = make_dialogues(B, params.dims(), n_speakers=params.n_speakers, n_classes=params.n_classes, min_len=20,
                             max_len=110, seed=seed, force_max=True)
    return ERCCollate(params)([[d] for d in dialogs])


def count_launches(tr, b):
    from erc_amd import capi
    capi.start_recording()
    tr.train_step(b)
    torch.cuda.synchronize()
    rec = capi.stop_recording()
    return len(rec) + 1          # + the memset of dM (the only launch that is not a C-ABI call)


def gpu_time(B, replays, warmup):
    from track_mm.dgcnv2 import DGCNParams
    from erc_amd.dgcnv2 import DGCNv2Trainer
    from erc_amd.engine import GraphedStep
    params = DGCNParams().from_args(["--dataset=iemocap-cogmen-6"])
    tr = DGCNv2Trainer(params, "cuda:0")
    batch = make_batch(params, B, 7)
    n_utt = int(batch["text_length"].sum())
    b = tr.prepare_batch(batch)
    launches = count_launches(tr, b)
    step = GraphedStep(lambda: tr.train_step(b), warmup=2)
    for _ in range(warmup):
        step()
    times = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = statistics.median(times)
    return params, batch, dict(ms_per_step=ms, utt_per_s=n_utt / ms * 1e3, launches_per_step=launches, n_utt=n_utt,
                               T=int(batch["text_length"].max()), min_ms=min(times), max_ms=max(times))


def cpu_time(params, batch, steps):
    from erc_amd.capacity import IEMOCAP6_WEIGHTS
    from erc_amd.dgcnv2 import DGCNModule
    from tests.dgcnv2_oracle import DEAD, forward
    torch.set_num_threads(16)
    m = DGCNModule("LSTM", input_size=params.hidden_all, n_speakers=params.n_speakers, n_classes=params.n_classes)
    P = {k: torch.nn.Parameter(v.detach().clone()) for k, v in m.state_dict().items()}
    opt = torch.optim.Adam([v for k, v in P.items() if not k.startswith(DEAD)], lr=3e-4)
    w = torch.tensor(IEMOCAP6_WEIGHTS)
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        logits, _ = forward(P, batch)
        loss = torch.nn.functional.cross_entropy(logits, batch["label"], weight=w)
        opt.zero_grad()
        loss.backward()
        opt.step()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="32")
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu_steps", type=int, default=2)
    args = ap.parse_args()
    for B in (int(v) for v in args.batch.split(",")):
        params, batch, res = gpu_time(B, args.replays, args.warmup)
        cpu_ms = cpu_time(params, batch, args.cpu_steps) if args.cpu_steps > 0 else None
        res.update(module="dgcnv2", base_model="LSTM", dataset="iemocap-cogmen-6", modality="atv", B=B, replays=args.replays,
                   cpu16_ms_per_step=cpu_ms, speedup_vs_cpu16=(cpu_ms / res["ms_per_step"]) if cpu_ms else None)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
