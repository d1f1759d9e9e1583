#!/usr/bin/env python3
"""MMIN base model training step (--module=mmin_base; synthetic utterances: audio [B, Ta, 130], visual [B, 50, 342], text
[B, 22, 1024]) timed with device events: the eager step and the step captured into a HIP graph (warm-up replays, then the median
of --replays), the two scan launches (both encoders in each) and the two text CNN entry points timed on their own (the step's
recorded calls re-issued), and the same step restated on the CPU (tests/mmin_ref.py in float64 + torch.optim.Adam, 16 threads) as
the baseline.  One JSON line per (batch size, Ta).

    python tools/mmin_bench.py [--batch 32] [--ta 100,400] [--replays 50] [--cpu_steps 1]

Whole epochs (training + validation + test, in every loop form) are timed by tools/epoch_bench.py --module=mmin_base.
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
ALONE = ("erc_lstm128_pool_fwd", "erc_lstm128_pool_bwd", "erc_textcnn_pool_fwd", "erc_textcnn_pool_bwd", "erc_wgrad_table",
         "erc_adam_step", "erc_ema_step")


def make_batch(B, Ta, seed):
    from erc_amd.mmin import mmin_collate
    from erc_amd.synthetic import make_mmin_samples
    return mmin_collate(make_mmin_samples(B, "train", seed=seed, frames=(Ta, Ta)))


def event_times(fn, n, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def gpu_time(B, Ta, replays, warmup):
    from erc_amd import capi
    from erc_amd.engine import GraphedStep
    from erc_amd.mmin import MMINBaseTrainer
    from track_mm.mmin_base import MMINBaseParams
    tr = MMINBaseTrainer(MMINBaseParams().from_args([]), "cuda:0")
    b = tr.prepare_batch(make_batch(B, Ta, 7))
    capi.start_recording()
    tr.train_step(b)
    torch.cuda.synchronize()
    rec = capi.stop_recording()
    res = {"B": B, "Ta": Ta, "launching_calls_per_step": sum(1 for e in rec if capi._launches(e[0]))}
    for name in ALONE:
        entries = [e for e in rec if e[0] == name]
        assert len(entries) == 1, (name, len(entries))
        t = event_times(lambda: capi.replay(entries[0]), replays, warmup)
        res[name[4:] + "_ms"] = statistics.median(t)
    res["scan_fwd_us_per_step"] = res["lstm128_pool_fwd_ms"] / max(Ta, 50) * 1e3
    res["scan_bwd_us_per_step"] = res["lstm128_pool_bwd_ms"] / max(Ta, 50) * 1e3
    eager = event_times(lambda: tr.train_step(b), replays, warmup)
    step = GraphedStep(lambda: tr.train_step(b), warmup=2)
    times = event_times(step, replays, warmup)
    ms = statistics.median(times)
    res.update(eager_ms_per_step=statistics.median(eager), ms_per_step=ms, min_ms=min(times), max_ms=max(times), utt_per_s=B / ms * 1e3,
               replays_by=step.captured.replays_by)
    return res


def cpu_time(B, Ta, steps):
    """the restated step in float64 (tests/mmin_ref.py: forward, backward on its own routing) + torch.optim.Adam + the EMA formula"""
    from tests import mmin_ref as R
    from erc_amd.mmin import MMINBaseModule
    torch.set_num_threads(16)
    m = MMINBaseModule(R.VISUAL_D, R.TEXT_D, R.AUDIO_D, 4)
    P = {k: v.detach().double().requires_grad_() for k, v in m.state_dict().items()}
    ema = {k: v.detach().clone() for k, v in P.items()}
    opt = torch.optim.Adam(list(P.values()), lr=2e-4)
    batch = make_batch(B, Ta, 7)
    times = []
    for _ in range(steps + 1):
        t0 = time.perf_counter()
        with torch.no_grad():
            r = R.model_loss_grads({k: v.detach() for k, v in P.items()}, batch)
            for k, v in P.items():
                v.grad = r["grads"][k].reshape(v.shape)
            opt.step()
            for k in ema:
                ema[k].mul_(0.999).add_(P[k].detach(), alpha=0.001)
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="32")
    ap.add_argument("--ta", default="100,400")
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu_steps", type=int, default=1)
    args = ap.parse_args()
    for B in (int(v) for v in args.batch.split(",")):
        for Ta in (int(v) for v in args.ta.split(",")):
            res = gpu_time(B, Ta, args.replays, args.warmup)
            if args.cpu_steps > 0:
                res["cpu16_float64_ms_per_step"] = cpu_time(B, Ta, args.cpu_steps)
                res["speedup_vs_cpu16"] = res["cpu16_float64_ms_per_step"] / res["ms_per_step"]
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
