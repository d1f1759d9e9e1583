#!/usr/bin/env python3
"""bc-LSTM / bc-GRU training step (--module=bclstm, --module=bcgru; synthetic iemocap-cogmen dialogues of up to 110 utterances;
D = 712 for atv, 1380 with sbert text) timed as a captured HIP graph with device events: warm-up replays, then the median of
--replays replays.  Prints one JSON line per (cell, dataset, batch size) with ms/step (median, min, max), utterances/s,
launches per step, the four scan launches of the step timed on their own (the recorded calls re-issued: layer 0 and 1, forward
and backward; ms, share of the step, us per scan step) and the same step restated on the CPU (tests/bcrnn_oracle.py, autograd
+ Adam, 16 threads) as the baseline.  Both cells run in one process, so the LSTM scan launches of the bc-LSTM step are the
yardstick of the GRU's: ``gru_vs_lstm`` is the ratio of the time per scan step.

    python tools/bcrnn_bench.py [--cell lstm,gru] [--batch 16,32] [--dataset iemocap-cogmen-6,iemocap-cogmen-sbert-6]
                                [--replays 50] [--cpu_steps 1]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SCANS = {"lstm": ("erc_lstm_scan_fwd", "erc_lstm_scan_bwd"), "gru": ("erc_gru100_scan_fwd", "erc_gru100_scan_bwd")}


def make_batch(params, B, seed):
    from erc_amd.collate import ERCCollate
    from erc_amd.synthetic import make_dialogues
    dialogs = make_dialogues(B, params.dims(), n_speakers=params.n_speakers, n_classes=params.n_classes, min_len=20,
                             max_len=110, seed=seed, force_max=True)
    return ERCCollate(params)([[d] for d in dialogs])


def record_step(tr, b):
    from erc_amd import capi
    capi.start_recording()
    tr.train_step(b)
    torch.cuda.synchronize()
    return capi.stop_recording()


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


def gpu_time(cell, dataset, B, replays, warmup):
    from erc_amd import capi
    from erc_amd.engine import GraphedStep
    plugin = importlib.import_module("track_mm.bc" + cell)
    params = plugin.ParamsType().from_args(["--dataset=%s" % dataset])
    tr = plugin.main.args[0](params, "cuda:0")
    batch = make_batch(params, B, 7)
    n_utt, T = int(batch["text_length"].sum()), int(batch["text_length"].max())
    b = tr.prepare_batch(batch)
    rec = record_step(tr, b)
    res = {}
    for kind, name in zip(("fwd", "bwd"), SCANS[cell]):
        entries = [e for e in rec if e[0] == name]           # two launches per step: the layers
        assert len(entries) == 2, (name, len(entries))
        ts = [event_times(lambda e=e: capi.replay(e), replays, warmup) for e in entries]
        res["scan_%s_ms" % kind] = [statistics.median(t) for t in ts]
        res["scan_%s_min_max_ms" % kind] = [[min(t), max(t)] for t in ts]
        res["scan_%s_us_per_step" % kind] = statistics.mean(res["scan_%s_ms" % kind]) / T * 1e3
    step = GraphedStep(lambda: tr.train_step(b), warmup=2)
    times = event_times(step, replays, warmup)
    ms = statistics.median(times)
    res.update(ms_per_step=ms, utt_per_s=n_utt / ms * 1e3, launches_per_step=len(rec), n_utt=n_utt, T=T, D=params.hidden_all,
               min_ms=min(times), max_ms=max(times), scan_share=(sum(res["scan_fwd_ms"]) + sum(res["scan_bwd_ms"])) / ms)
    return params, batch, res


def cpu_time(cell, params, batch, steps):
    from erc_amd import bcrnn
    from erc_amd.capacity import IEMOCAP6_WEIGHTS
    from tests.bcrnn_oracle import forward
    torch.set_num_threads(16)
    m = (bcrnn.LSTMModule if cell == "lstm" else bcrnn.GRUModule)(params.hidden_all, 100, 100, n_classes=params.n_classes)
    P = {k: torch.nn.Parameter(v.detach().clone()) for k, v in m.state_dict().items()}
    opt = torch.optim.Adam(list(P.values()), lr=3e-4)
    w = torch.tensor(IEMOCAP6_WEIGHTS)
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        log_prob, _ = forward(P, batch, cell)
        loss = torch.nn.functional.nll_loss(log_prob, batch["label"], weight=w)
        opt.zero_grad()
        loss.backward()
        opt.step()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", default="lstm,gru")
    ap.add_argument("--batch", default="16,32")
    ap.add_argument("--dataset", default="iemocap-cogmen-6,iemocap-cogmen-sbert-6")
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu_steps", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bcrnn_bench.py times the step on the GPU: no device found")
    for dataset in args.dataset.split(","):
        for B in (int(v) for v in args.batch.split(",")):
            yard = None
            for cell in args.cell.split(","):
                params, batch, res = gpu_time(cell, dataset, B, args.replays, args.warmup)
                cpu_ms = cpu_time(cell, params, batch, args.cpu_steps) if args.cpu_steps > 0 else None
                res.update(module="bc" + cell, dataset=dataset, modality="atv", B=B, replays=args.replays, cpu16_ms_per_step=cpu_ms,
                           speedup_vs_cpu16=(cpu_ms / res["ms_per_step"]) if cpu_ms else None)
                if cell == "lstm":
                    yard = res
                elif yard is not None:
                    res["gru_vs_lstm"] = {k: res["scan_%s_us_per_step" % k] / yard["scan_%s_us_per_step" % k] for k in ("fwd", "bwd")}
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
