#!/usr/bin/env python3
"""MMIN base model training step (--module=mmin_base; synthetic utterances: audio [B, Ta, 130], visual [B, 50, 342], text
[B, 22, 1024]) timed with device events: the eager step and the step captured into a HIP graph (warm-up replays, then the median
of --replays), the two scan launches (both encoders in each) and the two text CNN entry points timed on their own (the step's
recorded calls re-issued), and the same step restated on the CPU (tests/mmin_ref.py in float64 + torch.optim.Adam, 16 threads) as
the baseline.  One JSON line per (batch size, Ta).

    python tools/mmin_bench.py [--batch 32] [--ta 100,400] [--replays 50] [--cpu_steps 1]

    python tools/mmin_bench.py --eval_missing [--batch 32] [--ta 100,400] [--repeats 20]

``--eval_missing`` times a validation epoch of 64 utterances (two passes: model and EMA) with a host clock around work that ends
in a device synchronise, the variants alternating inside one process: the plain pass (the code path without the flag), the pass
with the fused scoring behind every forward, and the naive route (the plain pass plus six more over host-masked batches); then
the same epoch under ``--resident_eval`` with and without the flag, each in a child process of its own (a captured step binds to
its trainer); then erc_mmin_collate_masked beside erc_mmin_collate on one bucket of B slots (device events).

Whole epochs (training + validation + test, in every loop form) are timed by tools/epoch_bench.py --module=mmin_base.
"""
import argparse
import json
import os
import statistics
import subprocess
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


# ------------------------------------------------------------------------------------------------------------ --eval_missing
N_VAL = 64


def _eval_trainer(B, *flags):
    from erc_amd.mmin import MMINBaseTrainer
    from track_mm.mmin_base import MMINBaseParams
    p = MMINBaseParams().from_args(["--val.batch_size=%d" % B, "--train.batch_size=%d" % B, "--test.batch_size=%d" % B] + list(flags))
    tr = MMINBaseTrainer(p, "cuda:0")
    tr.ema.mul_(0.5)           # the EMA pass computes with weights of its own
    return tr


def _val_samples(Ta):
    from erc_amd.synthetic import make_mmin_samples
    return make_mmin_samples(N_VAL, "val", seed=11, frames=(Ta, Ta))


def _wall_ms(fns, repeats, warmup):
    """median wall time of every variant, the variants alternating; each call ends in a device synchronise"""
    times = [[] for _ in fns]
    for r in range(warmup + repeats):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                times[i].append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(t) for t in times], [min(t) for t in times], [max(t) for t in times]


def eval_missing_default_loop(B, Ta, repeats, warmup):
    from torch.utils.data import DataLoader
    from erc_amd import capi
    from erc_amd.mmin import MISSING_TYPES, MODAL_KEYS, mmin_collate
    plain, fused = _eval_trainer(B), _eval_trainer(B, "--eval_missing")
    loader = DataLoader(_val_samples(Ta), batch_size=B, shuffle=False, collate_fn=mmin_collate)
    batches = [plain.prepare_batch(b) for b in loader]
    masked = [[dict(b, **{key: b[key] * m[i] for i, key in enumerate(MODAL_KEYS)}) for m in MISSING_TYPES] for b in batches]

    def naive():
        plain.eval_epoch(loader)
        for k in (0, 1):
            with (plain.ema_weights() if k else _null()):
                logits = [plain.to_logits(mb).clone() for six in masked for mb in six]
        torch.stack([lg.argmax(-1) for lg in logits]).cpu()
    capi.start_recording()
    fused.eval_epoch(loader)
    rec = capi.stop_recording()
    names = [e[0] for e in rec]
    med, lo, hi = _wall_ms([lambda: plain.eval_epoch(loader), lambda: fused.eval_epoch(loader), naive], repeats, warmup)
    return {"eval_missing": "default_loop", "B": B, "Ta": Ta, "n_val": N_VAL, "plain_ms": med[0], "fused_ms": med[1], "naive_ms": med[2],
            "plain_min_max_ms": [lo[0], hi[0]], "fused_min_max_ms": [lo[1], hi[1]], "naive_min_max_ms": [lo[2], hi[2]],
            "fused_over_plain": med[1] / med[0], "naive_over_fused": med[2] / med[1],
            "zero_scans_per_epoch": names.count("erc_lstm128_prefix_max"), "launching_calls_per_epoch": sum(1 for n in names if capi._launches(n))}


def _null():
    import contextlib
    return contextlib.nullcontext()


def eval_missing_resident_child(B, Ta, repeats, warmup, with_flag):
    from erc_amd.datasets import MMINDeviceStore
    from erc_amd.mmin import MMINResidentEval
    flags = ["--device_collate", "--resident", "--resident_eval"] + (["--eval_missing"] if with_flag else [])
    tr = _eval_trainer(B, *flags)
    ev = MMINResidentEval(tr, MMINDeviceStore(_val_samples(Ta), "cuda:0"), B)
    med, lo, hi = _wall_ms([ev.epoch], repeats, warmup)
    return {"eval_missing": "resident_eval", "with_flag": with_flag, "B": B, "Ta": Ta, "n_val": N_VAL, "epoch_ms": med[0],
            "min_max_ms": [lo[0], hi[0]], "graph_replays": ev.replays, "graphs_captured": ev.captures}


def collate_masked_times(B, T_cap, replays, warmup):
    from erc_amd import capi
    from erc_amd.datasets import MMINMaskedDeviceStore
    from erc_amd.mmin import MMINBaseTrainer
    from erc_amd.synthetic import make_mmin_samples
    from track_mm.mmin_base import MMINBaseParams
    tr = MMINBaseTrainer(MMINBaseParams().from_args(["--train.batch_size=%d" % B]), "cuda:0")
    store = MMINMaskedDeviceStore(make_mmin_samples(B, "train", seed=7, frames=(T_cap, T_cap)), "cuda:0")
    bits = [[(1, 2, 4, 3, 5, 6)[i % 6] for i in range(B)]]
    table, _ = store.table([list(range(B))], B, bits)
    d4 = torch.from_numpy(table[0]).to("cuda:0")
    d3 = d4[:3 * B].contiguous()
    out = tr.make_bucket(B, T_cap, int(store.visual.shape[1]), int(store.text.shape[1]))
    call = lambda desc, masked: capi.mmin_collate(desc, store.audio, store.visual, store.text, store.label, B, T_cap, T_cap, out["audio_feature"],
                                                  out["visual_feature"], out["text_feature"], out["label"], out["counts"], masked=masked)
    t3 = event_times(lambda: call(d3, False), replays, warmup)
    t4 = event_times(lambda: call(d4, True), replays, warmup)
    written = sum(out[k].numel() * 4 for k in ("audio_feature", "visual_feature", "text_feature"))
    return {"eval_missing": "collate", "B": B, "T_cap": T_cap, "mmin_collate_ms": statistics.median(t3),
            "mmin_collate_masked_ms": statistics.median(t4), "bytes_written": written}


def eval_missing_main(args):
    if args.child:
        B, Ta = int(args.batch), int(args.ta)
        print(json.dumps(eval_missing_resident_child(B, Ta, args.repeats, args.warmup, args.child == "resident_missing")), flush=True)
        return
    for B in (int(v) for v in args.batch.split(",")):
        for Ta in (int(v) for v in args.ta.split(",")):
            print(json.dumps(eval_missing_default_loop(B, Ta, args.repeats, args.warmup)), flush=True)
            for child in ("resident_plain", "resident_missing"):      # a fresh process each: a captured step binds to its trainer
                cmd = [sys.executable, os.path.abspath(__file__), "--eval_missing", "--child=" + child, "--batch=%d" % B, "--ta=%d" % Ta,
                       "--repeats=%d" % args.repeats, "--warmup=%d" % args.warmup]
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if res.returncode != 0:
                    raise SystemExit("child %s failed: %s" % (child, res.stderr[-2000:]))
                print(res.stdout.strip().splitlines()[-1], flush=True)
        for T_cap in (128, 400):
            print(json.dumps(collate_masked_times(B, T_cap, args.replays, args.warmup)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eval_missing", action="store_true", help="time a validation epoch under --eval_missing and the masked collate")
    ap.add_argument("--repeats", type=int, default=20, help="--eval_missing: timed epochs per variant")
    ap.add_argument("--child", default="", help="--eval_missing: (internal) resident_plain | resident_missing, one process each")
    ap.add_argument("--batch", default="32")
    ap.add_argument("--ta", default="100,400")
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu_steps", type=int, default=1)
    args = ap.parse_args()
    if args.eval_missing:
        return eval_missing_main(args)
    for B in (int(v) for v in args.batch.split(",")):
        for Ta in (int(v) for v in args.ta.split(",")):
            res = gpu_time(B, Ta, args.replays, args.warmup)
            if args.cpu_steps > 0:
                res["cpu16_float64_ms_per_step"] = cpu_time(B, Ta, args.cpu_steps)
                res["speedup_vs_cpu16"] = res["cpu16_float64_ms_per_step"] / res["ms_per_step"]
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
