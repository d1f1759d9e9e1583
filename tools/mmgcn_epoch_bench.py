#!/usr/bin/env python3
"""MMGCN (--module=mmgcn) over whole reshuffled epochs -- the training epoch AND the test epoch behind it, as train_mm.py
runs them -- on IEMOCAP-shaped synthetic data (iemocap-cogmen-6 atv: 120 training and 31 test dialogues of 20..110
utterances, B = 16), in five modes:

  default        no flag: every step launched from Python on its exact shape (a shape is captured only when it repeats, which
                 under reshuffling it almost never does; every new (B, T, N) builds and zero-fills a workspace first)
  exact          --fixed_batches: the opt-in sampling whose batch shapes repeat, so every step replays an exact-shape graph
  buckets        --capacity_buckets=True: capacity buckets (16 x T_cap x N_cap, N_cap a multiple of 128), one captured graph
                 each, every batch a copy-in + replay
  resident       --device_collate --resident: dialogues in HBM, a step's input is 2 B int32
  resident_eval  ... --resident_eval: the test epoch from HBM too, scored on the device

Every mode runs in a fresh process.  An epoch's time is the wall time between two of the child's epoch lines (training, test
epoch, metrics); ``train_s`` is the training part alone (utterances / the reported utterances per second).  ``--warmup``
epochs (default 1; ``exact`` gets one more: a shape is captured on its second visit) are dropped, then ``--epochs`` (5) are
timed: median, fastest and slowest.  ``--repo DIR`` times another checkout's train_mm.py (the baseline: the parent commit's
default loop) with the same tool.

``--steps`` measures, in this process, the ms per replayed step of one bucket's graph and of an exact-shape captured graph of
the same batch (the difference is what the padding to N_cap / T_cap costs), and reports the node capacities five reshuffled
epochs touch and the workspace bytes of each of those buckets.  One JSON line per result.

    python tools/mmgcn_epoch_bench.py [--modes default,exact,buckets,resident,resident_eval] [--steps]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"default": [], "exact": ["--fixed_batches"], "buckets": ["--capacity_buckets=True"],
         "resident": ["--device_collate", "--resident"], "resident_eval": ["--device_collate", "--resident", "--resident_eval"]}
DATA = ["--dataset=iemocap-cogmen-6", "--modality=atv", "--n_train=120", "--n_test=31", "--train.batch_size=16",
        "--test.batch_size=16"]


def train_dialogues(p):
    """the synthetic training split the child draws (params.seed = 1, rank 0: trainer.load_dialogues)"""
    from erc_amd.synthetic import make_dialogues
    return make_dialogues(p.n_train, p.dims(), n_speakers=p.n_speakers, n_classes=p.n_classes, min_len=20, max_len=110, seed=p.seed)


def n_utterances():
    sys.path.insert(0, REPO)
    from erc_amd.params import ERCParams
    return [len(d["label"]) for d in train_dialogues(ERCParams().from_args(DATA))]


def run(repo, mode, epochs, warmup, timeout):
    if mode == "exact":
        warmup += 1
    args = [sys.executable, "train_mm.py", "--module=mmgcn", "--epoch=%d" % (epochs + warmup), "--log_every=0"] + DATA + MODES[mode]
    err = tempfile.TemporaryFile(mode="w+")
    proc = subprocess.Popen(args, cwd=repo, stdout=subprocess.PIPE, stderr=err, text=True)
    stamps, lines, t_end = [], [], time.monotonic() + timeout
    try:
        for raw in proc.stdout:
            if raw.startswith("{") and "train_utt_per_s" in raw:
                stamps.append(time.perf_counter())
                lines.append(json.loads(raw))
            if time.monotonic() > t_end:
                proc.kill()
                break
        proc.wait(timeout=30)
    finally:
        if proc.poll() is None:
            proc.kill()
    if proc.returncode != 0 or len(lines) != epochs + warmup:
        err.seek(0)
        return {"tool": "mmgcn_epoch_bench", "mode": mode, "error": err.read()[-600:]}
    n_utt = sum(n_utterances())
    epoch_s = [b - a for a, b in zip(stamps[warmup - 1:], stamps[warmup:])]
    train_s = [n_utt / l["train_utt_per_s"] for l in lines[warmup:]]
    last = lines[-1]
    r3 = lambda v: round(v, 4)
    return {"tool": "mmgcn_epoch_bench", "repo": os.path.relpath(repo, REPO), "mode": mode,
            "epochs_timed": len(epoch_s), "warmup_epochs": warmup, "steps_per_epoch": -(-120 // 16),
            "epoch_s_median": r3(statistics.median(epoch_s)), "epoch_s_min": r3(min(epoch_s)), "epoch_s_max": r3(max(epoch_s)),
            "train_s_median": r3(statistics.median(train_s)), "train_s_min": r3(min(train_s)), "train_s_max": r3(max(train_s)),
            "epoch_s": [r3(v) for v in epoch_s], "train_s": [r3(v) for v in train_s],
            "graph_replays": last["graph_replays"], "graphs_captured": last["graphs_captured"], "eager_steps": last["eager_steps"],
            "test_acc_last": last["test"]["acc"]}


def tensor_bytes(obj, seen=None):
    """bytes of every distinct tensor storage reachable from a workspace (dicts, lists, the planner's slab space)"""
    import torch
    seen = set() if seen is None else seen
    if torch.is_tensor(obj):
        key = obj.untyped_storage().data_ptr()
        if key in seen:
            return 0
        seen.add(key)
        return obj.untyped_storage().nbytes()
    if isinstance(obj, dict):
        return sum(tensor_bytes(v, seen) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return sum(tensor_bytes(v, seen) for v in obj)
    slabs = getattr(obj, "ws", None)      # a GemmPlanner: its slab space
    return tensor_bytes(slabs, seen) if torch.is_tensor(slabs) else 0


def step_times(iters):
    """ms per replayed step: one bucket's graph against an exact-shape graph of the same batch; the buckets five reshuffled
    epochs touch and what each one's workspace holds"""
    sys.path.insert(0, REPO)
    import torch
    from erc_amd.capacity import node_capacity
    from erc_amd.collate import ERCCollate
    from erc_amd.mmgcn import MMGCNTrainer
    from track_mm.mmgcn import MMGCNParams
    p = MMGCNParams().from_args(DATA + ["--capacity_buckets=True"])
    tr = MMGCNTrainer(p, "cuda:0")
    train = train_dialogues(p)
    lens = [len(d["label"]) for d in train]
    tr.t_cap = max(lens)
    gen = torch.Generator().manual_seed(p.seed)
    caps = []
    for _ in range(5):
        order = torch.randperm(len(lens), generator=gen).tolist()
        caps += [node_capacity(sum(lens[i] for i in order[s:s + 16]), tr.N_BUCKET, 16 * tr.t_cap) for s in range(0, len(lens), 16)]
    batch = tr.prepare_batch(ERCCollate(p)([[d] for d in train[:16]]))
    key, make, fill = tr.capacity_bucket(batch)
    static = make()
    fill(static, batch)
    T, B = (int(v) for v in batch["speaker_tensor"].shape[:2])
    out = {"tool": "mmgcn_epoch_bench", "batch": {"B": B, "T": T, "N": int(batch["label"].shape[0])}, "bucket": list(key[1:]),
           "node_capacities_of_5_epochs": {str(c): caps.count(c) for c in sorted(set(caps))}}
    for name, b, cap in (("exact_step_ms", batch, False), ("bucket_step_ms", static, True)):
        tr.model.dynamic_n = cap
        tr.train_step(b)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            tr.train_step(b)
        for _ in range(10):
            g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            g.replay()
        torch.cuda.synchronize()
        out[name] = round((time.perf_counter() - t0) / iters * 1e3, 4)
        out[name.replace("step_ms", "workspace_mb")] = round(tensor_bytes(tr.model._last_ws) / 2 ** 20, 1)
        tr.model.dynamic_n = False
        del g
    tr.model.check_cluster()
    # the workspace of every bucket an epoch touches, built one at a time (nothing runs on it)
    out["workspace_mb_per_bucket"] = {}
    for c in sorted(set(caps)):
        ws = tr.model._make_workspace(16, tr.t_cap, c, tr.device, cap=True)
        out["workspace_mb_per_bucket"][str(c)] = round(tensor_bytes(ws) / 2 ** 20, 1)
        del ws
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="default,exact,buckets,resident,resident_eval")
    ap.add_argument("--repo", default=REPO, help="the checkout whose train_mm.py is timed")
    ap.add_argument("--steps", action="store_true", help="also time one replayed step, bucket against exact shape")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per run")
    a = ap.parse_args()
    for mode in [m for m in a.modes.split(",") if m]:
        print(json.dumps(run(os.path.abspath(a.repo), mode, a.epochs, max(1, a.warmup), a.timeout)), flush=True)
    if a.steps:
        print(json.dumps(step_times(a.iters)), flush=True)


if __name__ == "__main__":
    main()
