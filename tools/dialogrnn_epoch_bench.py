#!/usr/bin/env python3
"""DialogueRNN (--module=dialogrnn) over whole reshuffled epochs of synthetic iemocap-cogmen-6 dialogues (120 training and 31
test dialogues of 20..110 utterances, B = 32: 4 steps per epoch; atv = 712 features, 1380 with the sbert text) -- the training
epoch AND the test epoch behind it, as train_mm.py runs them -- in five modes:

  default        no flag: every step launched from Python on its exact shape (a shape is captured only when it repeats, which
                 under reshuffling it almost never does; every new (B, T, N) builds and zero-fills a workspace first)
  exact          --fixed_batches: the opt-in sampling whose batch shapes repeat, so every step replays an exact-shape graph
  buckets        --capacity_buckets=True: capacity buckets (32 x T_cap x N_cap, N_cap a multiple of 128), one captured graph
                 each, every batch a copy-in + replay
  resident       --device_collate --resident: dialogues in HBM, a step's input is 2 B int32
  resident_eval  ... --resident_eval: the test epoch from HBM too, scored on the device

Every (dataset, mode) runs in a fresh child process of this tool, under its own ``timeout -k 10``; the first child that ends
with a non-zero status ends the tool with that status and nothing more is started.  The child builds trainer, loaders,
StepGraphs and the resident loops with trainer.run's own functions and runs trainer.run's epoch, timed with device events:
``train_ms`` from the first training launch to the last, ``epoch_ms`` to the end of the test epoch.  The first ``--warmup``
epochs (default 1; ``exact`` gets one more: a shape is captured on its second visit) are dropped, then ``--epochs`` (5) are
timed: median, fastest and slowest.  ``--repo DIR`` times another checkout's package with the same tool (the baseline: the
parent commit's default loop, ``--device_collate`` added with ``--collate_on_device``).  Per timed epoch it also reports the
steps, how many were graph replays and how many ran eagerly, the graphs captured, and ``launches_per_eager_step``: the launching
C-ABI calls of one eager training step in the mode's own form (a replayed step is one host call).  One JSON line per result.
Nothing outside the checkout is read.

    python tools/dialogrnn_epoch_bench.py [--datasets iemocap-cogmen-6,iemocap-cogmen-sbert-6]
                                          [--modes default,exact,buckets,resident,resident_eval] [--collate_on_device]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"default": [], "exact": ["--fixed_batches"], "buckets": ["--capacity_buckets=True"],
         "resident": ["--device_collate", "--resident"], "resident_eval": ["--device_collate", "--resident", "--resident_eval"]}
N_TRAIN, N_TEST = 120, 31


def data_args(dataset, batch):
    return ["--dataset=" + dataset, "--modality=atv", "--n_train=%d" % N_TRAIN, "--n_test=%d" % N_TEST,
            "--train.batch_size=%d" % batch, "--test.batch_size=%d" % batch]


def child(repo, dataset, mode, epochs, warmup, batch, collate_on_device):
    """one mode in this process, on the package of the checkout ``repo``; prints its JSON line"""
    sys.path.insert(0, repo)
    import torch
    from erc_amd import capi, trainer as T
    from erc_amd.dialogrnn import DialogRNNTrainer
    from track_mm.dialogrnn import DialogRNNParams
    if mode == "exact":
        warmup += 1
    extra = ["--device_collate"] if collate_on_device and "--device_collate" not in MODES[mode] else []
    params = DialogRNNParams().from_args(data_args(dataset, batch) + MODES[mode] + extra +
                                         ["--epoch=%d" % (epochs + warmup), "--log_every=0"])
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    T.fix_seed(params.seed)
    tr = DialogRNNTrainer(params, device)
    train_loader, test_loader = T.make_loaders(params, 0, 1, device)
    graphs, fixed = T._setup_graphs(params, tr, train_loader, 0, 1, device)
    n_steps = len(fixed) if fixed is not None else len(train_loader)
    ring = torch.zeros(max(1, n_steps), 4, dtype=torch.float32, device=device)
    resident, res_eval = T._setup_resident(params, tr, train_loader, test_loader, 0, 1)
    counters = resident or graphs
    seen = lambda: (counters.replays, counters.eager, counters.captures)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    train_ms, epoch_ms, counts, n_utt = [], [], [], 0
    for epoch in range(epochs + warmup):
        before = seen()
        tr.model.train()
        marks[0].record()
        if resident is not None:
            n_utt, _ = resident.epoch()
        elif fixed is not None:
            n_utt = sum(T._train_epoch_fixed(fixed, graphs, tr, ring))
        else:
            n_utt = sum(T._train_epoch_loader(train_loader, graphs, tr, ring))
        marks[1].record()
        tr.model.eval()
        if res_eval is not None:
            res_eval.epoch()
        else:
            T._test_epoch_loader(tr, test_loader, False)
        marks[2].record()
        torch.cuda.synchronize()
        train_ms.append(marks[0].elapsed_time(marks[1]))
        epoch_ms.append(marks[0].elapsed_time(marks[2]))
        counts.append([b - a for a, b in zip(before, seen())])
    loss = float((resident.acc[0] if resident is not None else ring[:n_steps, 0].sum()).cpu())
    # the launching C-ABI calls of one eager step (after the timed epochs: it is one more optimizer step)
    probe = tr.prepare_batch(T.first_batch(train_loader))
    bucket = tr.capacity_bucket(probe) if hasattr(tr, "capacity_bucket") else None
    tr.model.train()
    if bucket is not None:                       # the capacity step: on a bucket's static buffers, in capacity mode
        static = bucket[1]()
        bucket[2](static, probe)
        probe = static
    capi.start_recording()
    with T.dynamic_n(tr.model, bucket is not None):
        tr.train_step(probe)
    launches = sum(1 for name, _ in capi.stop_recording() if capi._launches(name))
    torch.cuda.synchronize()
    r3 = lambda v: round(v, 3)
    timed_t, timed_e, timed_c = train_ms[warmup:], epoch_ms[warmup:], counts[warmup:]
    steps_timed = sum(c[0] + c[1] for c in timed_c)
    print(json.dumps({"tool": "dialogrnn_epoch_bench", "repo": os.path.relpath(repo, REPO), "dataset": dataset,
                      "D_m": int(params.hidden_all), "mode": mode, "device_collate": bool(params.get("device_collate", False)),
                      "batch_size": batch, "epochs_timed": len(timed_e), "warmup_epochs": warmup, "steps_per_epoch": n_steps,
                      "utterances_per_epoch": n_utt,
                      "epoch_ms_median": r3(statistics.median(timed_e)), "epoch_ms_min": r3(min(timed_e)), "epoch_ms_max": r3(max(timed_e)),
                      "train_ms_median": r3(statistics.median(timed_t)), "train_ms_min": r3(min(timed_t)), "train_ms_max": r3(max(timed_t)),
                      "epoch_ms": [r3(v) for v in timed_e], "train_ms": [r3(v) for v in timed_t],
                      "replay_share_timed": r3(sum(c[0] for c in timed_c) / max(1, steps_timed)),
                      "replays_by_epoch": [c[0] for c in counts], "eager_steps_by_epoch": [c[1] for c in counts],
                      "captures_by_epoch": [c[2] for c in counts], "captures_total": counters.captures,
                      "eval_captures_total": res_eval.captures if res_eval is not None else 0,
                      "launches_per_eager_step": launches, "loss_finite": loss == loss and abs(loss) != float("inf")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--datasets", default="iemocap-cogmen-6,iemocap-cogmen-sbert-6")
    ap.add_argument("--modes", default="default,exact,buckets,resident,resident_eval")
    ap.add_argument("--collate_on_device", action="store_true", help="add --device_collate to the modes that do not have it")
    ap.add_argument("--repo", default=REPO, help="the checkout whose package is timed (the baseline: the parent commit's default loop)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", nargs=2, metavar=("DATASET", "MODE"), help="run one mode in this process")
    a = ap.parse_args()
    if a.child:
        return child(os.path.abspath(a.repo), a.child[0], a.child[1], a.epochs, max(1, a.warmup), a.batch, a.collate_on_device)
    for dataset in [d for d in a.datasets.split(",") if d]:
        for mode in [m for m in a.modes.split(",") if m]:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", dataset, mode,
                   "--epochs=%d" % a.epochs, "--warmup=%d" % a.warmup, "--batch=%d" % a.batch, "--repo=" + os.path.abspath(a.repo)]
            cmd += ["--collate_on_device"] if a.collate_on_device else []
            rc = subprocess.run(cmd, cwd=os.path.abspath(a.repo)).returncode
            if rc != 0:
                # a child that failed (abort, fault, time limit) may have left the card in a bad state: nothing more is started
                print(json.dumps({"tool": "dialogrnn_epoch_bench", "dataset": dataset, "mode": mode, "error": "exit status %d" % rc}),
                      flush=True)
                sys.exit(rc)


if __name__ == "__main__":
    main()
