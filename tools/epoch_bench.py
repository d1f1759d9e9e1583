#!/usr/bin/env python3
"""Whole reshuffled epochs of any ``--module`` -- the training epoch AND the test epoch behind it, as train_mm.py runs them
(trainer.EpochLoop, or the loop class the module's trainer names: trainer.epoch_loop_class) -- on the synthetic presets
below, in these modes:

  eager          --graph_capture=False: every step launched from Python (capacity buckets' static buffers, no replay)
  default        no flag: the module's default loop (exact shapes, captured when a shape repeats; capacity buckets where
                 the trainer has them on by default: COGMEN bf16, DialogueGCN)
  exact          --fixed_batches: the opt-in sampling whose batch shapes repeat, so every step replays an exact-shape graph
  buckets        --capacity_buckets=True: one captured graph per capacity bucket, every batch a copy-in + replay
  resident       --device_collate --resident: dialogues in HBM, a step's input is 2 B int32 (MMIN: utterances, 3 B int32)
  resident_eval  ... --resident_eval: the test epoch from HBM too, scored on the device

The MMIN modules' "test epoch" is their validation epoch (with the plateau scheduler behind it) plus their test epoch:
``test_ms`` of an ``mmin_base`` / ``mmin_miss`` record covers both, and ``eval_captures_total`` counts both evaluation loops.

Every (config, mode) runs in a fresh child process of this tool under its own ``timeout -k 10``, one at a time; the first
child that ends with a non-zero status ends the tool with that status after one error line, and nothing more is started.
``--modes`` may repeat a mode (resident,resident_eval,resident,resident_eval alternates host and device test epochs).  The
child builds the plugin's trainer and an EpochLoop and times every epoch with three device events: ``train_ms`` from the
first training launch to the last, ``epoch_ms`` to the end of the test epoch.  The first ``--warmup`` epochs (``exact`` gets
one more: a shape is captured on its second visit) are dropped, then ``--epochs`` are timed: median, fastest, slowest and
the list.  Per epoch it also reports the replays, eager steps and captures, and ``launches_per_eager_step``: the C-ABI
calls one eager training step makes to launch itself, in capacity form where the trainer offers a bucket -- every recorded
call, as tools/bcrnn_bench.py counts its ``launches_per_step`` and DESIGN.md states the steps (bc-RNN: 22); of these,
``kernel_launches_per_eager_step`` take a stream and enqueue work (bc-RNN: 19), the others are host-side queries.  After
the runs of a config the parent prints one ratio line per pair of modes that both ran (medians of their last runs).
``--repo DIR`` times another checkout's package; ``--set KEY=VALUE`` overrides a flag of the preset; ``--collate_on_device``
adds --device_collate to the modes that lack it; ``--eval_missing`` / ``--train_missing`` set the MMIN modules' flags of that name.

``--steps`` (trainers with capacity buckets) times, in one more child per config, the replayed step on a bucket's static
buffers against an exact-shape graph of the same first batch, and reports the workspace bytes of both, the node capacities
five reshuffled epochs touch with the workspace bytes of each, and the padding share 1 - mean(longest dialogue of the
batch / T_cap).  One JSON line per result.  Nothing outside the checkout is read.

    python tools/epoch_bench.py --module=dialogrnn [--config=iemocap,sbert] [--modes=default,resident] [--steps]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"eager": ["--graph_capture=False"], "default": [], "exact": ["--fixed_batches"], "buckets": ["--capacity_buckets=True"],
         "resident": ["--device_collate", "--resident"], "resident_eval": ["--device_collate", "--resident", "--resident_eval"]}
IEMOCAP = ["--dataset=iemocap-cogmen-6", "--n_train=120", "--n_test=31"]
MELD = ["--dataset=meld-mmgcn-7", "--modality=atv", "--loss_weights=False", "--n_train=1039", "--n_test=280"]
BCRNN = (32, {"iemocap": IEMOCAP, "meld": MELD})
# utterances of 50..400 audio frames (two T capacities at B = 32) and of exactly 100 (one)
MMIN_SPLITS = ["--dataset=iemocap-mmin-4", "--n_train=1024", "--n_val=64", "--n_test=64", "--val.batch_size=32"]
MMIN = (32, {"f50_400": MMIN_SPLITS + ["--mmin_frames=50,400"], "f100_100": MMIN_SPLITS + ["--mmin_frames=100,100"]})
# module -> (batch size, {config: flags})
PRESETS = {
    "cogmen": (32, {"iemocap": IEMOCAP + ["--compute=bf16"],
                    "meld": ["--dataset=iemocap-cogmen-6", "--compute=bf16", "--n_train=1039", "--n_test=280", "--syn_min_len=1",
                             "--syn_max_len=33"]}),
    "dgcn": (32, {"meld": MELD + ["--compute=bf16"], "iemocap": IEMOCAP + ["--compute=f32", "--relation_space=False"]}),
    "bclstm": BCRNN,
    "bcgru": BCRNN,
    "dgcnv2": (32, {"lstm": IEMOCAP + ["--modality=atv", "--base_model=LSTM"], "none": IEMOCAP + ["--modality=atv", "--base_model=None"]}),
    "dialogrnn": (32, {"iemocap": IEMOCAP + ["--modality=atv"],
                       "sbert": ["--dataset=iemocap-cogmen-sbert-6", "--modality=atv", "--n_train=120", "--n_test=31"]}),
    "cim": (32, {"iemocap": IEMOCAP + ["--modality=atv"],
                 "mosei": ["--dataset=mosei-cim-2", "--modality=atv", "--n_train=2240", "--n_test=672"]}),
    "dagerc": (16, {"bf16": IEMOCAP + ["--compute=bf16"], "f32": IEMOCAP + ["--compute=f32"]}),
    "mmgcn": (16, {"iemocap": IEMOCAP + ["--modality=atv"]}),
    "mmin_base": MMIN,
    "mmin_miss": MMIN,
}
# the multi-label metrics of CMU-MOSEI are no function of a confusion matrix; bc-LSTM / bc-GRU have no scored test step; the
# MMIN modules have no --fixed_batches and no node buckets, and without a capacity flag their --graph_capture=False is the
# default loop; mmin_miss's trainer refuses the capacity modes
MMIN_UNBUILT = {"exact", "eager", "steps"}
SKIPPED = {("cim", "mosei"): {"resident_eval"}, ("bclstm", None): {"resident_eval"}, ("bcgru", None): {"resident_eval"},
           ("mmin_base", None): MMIN_UNBUILT, ("mmin_miss", None): MMIN_UNBUILT | {"buckets", "resident", "resident_eval"}}


def skipped(module, config, mode):
    return mode in SKIPPED.get((module, config), ()) or mode in SKIPPED.get((module, None), ())


def plugin(module):
    """(trainer class, params class) of ``--module``: every plugin is ``partial(run, Trainer, ParamsType)``"""
    return importlib.import_module("track_mm." + module).main.args


def flags(module, config, mode, sets=(), collate_on_device=False):
    """the preset's command line for one mode; a later flag replaces an earlier one of the same key"""
    batch, configs = PRESETS[module]
    out = configs[config] + ["--train.batch_size=%d" % batch, "--test.batch_size=%d" % batch] + MODES.get(mode, [])
    if collate_on_device and "--device_collate" not in out:
        out.append("--device_collate")
    for kv in sets:
        key = "--" + kv.split("=", 1)[0]
        out = [f for f in out if f.split("=", 1)[0] != key] + ["--" + kv]
    return out


def warmup_of(mode, warmup):
    return max(1, warmup) + (mode == "exact")


def summarise(train_ms, epoch_ms, counts, warmup):
    """the timing part of a child's record: ``counts`` holds (replays, eager steps, captures) per epoch; the first ``warmup``
    epochs are dropped from the times"""
    r3 = lambda v: round(v, 3)
    tt, te, tc = train_ms[warmup:], epoch_ms[warmup:], counts[warmup:]
    test = [e - t for t, e in zip(tt, te)]
    out = {"epochs_timed": len(te), "warmup_epochs": warmup}
    for name, v in (("epoch_ms", te), ("train_ms", tt), ("test_ms", test)):
        out.update({name + "_median": r3(statistics.median(v)), name + "_min": r3(min(v)), name + "_max": r3(max(v)),
                    name: [r3(x) for x in v]})
    out.update(replay_share_timed=r3(sum(c[0] for c in tc) / max(1, sum(c[0] + c[1] for c in tc))),
               replays_by_epoch=[c[0] for c in counts], eager_steps_by_epoch=[c[1] for c in counts],
               captures_by_epoch=[c[2] for c in counts])
    return out


def ratios(module, config, recs):
    """one line per pair of modes that both ran: the first over the second, from the medians of their last runs"""
    names = list(recs)
    return [{"tool": "epoch_bench", "module": module, "config": config, "modes": [a, b],
             **{k + "_ratio": round(recs[a][k + "_median"] / max(recs[b][k + "_median"], 1e-9), 4) for k in ("train_ms", "test_ms", "epoch_ms")}}
            for i, a in enumerate(names) for b in names[i + 1:]]


def eager_probe(T, tr, loader):
    """(the first batch on the device, its capacity bucket filled with it or None)"""
    probe = tr.prepare_batch(T.first_batch(loader))
    bucket = tr.capacity_bucket(probe) if hasattr(tr, "capacity_bucket") else None
    if bucket is None:
        return probe, None
    static = bucket[1]()
    bucket[2](static, probe)
    return probe, (bucket[0], static)


def child(a):
    """one (config, mode) in this process, on the package of the checkout ``a.repo``; prints its JSON line"""
    sys.path.insert(0, a.repo)
    import torch
    from erc_amd import capi, trainer as T
    trainer_cls, params_cls = plugin(a.module)
    mode, steps = a.modes, a.modes == "steps"
    warmup = warmup_of(mode, a.warmup)
    params = params_cls().from_args(flags(a.module, a.config, "buckets" if steps else mode, a.set, a.collate_on_device) +
                                    ["--epoch=%d" % (a.epochs + warmup), "--log_every=0"])
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    T.fix_seed(params.seed)
    tr = trainer_cls(params, device)
    head = {"tool": "epoch_bench", "repo": os.path.relpath(a.repo, REPO), "module": a.module, "config": a.config, "mode": mode,
            "dataset": params.dataset, "batch_size": int(params.train.batch_size)}
    if steps:
        return print(json.dumps(dict(head, **step_times(T, tr, params, a.iters))), flush=True)
    loop = T.epoch_loop_class(trainer_cls)(params, tr, device)
    evals = [e for e in (getattr(loop, "res_val", None), loop.res_eval) if e is not None]      # (res_val: the MMIN loop's)
    multiemo = params.get("mosei_metric", "") == "multiemo"
    c = loop.counters
    seen = lambda: (c.replays, c.eager, c.captures) if c is not None else (0, 0, 0)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    train_ms, epoch_ms, counts, n_utt = [], [], [], 0
    for _ in range(a.epochs + warmup):
        before = seen()
        tr.model.train()
        marks[0].record()
        n_utt, per_step = loop.train_epoch()
        marks[1].record()
        tr.model.eval()
        loop.test_epoch(multiemo)
        marks[2].record()
        torch.cuda.synchronize()
        train_ms.append(marks[0].elapsed_time(marks[1]))
        epoch_ms.append(marks[0].elapsed_time(marks[2]))
        now = seen()
        counts.append([y - x for x, y in zip(before, now)] if c is not None else [0, len(per_step), 0])
    loss = float((loop.resident.acc[0] if loop.resident is not None else loop.ring[:loop.n_steps, 0].sum()).cpu())
    # the C-ABI calls of one eager step (after the timed epochs: it is one more optimizer step)
    probe, bucket = eager_probe(T, tr, loop.train_loader)
    tr.model.train()
    capi.start_recording()
    with T.dynamic_n(tr.model, bucket is not None):
        tr.train_step(bucket[1] if bucket is not None else probe)
    calls = [name for name, _ in capi.stop_recording()]
    launches = sum(1 for name in calls if capi._launches(name))
    torch.cuda.synchronize()
    print(json.dumps(dict(head, device_collate=bool(params.get("device_collate", False)), steps_per_epoch=loop.n_steps,
                          utterances_per_epoch=n_utt, **summarise(train_ms, epoch_ms, counts, warmup),
                          captures_total=c.captures if c is not None else 0,
                          eval_captures_total=sum(e.captures for e in evals),
                          launches_per_eager_step=len(calls), kernel_launches_per_eager_step=launches, loss_finite=loss == loss and abs(loss) != float("inf"))), flush=True)


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


def step_times(T, tr, params, iters):
    """ms per replayed step: one bucket's graph against an exact-shape graph of the same first batch; what five reshuffled
    epochs touch.  Everything comes from the lengths, the trainer's N_BUCKET and T_cap."""
    import torch
    from erc_amd.capacity import node_capacity
    loader, _ = T.make_loaders(params, 0, 1, tr.device)
    lens = loader.store.lengths.tolist() if isinstance(loader, T.StoreLoader) else [len(d["label"]) for d in loader.dataset.dialogs]
    B, t_cap = int(params.train.batch_size), max(lens)
    tr.t_cap = t_cap
    gen = torch.Generator().manual_seed(params.seed)
    caps, shares = [], []
    for _ in range(5):
        order = torch.randperm(len(lens), generator=gen).tolist()
        for s in range(0, len(lens), B):
            part = [lens[i] for i in order[s:s + B]]
            caps.append(node_capacity(sum(part), tr.N_BUCKET, B * t_cap))
            shares.append(max(part) / t_cap)
    batch, bucket = eager_probe(T, tr, loader)
    if bucket is None:
        raise SystemExit("--steps: this trainer offers no capacity bucket for the first batch of this configuration")
    mb = lambda: round(tensor_bytes(getattr(tr.model, "_last_ws", None)) / 2 ** 20, 1)
    out = {"batch": {"B": min(B, len(lens)), "N": int(batch["label"].shape[0])}, "bucket": list(bucket[0][1:]),
           "node_capacities_of_5_epochs": {str(v): caps.count(v) for v in sorted(set(caps))},
           "padding_share": round(1.0 - sum(shares) / len(shares), 4)}
    tr.model.train()
    for name, b, cap in (("exact", batch, False), ("bucket", bucket[1], True)):
        with T.dynamic_n(tr.model, cap):
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
        out[name + "_step_ms"] = round((time.perf_counter() - t0) / iters * 1e3, 4)
        out[name + "_workspace_mb"] = mb()
        del g
    getattr(tr.model, "check_cluster", lambda: None)()
    # the workspace of every bucket an epoch touches: one eager step on made-up lengths each (the precapture filler)
    out["workspace_mb_per_bucket"] = {}
    for key, make, _, synth in tr.all_capacity_buckets(batch):
        if key[3] in caps:
            static = make()
            synth(static)
            with T.dynamic_n(tr.model):
                tr.train_step(static)
            out["workspace_mb_per_bucket"][str(key[3])] = mb()
    torch.cuda.synchronize()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--module", required=True)
    ap.add_argument("--config", default="", help="comma-separated configs of the module's preset (default: all)")
    ap.add_argument("--modes", default="default,exact,buckets,resident,resident_eval", help="comma-separated; a mode may repeat")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--set", action="append", default=[], metavar="KEY=VALUE", help="override a flag of the preset (repeatable)")
    ap.add_argument("--collate_on_device", action="store_true", help="add --device_collate to the modes that do not have it")
    ap.add_argument("--eval_missing", action="store_true", help="mmin_base / mmin_miss: --set eval_missing=True (six more patterns per evaluation)")
    ap.add_argument("--train_missing", action="store_true", help="mmin_base: --set train_missing=True (the augmented baseline's masked training)")
    ap.add_argument("--steps", action="store_true", help="also time one replayed step, bucket against exact shape")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repo", default=REPO, help="the checkout whose package is timed")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", action="store_true", help="run the one (config, mode) given in this process")
    a = ap.parse_args(argv)
    a.repo = os.path.abspath(a.repo)
    a.set = a.set + [k + "=True" for k in ("eval_missing", "train_missing") if getattr(a, k)]
    if a.module not in PRESETS:
        raise SystemExit("--module=%s has no preset; known: %s" % (a.module, ", ".join(sorted(PRESETS))))
    if a.child:
        return child(a)
    for config in [c for c in a.config.split(",") if c] or list(PRESETS[a.module][1]):
        recs = {}
        for mode in [m for m in a.modes.split(",") if m] + (["steps"] if a.steps else []):
            if skipped(a.module, config, mode):
                continue
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--module=" + a.module,
                   "--config=" + config, "--modes=" + mode, "--epochs=%d" % a.epochs, "--warmup=%d" % a.warmup, "--iters=%d" % a.iters,
                   "--repo=" + a.repo] + ["--set=" + kv for kv in a.set] + (["--collate_on_device"] if a.collate_on_device else [])
            res = subprocess.run(cmd, cwd=a.repo, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(res.stdout or "")
            sys.stdout.flush()
            if res.returncode != 0:
                # a child that failed (abort, fault, time limit) may have left the card in a bad state: nothing more is started
                print(json.dumps({"tool": "epoch_bench", "module": a.module, "config": config, "mode": mode,
                                  "error": "exit status %d" % res.returncode}), flush=True)
                sys.exit(res.returncode)
            lines = [json.loads(l) for l in (res.stdout or "").splitlines() if l.startswith("{")]
            if mode != "steps" and lines and "train_ms_median" in lines[-1]:
                recs.pop(mode, None)
                recs[mode] = lines[-1]
        for line in ratios(a.module, config, recs):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
