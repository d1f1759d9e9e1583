#!/usr/bin/env python3
"""MMIN missing-modality training step (--module=mmin_miss; synthetic utterances: audio [B, Ta, 130], visual [B, 50, 342], text
[B, 22, 1024], one missing pattern per sample) timed with device events:

  * the eager step and the step captured into a HIP graph (warm-up replays, then the median of --replays);
  * erc_resae_fwd and erc_resae_bwd on their own (the step's recorded calls re-issued: both autoencoders in each launch);
  * the baseline the fused launches replace: the same two chains as per-layer erc_gemm_f32 calls -- 64 forward products with the
    bias and activation in the epilogue and 64 input-gradient products with the mask in the epilogue, entry points that predate
    csrc/resae.hip -- captured in ONE graph and replayed.  The baseline has no LeakyReLU epilogue (ReLU stands in: the same
    cost) and leaves out the residual additions, both in its favour;
  * the same step restated on the CPU (tests/mmin_miss_ref.py in float64 + torch.optim.Adam, 16 threads).

The fused launches and the per-layer graph are timed --visits times in turn in the same process (the spread over the visits is
what a difference has to exceed).  One JSON line per (batch size, Ta).

    python tools/mmin_miss_bench.py [--batch 32] [--ta 100,400] [--replays 50] [--visits 3] [--cpu_steps 1]

--eval_missing times the evaluation under the six missing-modality patterns instead: per Ta a validation
epoch of --n_val utterances in batches of --batch, the model's pass alone (no EMA pass, no host copy), median of --replays:

  * plain   the full-modality pass (one forward per batch);
  * fused   the plain pass with MMINMissModule.score_missing behind every forward (the zero-input features are recomputed in
            every timed pass, as an epoch does);
  * naive   the plain pass plus six more passes of the unchanged forward over batches masked on the host with MMINMissCollate's
            arithmetic and uploaded beforehand -- the yardstick, built here only;
  * kernels erc_resae_latents on the 6 B rows and erc_resae_fwd on the B rows (both networks, as the forward launches it), the
            recorded calls re-issued.

Each of the four runs in a child process of its own; every child times the plain pass first (``plain_ms``: the spread over the
children is what a difference has to exceed).  One JSON line per (Ta, what).
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.mmin_bench import event_times  # noqa: E402

N_BLOCKS = 5


def make_batch(B, Ta, seed):
    from erc_amd.mmin_miss import MISSING_TYPES, MMINMissCollate
    from erc_amd.synthetic import make_mmin_samples
    rnd = random.Random(seed)
    samples = [dict(s, missing_type=list(rnd.choice(MISSING_TYPES))) for s in make_mmin_samples(B, "train", seed=seed, frames=(Ta, Ta))]
    return MMINMissCollate(has_miss=True)(samples)


def per_layer_graph(model, B):
    """the two chains as 128 erc_gemm_f32 launches on the model's weights, captured in one graph"""
    from erc_amd import capi
    dims, names = capi.resae_layer_dims(N_BLOCKS), capi.resae_layer_names(N_BLOCKS)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda:0")
    act_of = [1 if (l < 6 * N_BLOCKS and l % 6 in (0, 1, 3, 4)) or l == 6 * N_BLOCKS else 0 for l in range(len(dims))]
    nets = []
    for net in ("netAE", "netAE_cycle"):
        acts = [f32(B, 384)] + [f32(B, n_out) for n_out, _ in dims]                  # acts[l]: input of layer l, acts[l + 1]: its output
        grads = [f32(B, 384)] + [f32(B, n_out) for n_out, _ in dims]
        nets.append((net, acts, grads))
        acts[0].normal_()
        grads[-1].normal_()

    def run():
        for net, acts, grads in nets:
            for l, ((n_out, n_in), name) in enumerate(zip(dims, names)):
                capi.gemm_f32(acts[l], n_in, 0, None, model.flat.w("%s.%s.weight" % (net, name)), n_in, 0, None, acts[l + 1], n_out, B, n_out,
                              n_in, bias=model.flat.w("%s.%s.bias" % (net, name)), act=act_of[l])
        for net, acts, grads in nets:
            for l in range(len(dims) - 1, -1, -1):
                n_out, n_in = dims[l]
                masked = l > 0 and act_of[l - 1]
                capi.gemm_f32(grads[l + 1], n_out, 0, None, model.flat.w("%s.%s.weight" % (net, names[l])), n_in, 1, None, grads[l], n_in, B,
                              n_in, n_out, **(dict(act=2, aux=acts[l], ldaux=n_in, act_scale=1.0) if masked else {}))
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    return g, 4 * len(dims)


def gpu_time(B, Ta, replays, warmup, visits):
    from erc_amd import capi
    from erc_amd.engine import GraphedStep
    from erc_amd.mmin_miss import MMINMissTrainer
    from track_mm.mmin_miss import MMINMissParams
    tr = MMINMissTrainer(MMINMissParams().from_args([]), "cuda:0")
    b = tr.prepare_batch(make_batch(B, Ta, 7))
    capi.start_recording()
    tr.train_step(b)
    torch.cuda.synchronize()
    rec = capi.stop_recording()
    res = {"B": B, "Ta": Ta, "launching_calls_per_step": sum(1 for e in rec if capi._launches(e[0])),
           "wgrad_records": len(tr.model._last_ws["planner"].flushed)}
    fused = [[e for e in rec if e[0] == name] for name in ("erc_resae_fwd", "erc_resae_bwd")]
    assert all(len(e) == 1 for e in fused)
    graph, n_launches = per_layer_graph(tr.model, B)
    res["per_layer_launches"] = n_launches
    rows = {"resae_fwd_ms": [], "resae_bwd_ms": [], "per_layer_graph_ms": []}
    for _ in range(visits):
        rows["resae_fwd_ms"].append(statistics.median(event_times(lambda: capi.replay(fused[0][0]), replays, warmup)))
        rows["resae_bwd_ms"].append(statistics.median(event_times(lambda: capi.replay(fused[1][0]), replays, warmup)))
        rows["per_layer_graph_ms"].append(statistics.median(event_times(graph.replay, replays, warmup)))
    for k, v in rows.items():
        res[k] = statistics.median(v)
        res[k[:-3] + "_visits_ms"] = [round(x, 5) for x in v]
    res["fused_ms"] = res["resae_fwd_ms"] + res["resae_bwd_ms"]
    res["per_layer_over_fused"] = res["per_layer_graph_ms"] / res["fused_ms"]
    for name in ("erc_wgrad_table", "erc_adam_step", "erc_ema_step", "erc_lstm128_pool_fwd", "erc_lstm128_pool_bwd"):
        entries = [e for e in rec if e[0] == name]
        res[name[4:] + "_ms"] = sum(statistics.median(event_times(lambda e=e: capi.replay(e), replays, warmup)) for e in entries)
        res[name[4:] + "_calls"] = len(entries)
    eager = event_times(lambda: tr.train_step(b), replays, warmup)
    step = GraphedStep(lambda: tr.train_step(b), warmup=2)
    times = event_times(step, replays, warmup)
    ms = statistics.median(times)
    res.update(eager_ms_per_step=statistics.median(eager), ms_per_step=ms, min_ms=min(times), max_ms=max(times), utt_per_s=B / ms * 1e3,
               fused_share_of_step=res["fused_ms"] / ms, replays_by=step.captured.replays_by)
    return res


def cpu_time(B, Ta, steps):
    """the restated step in float64 (tests/mmin_miss_ref.py: both models' forward, the backward on its own routing and masks) +
    torch.optim.Adam + the EMA formula"""
    from tests import mmin_miss_ref as MR
    from tests import mmin_ref as R
    torch.set_num_threads(16)
    P = {k: v.double() for k, v in MR.named_filled(MR.sd_shapes(), 3).items()}
    Ppre = MR.named_filled(R.SD_SHAPES, 4)
    for v in P.values():
        v.requires_grad_()
    ema = {k: v.detach().clone() for k, v in P.items()}
    opt = torch.optim.Adam(list(P.values()), lr=2e-4)
    batch = make_batch(B, Ta, 7)
    times = []
    for _ in range(steps + 1):
        t0 = time.perf_counter()
        with torch.no_grad():
            rev = MR.encode(Ppre, batch["audio_feature_reverse"], batch["visual_feature_reverse"], batch["text_feature_reverse"])["features"]
            r = MR.model_loss_grads({k: v.detach() for k, v in P.items()}, batch, rev)
            for k, v in P.items():
                v.grad = r["grads"][k].reshape(v.shape)
            opt.step()
            for k in ema:
                ema[k].mul_(0.999).add_(P[k].detach(), alpha=0.001)
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times[1:])


def eval_missing_child(B, Ta, n_val, what, replays, warmup):
    """one measurement of --eval_missing (module docstring), in this process"""
    from erc_amd import capi
    from erc_amd.mmin_miss import MISSING_TYPES, MMINMissCollate, MMINMissTrainer
    from erc_amd.synthetic import make_mmin_samples
    from track_mm.mmin_miss import MMINMissParams
    tr = MMINMissTrainer(MMINMissParams().from_args(["--eval_missing"]), "cuda:0")
    tr.model.eval()
    samples = make_mmin_samples(n_val, "val", seed=7, frames=(Ta, Ta))
    groups = [samples[i:i + B] for i in range(0, n_val, B)]
    batches = [tr.prepare_batch(MMINMissCollate(has_miss=False)(g)) for g in groups]
    C, K = tr.model.n_classes, len(MISSING_TYPES)
    cm = torch.zeros(K, C, C, dtype=torch.int64, device="cuda:0")
    sums = torch.zeros(K, dtype=torch.float64, device="cuda:0")

    def plain():
        for b in batches:
            tr.to_logits(b)

    def fused():
        tr.model.begin_missing_pass()
        for b in batches:
            tr.to_logits(b)
            tr.model.score_missing(b["label"], cm, sums)
    res = {"eval_missing": what, "B": B, "Ta": Ta, "n_val": n_val, "batches": len(batches)}
    res["plain_ms"] = statistics.median(event_times(plain, replays, warmup))
    if what == "fused":
        res["fused_ms"] = statistics.median(event_times(fused, replays, warmup))
        res["added_ms"] = res["fused_ms"] - res["plain_ms"]
        res["added_over_plain"] = res["added_ms"] / res["plain_ms"]
        res["zero_scans_per_pass"] = tr.model.zero_scans // (replays + warmup)
    elif what == "naive":
        masked = [[tr.prepare_batch(MMINMissCollate(has_miss=True)([dict(s, missing_type=list(p)) for s in g])) for p in MISSING_TYPES]
                  for g in groups]

        def naive():
            for b, six in zip(batches, masked):
                tr.to_logits(b)
                for m in six:
                    tr.to_logits(m)
        res["naive_ms"] = statistics.median(event_times(naive, replays, warmup))
        res["added_ms"] = res["naive_ms"] - res["plain_ms"]
        res["added_over_plain"] = res["added_ms"] / res["plain_ms"]
    elif what == "kernels":
        capi.start_recording()
        tr.to_logits(batches[0])
        tr.model.score_missing(batches[0]["label"], cm, sums)
        torch.cuda.synchronize()
        rec = capi.stop_recording()
        for name in ("erc_resae_latents", "erc_resae_fwd", "erc_mmin_miss_expand", "erc_mmin_miss_score"):
            entry = [e for e in rec if e[0] == name][-1]
            res[name[4:] + "_ms"] = statistics.median(event_times(lambda: capi.replay(entry), replays, warmup))
        res["latents_rows"], res["fwd_rows"] = K * len(groups[0]), len(groups[0])
        res["latents_over_fwd"] = res["resae_latents_ms"] / res["resae_fwd_ms"]
        res["added_launching_calls_per_batch"] = sum(1 for e in rec[[e[0] for e in rec].index("erc_mmin_miss_expand"):] if capi._launches(e[0]))
    print(json.dumps(res), flush=True)


def eval_missing_parent(args):
    import subprocess
    for B in (int(v) for v in args.batch.split(",")):
        for Ta in (int(v) for v in args.ta.split(",")):
            for what in ("plain", "fused", "naive", "kernels"):
                cmd = [sys.executable, os.path.abspath(__file__), "--eval_missing_child", what, "--batch", str(B), "--ta", str(Ta),
                       "--replays", str(args.replays), "--warmup", str(args.warmup), "--n_val", str(args.n_val)]
                res = subprocess.run(cmd, timeout=600)
                if res.returncode != 0:      # a child that failed: nothing more is started on the GPU
                    raise SystemExit("tools/mmin_miss_bench.py --eval_missing: the %s child (Ta=%d) exited with %d" % (what, Ta, res.returncode))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="32")
    ap.add_argument("--ta", default="100,400")
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--visits", type=int, default=3)
    ap.add_argument("--cpu_steps", type=int, default=1)
    ap.add_argument("--eval_missing", action="store_true", help="time the evaluation under the six missing-modality patterns")
    ap.add_argument("--eval_missing_child", default=None, choices=("plain", "fused", "naive", "kernels"), help=argparse.SUPPRESS)
    ap.add_argument("--n_val", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mmin_miss_bench.py times the step on an MI355X; no GPU is visible (there is no CPU fallback)")
    if args.eval_missing_child:
        return eval_missing_child(int(args.batch), int(args.ta), args.n_val, args.eval_missing_child, args.replays, args.warmup)
    if args.eval_missing:
        return eval_missing_parent(args)
    for B in (int(v) for v in args.batch.split(",")):
        for Ta in (int(v) for v in args.ta.split(",")):
            res = gpu_time(B, Ta, args.replays, args.warmup, args.visits)
            if args.cpu_steps > 0:
                res["cpu16_float64_ms_per_step"] = cpu_time(B, Ta, args.cpu_steps)
                res["speedup_vs_cpu16"] = res["cpu16_float64_ms_per_step"] / res["ms_per_step"]
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
