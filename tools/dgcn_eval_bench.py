#!/usr/bin/env python3
"""DialogueGCN over whole epochs -- training epoch + the test epoch that follows it -- as train_mm.py runs them with
``--module=dgcn --device_collate --resident``:

  host      no further flag: the default test loop (device-collated batches, eager ``to_logits``, a synchronisation per
            batch, eight sklearn calls) -- the baseline
  device    ``--resident_eval``: trainer.ResidentEval (graph replays over the resident test store, the confusion matrix
            counted by erc_dgcn_tail_eval, one device -> host copy per epoch)

Two synthetic configurations at B = 32: ``meld`` (the MELD-sized 7-way atv bf16 config, BASELINE.json configs[4]: 1039 / 280
dialogues of 1 .. 33 utterances) and ``iemocap`` (IEMOCAP-6 f32, 120 / 31 dialogues of 20 .. 110 utterances, two speakers;
--relation_space=False runs the basis-space path capacity mode covers).  The modes alternate, each twice by default, every
run in a fresh process under a time limit of its own.  The parent stamps every epoch line as it arrives: a PAIR is the time
between two consecutive epoch lines (training epoch + test epoch + the line itself), the training epoch is what
train_mm.py timed between device synchronisations (utterances / train_utt_per_s), the test epoch is the difference
(``device`` also reports the ``test_s`` train_mm.py measured itself).  One JSON line per run with the median and min .. max
over the epochs after the first (the first pays one eager step + capture per bucket), then one line per config with the
ratios of the medians of its last host and device runs.  The first run that fails or runs into its time limit ends the
tool with a non-zero exit code: nothing more is started on the GPU after it.

    python tools/dgcn_eval_bench.py [--epochs 12] [--configs meld,iemocap] [--modes host,device,host,device] [--timeout 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CONFIGS = {
    "meld": ["--dataset=meld-mmgcn-7", "--modality=atv", "--compute=bf16", "--loss_weights=False", "--n_train=1039", "--n_test=280"],
    "iemocap": ["--dataset=iemocap-cogmen-6", "--compute=f32", "--relation_space=False", "--n_train=120", "--n_test=31"],
}
MODES = {"host": [], "device": ["--resident_eval"]}
SEED = 1


def utterances(flags):
    """(#training, #test utterances) of the synthetic split train_mm.py draws for these flags (trainer.load_dialogues, rank 0)"""
    from erc_amd.trainer import load_dialogues
    from track_mm.dgcn import DGCNParams
    train, test = load_dialogues(DGCNParams().from_args(flags))
    return sum(len(d["label"]) for d in train), sum(len(d["label"]) for d in test)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(config, mode, epochs, batch, timeout):
    flags = ["--module=dgcn", "--device_collate", "--resident", "--seed=%d" % SEED, "--epoch=%d" % epochs,
             "--train.batch_size=%d" % batch, "--test.batch_size=%d" % batch] + CONFIGS[config] + MODES[mode]
    args = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.join(REPO, "train_mm.py")] + flags
    n_train, n_test = utterances([f for f in flags if not f.startswith("--module")])
    head = {"tool": "dgcn_eval_bench", "config": config, "mode": mode, "batch": batch, "train_utterances": n_train,
            "test_utterances": n_test}
    proc = subprocess.Popen(args, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    stamps, lines, tail = [], [], []
    for raw in proc.stdout:                      # (ends when the child exits or its time limit closes the pipe)
        now = time.perf_counter()
        tail = (tail + [raw])[-8:]
        if raw.startswith("{") and "train_utt_per_s" in raw:
            stamps.append(now)
            lines.append(json.loads(raw))
    rc = proc.wait()
    if rc != 0 or len(lines) != epochs or epochs < 2:
        return dict(head, error="%d epoch lines of %d; last output: %s" % (len(lines), epochs, "".join(tail)[-600:]), returncode=rc)
    pair = [stamps[e] - stamps[e - 1] for e in range(1, epochs)]
    train = [n_train / lines[e]["train_utt_per_s"] for e in range(1, epochs)]
    test = [p - t for p, t in zip(pair, train)]
    rec = dict(head, epochs=epochs, epochs_measured=epochs - 1, train_s=spread(train), test_s=spread(test), pair_s=spread(pair),
               acc_last=lines[-1]["test"]["acc"], graph_replays=lines[-1]["graph_replays"])
    if "test_s" in lines[-1]:
        rec["test_s_reported"] = spread([l["test_s"] for l in lines[1:]])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=12)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--configs", default="meld,iemocap")
    ap.add_argument("--modes", default="host,device,host,device")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per run")
    a = ap.parse_args()
    for config in a.configs.split(","):
        recs = {}
        for mode in a.modes.split(","):
            rec = recs[mode] = run(config, mode, a.epochs, a.batch, a.timeout)
            print(json.dumps(rec), flush=True)
            if "error" in rec:
                # a run that failed (abort, fault, time limit) may have left the card in a bad state: nothing more is started
                raise SystemExit("dgcn_eval_bench: %s / %s exited with %s; stopping" % (config, mode, rec["returncode"]))
        if "host" in recs and "device" in recs:
            h, d = recs["host"], recs["device"]
            print(json.dumps({"tool": "dgcn_eval_bench", "config": config,
                              "test_epoch_host_over_device": h["test_s"]["median"] / d["test_s"]["median"],
                              "pair_host_over_device": h["pair_s"]["median"] / d["pair_s"]["median"],
                              "acc_last_host": h["acc_last"], "acc_last_device": d["acc_last"]}), flush=True)


if __name__ == "__main__":
    main()
