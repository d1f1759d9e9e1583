#!/usr/bin/env python3
"""Where the work items of the bf16 weight-gradient launch (csrc/wgrad_bf16.hip) spend their time: replays the bench
workload's launch with phase stamps on for one work item at a time -- every split of the first and of the last tile of
every record -- and prints, per record, when each phase was reached (us after the item's own start) next to when the item
started and ended relative to the start of work item 0 (the dispatch spread; bf16 forms only).

    python tools/wgrad_stamps.py [--batch 32] [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import struct
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

ENTRIES = ("erc_wgrad_bf16", "erc_wgrad_bf16_wide", "erc_wgrad_bf16_adam", "erc_wgrad_split", "erc_wgrad_split_adam")
DESC = "<QQQQQQQ14i"     # W2Desc (csrc/wgrad_bf16.hip)
# (slot, column): the item's own slots 1..5, then the slots its tile's splits write behind the wait (fused optimizer) or the
# tile's last arriver writes (plain form)
PHASES_ADAM = ((1, "loads"), (2, "K loop"), (3, "slab out"), (4, "drained"), (5, "splits seen"), (9, "sums"), (13, "quad 0"),
               (11, "+shadows"), (12, "quad 1"), (10, "end"))
PHASES_PLAIN = ((1, "loads"), (2, "K loop"), (3, "slab out"), (4, "drained"), (5, "ticket"), (9, "sums"), (10, "end"))


def records(table, n_desc):
    raw = bytes(table.cpu().numpy().tobytes())
    out = []
    for t in range(n_desc):
        f = struct.unpack_from(DESC, raw, t * struct.calcsize(DESC))
        keys = ("lda", "ldb", "ldc", "M", "N", "K", "ct", "cvec", "splits", "tiles_n", "item_base", "n_items", "tile_base", "kind")
        d = dict(zip(keys, f[7:]))
        d["gather"] = f[5] != 0
        out.append(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--compute", default="bf16", help="bf16 | f32x2 | f32x3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None, help="write the table here as well")
    a = ap.parse_args()
    from bench import synthetic_batch
    from erc_amd import capi, engine
    import track_mm.cogmen as plugin
    params = plugin.ParamsType().from_args(["--dataset=iemocap-cogmen-sbert-6", "--modality=atv", "--compute=" + a.compute])
    tr = plugin.COGMENTrainer(params, "cuda:0")
    batch = tr.prepare_batch(synthetic_batch(params, a.batch, 110, seed=1))
    for _ in range(3):
        tr.train_step(batch)
    caches, flush = [], engine.GemmPlanner.flush_wgrads_bf16     # the launch's table lives in the planner's cache

    def spy(self, cache):
        caches.append(cache)
        return flush(self, cache)
    engine.GemmPlanner.flush_wgrads_bf16 = spy
    capi.start_recording()
    tr.train_step(batch)
    rec = capi.stop_recording()
    engine.GemmPlanner.flush_wgrads_bf16 = flush
    torch.cuda.synchronize()
    call = [e for e in rec if e[0] in ENTRIES][0]
    split = "split" in call[0]
    n_desc, bases, n_items = call[1][2 if split else 1], call[1][3 if split else 2], call[1][4 if split else 3]
    recs = records(caches[0]["w16_table"], n_desc)
    adam = call[0].endswith("adam")
    phases = PHASES_ADAM if adam else PHASES_PLAIN
    has_ref = not split       # slot 14 (start of work item 0) is written by the bf16 forms only
    print("%s: %d work items, %d records" % (call[0], n_items, n_desc))
    st = torch.zeros(16, dtype=torch.int64, device="cuda:0")

    def measure(item):
        rows = []
        capi.wgrad_bf16_set_stamps(st, item)
        for _ in range(a.reps):
            st.zero_()
            capi.replay(call)
            torch.cuda.synchronize()
            rows.append(st.cpu().double())
        capi.wgrad_bf16_set_stamps(None)
        s = torch.stack(rows)
        rel = ((s - s[:, :1]) * 0.01).median(0).values          # us after the item's own start
        start = float(((s[:, 0] - s[:, 14]) * 0.01).median()) if has_ref else float("nan")
        return rel, start

    out = []
    for di, d in enumerate(recs):
        base = int(bases[di])
        if d["kind"] == 1:
            _, start = measure(base)
            print("== record %d: finished range of %d elements, work item %d: starts at %6.2f us" % (di, d["M"], base, start))
            out.append(dict(record=di, kind=1, item=base, start=start))
            continue
        wide = call[0].endswith("wide")
        n_tiles = d["n_items"] // d["splits"] if wide else d["tiles_n"]
        print("== record %d: M %d, N %d, K %d, ct %d, %s%d tile%s x %d splits = work items %d..%d" % (
            di, d["M"], d["N"], d["K"], d["ct"], "gathered B, " if d["gather"] else "", n_tiles, "s" if n_tiles > 1 else "",
            d["splits"], base, base + d["n_items"] - 1))
        print("   %4s %4s %5s | %7s | %s | %7s" % ("item", "tile", "split", "start", " ".join("%11s" % p[1] for p in phases), "ends at"))
        for tile in sorted({0, n_tiles - 1}):
            for sp in range(d["splits"]):
                item = base + tile * d["splits"] + sp
                rel, start = measure(item)
                vals = [float(rel[k]) for k, _ in phases]
                print("   %4d %4d %5d | %7.2f | %s | %7.2f" % (item, tile, sp, start, " ".join("%11.2f" % v for v in vals), start + vals[-1]))
                out.append(dict(record=di, item=item, tile=tile, split=sp, gather=d["gather"], start=start,
                                phases={p[1]: v for p, v in zip(phases, vals)}, end=start + vals[-1]))
    if has_ref:
        prod = [o for o in out if "end" in o]
        last = max(prod, key=lambda o: o["end"])
        print("dispatch spread of the measured items: %.2f us; last to end: work item %d of record %d at %.2f us after work item 0 started"
              % (max(o["start"] for o in out) - min(o["start"] for o in out), last["item"], last["record"], last["end"]))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(entry=call[0], n_items=n_items, items=out), fh, indent=1)


if __name__ == "__main__":
    main()
