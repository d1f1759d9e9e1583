#!/usr/bin/env python3
"""Reads a rocprofv3 --kernel-trace CSV of a COGMEN bench run and prints, for the steady state, the median duration of each
of the step's kernels and the idle time of the queue before it (end of the previous kernel -> its start).  The idle time
before the projection kernel is the gap BETWEEN two steps.  usage: trace_gaps.py <..._kernel_trace.csv> [json out]"""
import csv
import json
import statistics
import sys

rows = []
with open(sys.argv[1]) as fh:
    for r in csv.DictReader(fh):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
STEP = ("cogmen_project_graph_kernel", "cogmen_fwd_tile_kernel", "head_fused_kernel", "cogmen_bwd_tile_kernel", "wgrad_bf16_kernel")
short = lambda name: next((s for s in STEP if s in name), None)
dur, gap = {s: [] for s in STEP}, {s: [] for s in STEP}
for i in range(1, len(rows)):
    k, prev = short(rows[i][2]), short(rows[i - 1][2])
    # a kernel of the step directly behind its predecessor in the step (the projection: behind the previous step's last)
    if k is None or prev != STEP[STEP.index(k) - 1]:
        continue
    dur[k].append(rows[i][1] - rows[i][0])
    gap[k].append(rows[i][0] - rows[i - 1][1])
out = {}
for s in STEP:
    if not dur[s]:
        continue
    d, g = sorted(dur[s]), sorted(gap[s])
    out[s] = {"n": len(d), "dur_us_median": statistics.median(d) / 1e3, "dur_us_p10": d[len(d) // 10] / 1e3, "dur_us_p90": d[len(d) * 9 // 10] / 1e3,
              "idle_before_us_median": statistics.median(g) / 1e3, "idle_before_us_p10": g[len(g) // 10] / 1e3,
              "idle_before_us_p90": g[len(g) * 9 // 10] / 1e3}
    print("%-30s n=%5d  duration %6.2f us (p10 %6.2f, p90 %6.2f)   idle before it %6.2f us (p10 %6.2f, p90 %6.2f)" % (
        s, len(d), out[s]["dur_us_median"], out[s]["dur_us_p10"], out[s]["dur_us_p90"], out[s]["idle_before_us_median"],
        out[s]["idle_before_us_p10"], out[s]["idle_before_us_p90"]))
print("sum of medians: kernels %.2f us, idle %.2f us" % (sum(v["dur_us_median"] for v in out.values()),
                                                        sum(v["idle_before_us_median"] for v in out.values())))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as fh:
        json.dump(out, fh, indent=1)
