#!/usr/bin/env python
"""Back-end chain of one step from a rocprofv3 kernel trace (stats_kernel_trace.csv): per-kernel gap / duration on the queue that
carries be_marg_kernel (or be_marg_pre / be_marg_alg), between two consecutive marginalisation launches.    python tools/trace_chain.py trace.csv [step_from_end] [-v]
-v: every launch of the step in order (duration, gap before it)."""
import collections
import csv
import sys

rows = list(csv.DictReader(open([a for a in sys.argv[1:] if a != "-v"][0])))
for r in rows:
    r["s"] = int(r["Start_Timestamp"]); r["e"] = int(r["End_Timestamp"])
rows.sort(key=lambda r: r["s"])
qs = collections.defaultdict(list)
for r in rows:
    qs[r["Queue_Id"]].append(r)
verbose = "-v" in sys.argv
args = [a for a in sys.argv[1:] if a != "-v"]
back = int(args[1]) if len(args) > 1 else 2
for q, l in sorted(qs.items()):
    # (VIO_MARG_SPLIT: be_marg_pre + be_marg_alg -- a step ends with the second)
    ms = [i for i, r in enumerate(l) if r["Kernel_Name"].startswith("be_marg") and not r["Kernel_Name"].startswith("be_marg_pre")]
    if len(ms) < back + 2:
        continue
    seg = l[ms[-back - 1] + 1:ms[-back] + 1]
    prev = l[ms[-back - 1]]["e"]
    agg = collections.OrderedDict()
    gaps = 0.0
    for r in seg:
        name = r["Kernel_Name"].split("(")[0]
        gap = max(r["s"] - prev, 0) / 1e3
        a = agg.setdefault(name, [0, 0.0, 0.0])
        a[0] += 1; a[1] += (r["e"] - r["s"]) / 1e3; a[2] += gap
        gaps += gap
        if verbose:
            print("      %-24s %8.1f us   gap %6.1f us" % (name, (r["e"] - r["s"]) / 1e3, gap))
        prev = r["e"]
    print("queue %s: step span %.3f ms, gaps %.3f ms" % (q, (seg[-1]["e"] - l[ms[-back - 1]]["e"]) / 1e6, gaps / 1e3))
    for name, a in agg.items():
        print("   %-24s x%-3d busy %8.1f us  (avg %6.1f)  gaps before %7.1f us" % (name, a[0], a[1], a[1] / a[0], a[2]))
    # VIO_MARG_SPLIT: be_ingest / ps_setup of the step run on another queue, beside the be_marg_alg launch that ends the previous step
    alg = l[ms[-back - 1]]
    if alg["Kernel_Name"].startswith("be_marg_alg"):
        for q2, l2 in sorted(qs.items()):
            for r in l2:
                if q2 != q and alg["s"] <= r["s"] <= seg[-1]["e"] and r["Kernel_Name"].startswith(("be_ingest", "ps_setup")):
                    print("   queue %s %-20s %6.1f us: starts %+8.1f us after be_marg_alg started, ends %+8.1f us after it ended" %
                          (q2, r["Kernel_Name"].split("(")[0][:20], (r["e"] - r["s"]) / 1e3, (r["s"] - alg["s"]) / 1e3, (r["e"] - alg["e"]) / 1e3))
