#!/usr/bin/env python3
"""Timeline of a twist group of the decode-ahead headline step from a rocprofv3
--kernel-trace csv (diagnostics; tools/group_trace.py has the per-position
k_play view): per group, relative to the start of its first k_play launch, when
the K play launches end, when the steady twist (k_mt_ahead<false, ..>) and the
k_decode beside it start and end, the gap before the first launch and the
period to the next group.  Prints the mean and the median over the steady
groups.  With SN_OPT_PLAY_GROUP 1 and whole-group calls a group is one launch:
pass K = 1.

usage: group_timeline.py kernel_trace.csv K
"""
import csv
import json
import sys
from statistics import mean, median


def main():
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
                  for r in csv.DictReader(open(sys.argv[1])))
    K = int(sys.argv[2])
    plays = [r for r in rows if "k_play" in r[2]]
    twists = [r for r in rows if "k_mt_ahead<false" in r[2]]
    decodes = [r for r in rows if "k_decode" in r[2]]
    groups = []  # (first play launch, twist, decode): a twist belongs to the last launch that started before it
    for t in twists:
        i = max((k for k, p in enumerate(plays) if p[0] <= t[0]), default=None)
        if i is None or i + K > len(plays):
            continue
        # the decode enqueued beside it: the first to start from 20 us before the launch on
        d = min((x for x in decodes if x[0] >= plays[i][0] - 20000), key=lambda x: x[0], default=None)
        groups.append((i, t, d))
    out = []
    for n, (i, t, d) in enumerate(groups[3:-1], 3):  # skip the pipeline's start
        p0 = plays[i][0]
        g = {"period": plays[groups[n + 1][0]][0] - p0, "gap_before": p0 - plays[i - 1][1],
             "play_busy": sum(plays[k][1] - plays[k][0] for k in range(i, i + K)), "play_end": plays[i + K - 1][1] - p0,
             "twist_start": t[0] - p0, "twist_end": t[1] - p0, "twist_dur": t[1] - t[0]}
        if d:
            g.update(dec_start=d[0] - p0, dec_end=d[1] - p0, dec_dur=d[1] - d[0])
        for k in range(K):
            g[f"play{k}_dur"] = plays[i + k][1] - plays[i + k][0]
        out.append(g)
    if not out:
        print(json.dumps({"plays": len(plays), "twists": len(twists)}))
        return
    keys = list(out[0])
    print(json.dumps({"groups": len(out), "K": K, "unit": "us",
                      "mean": {k: round(mean(g[k] for g in out if k in g) / 1e3, 2) for k in keys},
                      "median": {k: round(median(g[k] for g in out if k in g) / 1e3, 2) for k in keys}}, indent=1))


if __name__ == "__main__":
    main()
