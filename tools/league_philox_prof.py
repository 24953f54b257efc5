#!/usr/bin/env python3
"""A mixed league on numpy-MT streams against the same league on Philox streams
(DESIGN.md 4e): whole rounds, the checkpoint, and -- from kernel traces taken in
runs of their own -- the MCS search kernels per dispatch.

One process, 65 536 slots, players 2..4, roster DrunkHamster x 3 +
MCSAgent(10, 100) x 2, training off.  After a warm-up the two leagues play
whole rounds in turn, a HIP event pair around each play_games(1); medians and
min-max over `--rounds`.  The numpy leg is the yardstick: the unchanged
reference-exact league on the same GPU in the same run.  Then each league is
saved once (BatchedTournament.save: file size, wall time).

Usage:  python tools/league_philox_prof.py [--slots 65536] [--rounds 10] [--warmup 2]
        [--leg both|numpy|philox] [--kernel-stats DIR] [--out profiles/league_philox_ab.json]
--leg numpy|philox plays that leg alone (no checkpoint), for a kernel trace of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/numpy -- \\
      python tools/league_philox_prof.py --leg numpy --rounds 2 --warmup 1
--kernel-stats DIR: fold the *kernel_stats.csv found under DIR/numpy and DIR/philox into the result.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-6-nimmt_amd"))

LEAGUE_KERNELS = ("k_league_mcs", "k_league_step", "k_reset")


def make(rng, slots):
    from rl_6_nimmt.agents import DrunkHamster, MCSAgent
    from rl_6_nimmt.league import BatchedTournament

    t = BatchedTournament(slots, 2, 4, seed=17, rng=rng, fused=False, train=False)
    for i in range(3):
        t.add_player(f"h{i}", DrunkHamster())
    for i in range(2):
        t.add_player(f"m{i}", MCSAgent(mc_per_card=10, mc_max=100))
    return t


def timed_round(t):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t.play_games(1)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)  # ms


def timed_save(t, path):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t.save(path)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return {"file_bytes": os.path.getsize(path), "wall_s": wall}


def kernel_stats(root, leg):
    """the league kernels' rows of a rocprofv3 --stats CSV under root/leg"""
    out = {}
    for path in glob.glob(os.path.join(root, leg, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                if not any(k in name for k in LEAGUE_KERNELS):
                    continue
                short = name.split("(")[0].replace("void ", "")
                out[short] = {"calls": int(row["Calls"]), "total_ms": int(row["TotalDurationNs"]) / 1e6,
                              "mean_us": float(row["AverageNs"]) / 1e3, "min_us": int(row["MinNs"]) / 1e3,
                              "max_us": int(row["MaxNs"]) / 1e3, "percent_of_gpu_time": float(row["Percentage"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg", default="both", choices=("both", "numpy", "philox"))
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("league_philox_prof: no GPU -- times are taken on the device or not at all")
    from rl_6_nimmt import _native as nat

    legs = ("numpy", "philox") if args.leg == "both" else (args.leg,)
    leagues = {leg: make(leg, args.slots) for leg in legs}
    times = {leg: [] for leg in legs}
    for r in range(args.warmup + args.rounds):
        for leg in legs:  # the legs alternate
            ms = timed_round(leagues[leg])
            if r >= args.warmup:
                times[leg].append(ms)
    result = {"device": torch.cuda.get_device_name(), "slots": args.slots, "players": [2, 4],
              "roster": "DrunkHamster x 3 + MCSAgent(10, 100) x 2", "rounds": args.rounds, "warmup": args.warmup}
    for leg in legs:
        t, ms = leagues[leg], times[leg]
        mode = nat.SN_RNG_NUMPY_MT if leg == "numpy" else nat.SN_RNG_PHILOX
        result[leg] = {"round_ms_median": statistics.median(ms), "round_ms_min": min(ms), "round_ms_max": max(ms),
                       "round_ms": ms, "q6_slot_rounds": t.q6_slot_rounds,
                       "state_bytes": int(nat.lib().sn_state_bytes(args.slots, 4, mode, 1, None, None))}
        if args.leg == "both":
            t.clear_records()  # the checkpoint of a league that folds its records as it goes: the handle dominates
            with tempfile.TemporaryDirectory() as d:
                result[leg]["save"] = timed_save(t, os.path.join(d, "league.pt"))
        if args.kernel_stats:
            result[leg]["kernels"] = kernel_stats(args.kernel_stats, leg)
    if args.leg == "both":
        n, p = result["numpy"], result["philox"]
        result["philox_over_numpy_round"] = p["round_ms_median"] / n["round_ms_median"]
        result["numpy_round_spread_ms"] = n["round_ms_max"] - n["round_ms_min"]
        result["state_bytes_ratio"] = n["state_bytes"] / p["state_bytes"]
        result["save_file_ratio"] = n["save"]["file_bytes"] / p["save"]["file_bytes"]
    for t in leagues.values():
        t.close()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
