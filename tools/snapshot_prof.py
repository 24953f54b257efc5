#!/usr/bin/env python3
"""What a device snapshot costs (sn_state_save / sn_state_load, csrc/sechs_snapshot.hip).

One process, on the GPU or not at all.  At `--games` (65 536) games, N = 4, numpy-MT, after a rollout that leaves
the streams mid-round and straddled:
  save         sn_state_save alone (the pipeline already folded: k_snapshot_save), HIP events, median of --reps
  save_after_rollout  the same call right after a 10-step rollout: the pipeline sync (k_pipe_code) is in it
  load         sn_state_load, HIP events around the call; it is [sync] (header read-back, a stream
               synchronise), so the host wall time of the call is given beside it
  rate         bytes moved = twice the blob (every byte read once and written once) over the time, against the
               6.3 TB/s a float4 copy reaches on this part (MI355X_MICROARCH.md)
  get_mt_state the only route before snapshots: per game a device synchronise and three copies, RNG only; timed
               over 256 games and SCALED to --games (labelled so)
  league       BatchedTournament.save / load wall time for a DrunkHamster + MCSAgent(mc_max=20) +
               PUCTAgent(mc_max=20) + DDQN_PRBAgent league (fused=False, train=False) at --slots slots after one round

Usage:  python tools/snapshot_prof.py [--games 65536] [--slots 65536] [--reps 30] [--warmup 5] [--no-league]
        [--out FILE]
(--out: the JSON is also written to FILE, e.g. profiles/snapshot_prof.json; by default it is only printed)
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-6-nimmt_amd"))

HBM_ACHIEVABLE_GBPS = 6300.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def wall(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e6  # us


def summary(ts):
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts), "runs": len(ts)}


def run_env(games, reps, warmup):
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(games, 4, seed=1, rng="numpy")
    dev = env.device
    env.reset()
    env.rollout(23, want_rewards=False, want_done=False)
    n = nat.lib().sn_state_size(env._h)
    blob = torch.empty((n,), dtype=torch.uint8, device=dev)
    L, h = nat.lib(), env._h

    def save():
        nat.check(L.sn_state_save(h, nat.ptr(blob), n, env._stream()), "sn_state_save")

    def load():
        nat.check(L.sn_state_load(h, nat.ptr(blob), n, 0, env._stream()), "sn_state_load")

    out = {"games": games, "num_players": 4, "rng": "numpy", "blob_bytes": n, "bytes_moved": 2 * n}
    save()  # folds the pipeline: the timed saves are k_snapshot_save alone
    ts = [timed(save) for _ in range(warmup + reps)][warmup:]
    out["save"] = summary(ts)
    ts = []
    for r in range(warmup + reps):
        env.rollout(10, want_rewards=False, want_done=False)
        t = timed(save)
        if r >= warmup:
            ts.append(t)
    out["save_after_rollout"] = summary(ts)
    save()
    ts, tw = [], []
    for r in range(warmup + reps):
        t, w = timed(load), wall(load, dev)
        if r >= warmup:
            ts.append(t)
            tw.append(w)
    out["load"], out["load_host_wall"] = summary(ts), summary(tw)
    for k in ("save", "save_after_rollout", "load"):
        out[k]["GBps"] = 2 * n / out[k]["median_us"] / 1e3
        out[k]["share_of_achievable_hbm"] = out[k]["GBps"] / HBM_ACHIEVABLE_GBPS
    env.rollout(10, want_rewards=False, want_done=False)
    sample = min(256, games)

    def old_route():
        for g in range(sample):
            env.get_mt_state(g)

    old_route()
    tw = [wall(old_route, dev) for _ in range(5)]
    out["get_mt_state"] = {"games_timed": sample, "median_us": statistics.median(tw),
                           "scaled_to_games": games, "scaled_us": statistics.median(tw) * games / sample,
                           "note": "SCALED from %d games; RNG state only, no game fields" % sample}
    assert env.pipe_errors() == 0
    env.close()
    return out


def run_league(slots, reps):
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.league import BatchedTournament

    torch.manual_seed(0)
    t = BatchedTournament(slots, 2, 4, seed=3, fused=False, train=False)
    t.add_player("h")
    t.add_player("m", A.MCSAgent(mc_max=20))
    t.add_player("p", A.PUCTAgent(mc_max=20))
    q = A.DDQN_PRBAgent(history_length=64, minibatch=16)
    q.eps = 0.3
    t.add_player("q", q)
    t.play_games(1)
    dev = t.env.device
    out = {"slots": slots, "rounds_played": 1}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "league.pt")
        ts, tl = [], []
        for _ in range(reps):
            ts.append(wall(lambda: t.save(path), dev))
            box = []
            tl.append(wall(lambda: box.append(BatchedTournament.load(path)), dev))
            box[0].close()
            print(f"league save {ts[-1] / 1e6:.2f} s, load {tl[-1] / 1e6:.2f} s", file=sys.stderr, flush=True)
        out["file_bytes"] = os.path.getsize(path)
    out["save_wall"], out["load_wall"] = summary(ts), summary(tl)
    t.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--league-reps", type=int, default=3)
    ap.add_argument("--no-league", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.reps < 20:
        sys.exit("snapshot_prof: --reps >= 20 (the figures are medians)")
    if not torch.cuda.is_available():
        sys.exit("snapshot_prof: no GPU -- times are taken on the device or not at all")
    result = {"device": torch.cuda.get_device_name(0), "hbm_achievable_GBps": HBM_ACHIEVABLE_GBPS,
              "env": run_env(args.games, args.reps, args.warmup)}

    def emit():
        text = json.dumps(result, indent=1)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return text

    emit()  # the league part takes minutes at 65 536 slots: the handle's figures are on disk before it starts
    print("handle part done", file=sys.stderr, flush=True)
    if not args.no_league:
        result["league"] = run_league(args.slots, args.league_reps)
    print(emit())


if __name__ == "__main__":
    main()
