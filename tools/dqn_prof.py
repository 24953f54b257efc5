#!/usr/bin/env python3
"""The batched DQN kernels (sn_dqn_* in csrc/sechs_agents.hip, sn_per_gather in
csrc/sechs_replay.hip) against their PyTorch-ROCm forms on the same inputs,
and one league round with a DDQN_PRBAgent seat by phase.

One process; every call is timed with device events after a warm-up; the native
and the torch leg of an operation alternate; medians over `--reps` with min-max.
  D = 16 384 deciders (4 096 games x 4 seats), one episode = 163 840 rows,
  a 65 536-row minibatch, a 2^20-slot ring of 112-byte rows.
Yardsticks:  obs     env.obs() + seat indexing + .float()
             select  legal mask + argmax + where (torch.rand for the draws)
             pack    slices / cat / view (dqn.pack_rows_host)
             unpack  slicing + .float() (dqn.unpack_rows_host)
             target  max / argmax + gather + mul + add (dqn.bellman_target_host)
             gather  index_select on a ring tensor
             select_duel  dqn.duelling_q_host on the [A | V | pad] head output (stride 112), then
                          sn_dqn_select on the materialised Q
             pack_nstep   dqn.pack_rows_nstep_host (n = 3, gamma = 0.99)
Algorithmic bytes per call: BYTES below.

--noisy: instead, a league round with a Noisy_D3QN_PRB_NStep seat against one
with a D3QN_PRB_NStep seat (both n_steps = 3; the same slots, seeds and
opponents): two tournaments in this process, their rounds alternating, the
phases of every round from device events, medians over `--reps` rounds; then
the noisy decide's four steps per layer (scale, plain GEMM, sigma GEMM,
combine) one by one on a decision batch of the league's size.

Usage:  python tools/dqn_prof.py [--reps 30] [--warmup 5] [--no-league] [--slots 65536] [--out dqn_prof.json]
        python tools/dqn_prof.py --noisy [--reps 10] [--slots 65536] [--out dqn_noisy_prof.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-6-nimmt_amd"))

GAMES, SEATS, T, MINIBATCH, CAPACITY = 4096, 4, 10, 65536, 1 << 20
D = GAMES * SEATS
# what each call has to move: the device state it reads (3 hand + 8 board words per decision) or its inputs, and its outputs
BYTES = {"obs": D * (44 + 48 + 192), "select": D * (12 + 10 * 4 + 12), "pack": T * D * (96 + 8 + 112),
         "unpack": MINIBATCH * (112 + 2 * 192 + 16), "target": MINIBATCH * (2 * 416 + 12),
         "gather": MINIBATCH * (4 + 2 * 112), "select_duel": D * (12 + 105 * 4 + 12),
         "pack_nstep": T * D * (96 + 8 + 112)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def kernel_legs():
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.dqn import (BatchedDQN, bellman_target_host, duelling_q_host, gamma_powers, pack_rows_host,
                                pack_rows_nstep_host, unpack_rows_host)
    from rl_6_nimmt.replay import DevicePER
    from rl_6_nimmt.utils.nets import MultiHeadedMLP
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    L = nat.lib()
    env = VecSechsNimmtEnv(GAMES, SEATS, seed=1)
    dev = env.device
    env.reset()
    net = MultiHeadedMLP(47, (64,), (104,), torch.nn.ReLU(), (None,)).to(dev)
    eng = BatchedDQN(env, net, capacity=CAPACITY, net_dtype=torch.float32, eps_func=lambda e: 0.1)
    st = env._stream()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    q = eng._params(10)
    ref = ctypes.byref(q)
    flat = torch.arange(D, device=dev)

    obs_i8 = torch.empty((D, 48), dtype=torch.int8, device=dev)
    states = torch.empty((D, 48), dtype=torch.float32, device=dev)

    def obs_native():
        nat.check(L.sn_dqn_obs(env._h, ref, nat.ptr(obs_i8), nat.ptr(states), 0, st), "sn_dqn_obs")

    def obs_torch():
        o = env.obs().reshape(D, 47)[flat]
        return o, o.float()

    qv = torch.randn((D, 104), device=dev, generator=g)
    actions = torch.zeros((GAMES, SEATS), dtype=torch.int32, device=dev)
    index = torch.zeros((D,), dtype=torch.int32, device=dev)
    value = torch.zeros((D,), dtype=torch.float32, device=dev)
    hands = env.hands().reshape(D, 10).long()
    rows_d = flat[:, None]

    def select_native():
        nat.check(L.sn_dqn_select(env._h, ref, nat.ptr(qv), 104, 0.1, nat.ptr(actions), nat.ptr(index), nat.ptr(value),
                                  st), "sn_dqn_select")

    def select_torch():
        legal = torch.zeros((D, 104), dtype=torch.bool, device=dev)
        legal[rows_d, hands] = True
        masked = torch.where(legal, qv, torch.full_like(qv, -1e8))
        best, greedy = masked.max(dim=1)
        u = torch.rand((2, D), device=dev)
        rnd = hands.gather(1, (u[1] * 10).long()[:, None])[:, 0]
        explore = u[0] <= 0.1
        return torch.where(explore, rnd, greedy), torch.where(explore, torch.full_like(best, -1.0), best)

    heads = torch.randn((D, 112), device=dev, generator=g)  # [A | V | pad], as the engine's padded head GEMM leaves it

    def select_duel_native():
        nat.check(L.sn_dqn_select_duel(env._h, ref, nat.ptr(heads), 112, 104, 0, 0.1, nat.ptr(actions), nat.ptr(index),
                                       nat.ptr(value), st), "sn_dqn_select_duel")

    def select_duel_torch():
        qd = duelling_q_host(heads[:, 104:105], heads[:, :104])
        nat.check(L.sn_dqn_select(env._h, ref, nat.ptr(qd), qd.stride(0), 0.1, nat.ptr(actions), nat.ptr(index),
                                  nat.ptr(value), st), "sn_dqn_select")

    ep_obs = torch.randint(0, 104, (T + 1, D, 48), dtype=torch.int8, device=dev, generator=g)
    ep_obs[..., 47] = 0
    ep_act = torch.randint(0, 104, (T, D), dtype=torch.int32, device=dev, generator=g)
    ep_rew = -torch.randint(0, 40, (T, D), dtype=torch.int32, device=dev, generator=g)
    ep_rows = torch.empty((T * D, 112), dtype=torch.uint8, device=dev)

    def pack_native():
        nat.check(L.sn_dqn_pack(T, D, nat.ptr(ep_obs), nat.ptr(ep_act), nat.ptr(ep_rew), nat.ptr(ep_rows), st),
                  "sn_dqn_pack")

    gpow = nat.SnDqnGpow()
    gpow.v[:] = gamma_powers(0.99)

    def pack_nstep_native():
        nat.check(L.sn_dqn_pack_nstep(T, D, 3, gpow, nat.ptr(ep_obs), nat.ptr(ep_act), nat.ptr(ep_rew), nat.ptr(ep_rows),
                                      st), "sn_dqn_pack_nstep")

    per = DevicePER(CAPACITY, 112, device=dev)
    ring = torch.randint(0, 256, (CAPACITY, 112), dtype=torch.uint8, device=dev, generator=g)
    for at in range(0, CAPACITY, 1 << 16):
        per.store(ring[at: at + (1 << 16)])
    slots = torch.randint(0, CAPACITY, (MINIBATCH,), dtype=torch.int32, device=dev, generator=g)
    slots64 = slots.long()
    pack_native()
    batch = ep_rows[:MINIBATCH].clone()

    ql = torch.randn((MINIBATCH, 104), device=dev, generator=g)
    qt = torch.randn((MINIBATCH, 104), device=dev, generator=g)
    reward = -torch.randint(0, 40, (MINIBATCH,), device=dev, generator=g).float()
    not_done = (torch.rand((MINIBATCH,), device=dev, generator=g) > 0.1).float()

    return {"obs": (obs_native, obs_torch),
            "select": (select_native, select_torch),
            "pack": (pack_native, lambda: pack_rows_host(ep_obs, ep_act, ep_rew)),
            "unpack": (lambda: eng.unpack(batch), lambda: unpack_rows_host(batch)),
            "target": (lambda: eng.bellman_target(ql, qt, reward, not_done),
                       lambda: bellman_target_host(ql, qt, reward, not_done, eng.gamma)),
            "gather": (lambda: per.gather(slots), lambda: ring.index_select(0, slots64)),
            "select_duel": (select_duel_native, select_duel_torch),
            "pack_nstep": (pack_nstep_native, lambda: pack_rows_nstep_host(ep_obs, ep_act, ep_rew, 3, 0.99))}, \
        (env, eng, per)


def league_round(slots, rounds):
    from rl_6_nimmt.agents import DDQN_PRBAgent, DrunkHamster
    from rl_6_nimmt.league import BatchedTournament

    torch.manual_seed(0)
    t = BatchedTournament(slots, 2, 4, seed=1, train=True, fused=False)
    for name, agent in (("R0", DrunkHamster()), ("R1", DrunkHamster()), ("DDQN_PRB", DDQN_PRBAgent(history_length=1000)),
                        ("R2", DrunkHamster())):
        t.add_player(name, agent)
    t.play_games(1)  # warm-up: allocations, the first GEMM plans, the optimiser state
    t.phase_timing = True
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t.play_games(rounds)
    b.record()
    b.synchronize()
    eng = t.engines["DDQN_PRB"]
    out = {"slots": slots, "rounds": rounds, "round_ms": a.elapsed_time(b) / rounds,
           "phase_ms_per_round": {k: v / rounds for k, v in t.phase_ms.items()},
           "phase_host_ms_per_round": {k: v / rounds for k, v in t.phase_host_ms.items()},
           "minibatch": eng.minibatch, "updates": eng.updates, "capacity": eng.capacity, "replay_len": len(eng.replay),
           "optimizer_steps": t.optimizer_steps, "pipe_errors": t.env.pipe_errors()}
    t.close()
    return out


def noisy_rounds(slots, reps, warmup):
    """the noisy seat's round against the plain seat's, rounds alternating"""
    from rl_6_nimmt.agents import D3QN_PRB_NStep, DrunkHamster, Noisy_D3QN_PRB_NStep
    from rl_6_nimmt.league import BatchedTournament

    seats = {"noisy": Noisy_D3QN_PRB_NStep, "plain": D3QN_PRB_NStep}
    leagues = {}
    for key, cls in seats.items():
        torch.manual_seed(0)
        t = BatchedTournament(slots, 2, 4, seed=1, train=True, fused=False)
        for name, agent in (("R0", DrunkHamster()), ("R1", DrunkHamster()), ("Q", cls(history_length=1000, n_steps=3)),
                            ("R2", DrunkHamster())):
            t.add_player(name, agent)
        t.play_games(1)  # warm-up: allocations, the first GEMM plans, the optimiser state
        t.phase_timing = True
        leagues[key] = t
    rounds = {key: [] for key in seats}
    for r in range(warmup + reps):
        for key in (("noisy", "plain") if r % 2 == 0 else ("plain", "noisy")):
            t = leagues[key]
            t.phase_ms, t.phase_host_ms = {}, {}
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t.play_games(1)
            b.record()
            b.synchronize()
            if r >= warmup:
                rounds[key].append(dict(t.phase_ms, round=a.elapsed_time(b)))
    out = {"slots": slots, "reps": reps, "net_dtype": str(leagues["noisy"].net_dtype)}
    for key, t in leagues.items():
        eng = t.engines["Q"]
        phases = {k: [r[k] for r in rounds[key]] for k in rounds[key][0]}
        out[key] = {"agent": seats[key].__name__,
                    "phase_ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in phases.items()},
                    "deciders_last_round": int(eng.D), "minibatch": eng.minibatch, "updates": eng.updates,
                    "pipe_errors": t.env.pipe_errors()}
        t.close()
    dec = {key: out[key]["phase_ms"]["decide Q"]["median"] for key in seats}
    out["decide_ms_noisy_over_plain"] = dec["noisy"] / dec["plain"]
    return out


def noisy_steps(deciders, reps, warmup, dtype=torch.bfloat16):
    """the four steps of every layer of a noisy duelling decide, each timed on its own (us, medians)"""
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.dqn import BatchedDQN, noisy_tag
    from rl_6_nimmt.utils.nets import DuellingDQNNet, NoisyFactorizedLinear
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    games = deciders // SEATS
    env = VecSechsNimmtEnv(games, SEATS, seed=1)
    dev = env.device
    env.reset()
    torch.manual_seed(0)
    net = DuellingDQNNet(47, (64,), 104, torch.nn.ReLU(), linear=NoisyFactorizedLinear, init_sigma=0.5).to(dev)
    eng = BatchedDQN(env, net, capacity=1 << 10, net_dtype=dtype)
    dn, n = eng.sync_net(), games * SEATS
    L, st, q = nat.lib(), env._stream(), eng._params(10)
    ref, bf16 = ctypes.byref(q), int(dtype == torch.bfloat16)
    x = torch.randn((n, 48), device=dev).to(dtype)
    w, b, sg_w, sb = dn.layers[0]
    xs, mu32, sg32 = torch.empty_like(x), torch.randn((n, 64), device=dev), torch.randn((n, 64), device=dev)
    h = torch.randn((n, 64), device=dev).to(dtype)
    hs = torch.empty((n, 128), dtype=dtype, device=dev)
    hmu, hsg = torch.randn((n, 112), device=dev), torch.randn((n, 112), device=dev)

    def scale(layer, src, dst, col):
        nat.check(L.sn_noisy_scale(env._h, ref, noisy_tag(layer, 0), nat.ptr(src), src.stride(0), src.shape[1], bf16,
                                   ctypes.c_void_p(dst.data_ptr() + col * dst.element_size()), dst.stride(0), st),
                  "sn_noisy_scale")

    def combine(layer, mu, sg, col0, width, sigma_b, relu):
        nat.check(L.sn_noisy_combine(env._h, ref, noisy_tag(layer, 1), nat.ptr(mu), nat.ptr(sg), mu.stride(0), col0, width,
                                     nat.ptr(sigma_b), relu, nat.ptr(mu), st), "sn_noisy_combine")

    legs = {"latent scale": lambda: scale(0, x, xs, 0),
            "latent GEMM (+ .float())": lambda: torch.addmm(b, x, w.t()).float(),
            "latent sigma GEMM (+ .float())": lambda: torch.mm(xs, sg_w.t()).float(),
            "latent combine (+ cast back)": lambda: (combine(0, mu32, sg32, 0, 64, sb, 1), mu32.to(dtype)),
            "heads scale (V and A)": lambda: (scale(1, h, hs, 0), scale(2, h, hs, 64)),
            "heads GEMM (+ .float())": lambda: torch.addmm(dn.head_b, h, dn.head_w).float(),
            "heads sigma GEMM (+ .float())": lambda: torch.mm(hs, dn.head_s).float(),
            "heads combine (V and A)": lambda: (combine(1, hmu, hsg, 104, 1, dn.head_sb, 0),
                                                combine(2, hmu, hsg, 0, 104, dn.head_sb, 0)),
            "plain latent GEMM (bias + ReLU fused)": lambda: torch._addmm_activation(b, x, w.t())}
    times = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            t = timed(fn)
            if r >= warmup:
                times[k].append(t)
    return {"deciders": n, "net_dtype": str(dtype),
            "us": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-league", action="store_true")
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--noisy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dqn_prof: no GPU -- times are taken on the device or not at all")
    if args.noisy:
        result = {"league": noisy_rounds(args.slots, args.reps, args.warmup)}
        result["steps"] = noisy_steps(result["league"]["noisy"]["deciders_last_round"] // SEATS * SEATS or SEATS,
                                      max(args.reps, 20), args.warmup)
        text = json.dumps(result, indent=1)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    legs, keep = kernel_legs()
    result = {"deciders": D, "episode_rows": T * D, "minibatch": MINIBATCH, "capacity": CAPACITY, "reps": args.reps,
              "bytes": BYTES}
    for op, (native, yard) in legs.items():
        t_n, t_y = [], []
        for r in range(args.warmup + args.reps):
            a, b = timed(native), timed(yard)
            if r >= args.warmup:
                t_n.append(a)
                t_y.append(b)
        res = {"native_us": statistics.median(t_n), "native_min_us": min(t_n), "native_max_us": max(t_n),
               "torch_us": statistics.median(t_y), "torch_min_us": min(t_y), "torch_max_us": max(t_y)}
        res["native_GBps"] = BYTES[op] / res["native_us"] / 1e3
        res["torch_over_native"] = res["torch_us"] / res["native_us"]
        result[op] = res
    del legs, keep
    if not args.no_league:
        result["league"] = league_round(args.slots, args.rounds)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
