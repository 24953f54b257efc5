#!/usr/bin/env python3
"""Golden-vector generator for the 6 nimmt! hot path.

Runs ONLY in the build container (never on the GPU box): it imports the
reference implementation from /root/reference (read-only) and records its
outputs as small JSON / NPZ fixtures under tests/golden/.  The fixtures are
data (inputs + expected outputs); no reference source is copied.

The reference imports three third-party modules that are absent from this
image (gym, numba, multi_elo).  None of them takes part in the arithmetic
being pinned (env.py only subclasses gym.Env and builds Discrete/Box space
descriptors, numba only decorates the PER buffer's helpers (F15 / F16 below), multi_elo is
only called by Tournament._compute_elos, which is not exercised here), so the
generator puts attribute-holder stand-ins for them on sys.path in a
temporary directory before importing the reference.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_fixtures.py [--out tests/golden]

Fixture families (SURVEY.md §4 "What the build must add"):
  F0 mt19937.json        numpy legacy MT19937 seeding / shuffle / choice vectors
  F1 notebook_games.json five rendered games from experiments/simple_tournament.ipynb
  F2 random_games.npz    seeded GameSession(DrunkHamster x N) games, N = 1..10
     random_sessions.json multi-episode sessions (auto-reset stream continuation)
  F3 edge_cases.json     crafted + random reset_to positions, one step each
  F4 mcs_games.json      seeded GameSession(MCSAgent, DrunkHamster...) games
  F5 puct_math.json      PUCTAgent._compute_pucts / _normalize_q vectors
  F6 normalization.json  SechsNimmtStateNormalization vectors
  F7 positions.json      Tournament._compute_relative/absolute_positions vectors
  F8 puct_policy.npz     PUCTAgent policy-net weights + _compute_policy outputs
  F9 customed_games.json seeded GameSession(PUCTCustomedAgent, DrunkHamster...)
     customed_weights.npz  training games: actions, log-probs, value outcomes,
                           losses, and the 2-head net before / after each game
  F10 reinforce_games.json seeded GameSession(BatchedReinforceAgent, ...)
      reinforce_weights.npz  training games: actions, log-probs, entropies,
                           losses, final weights
  F12 acer_games.json    seeded GameSession(BatchedACERAgent, ...) training
      acer_weights.npz     sessions (torch + numpy + Python `random` seeded):
                           per ACER seat and step the observation, legal
                           cards, move, log-prob, value, reward and done; the
                           (actor, correction, critic) losses of every update;
                           initial and final weights
  F11 tournament_games.json seeded Tournament.play_game() sequences: seat
                           draws (agent names in seat order), results,
                           relative positions, wins, per-agent tallies --
                           (a) DrunkHamster + MCSAgent leagues (the drop-in
                           Tournament), (b) DrunkHamster-only leagues, one
                           seeded stream per slot (the batched league).
                           Tournament._compute_elos is replaced by a no-op
                           (multi_elo is absent: Elo stays unpinned).
  F13 evolve_games.json  seeded Tournament games with evolve() between blocks
                           (every metric, copies / max_players /
                           max_per_descendant combinations, two or three
                           evolves): games and the roster after each evolve
  F15 per_traces.json    seeded PriorityReplayBuffer traces (store / sample /
                           batch_update rounds): per round the uniforms, the
                           errors, the sampled tree indices, priorities and
                           weights, beta and len; tree snapshots (the float
      per_traces.npz       arrays in the .npz)
  F16 dqn_games.json     seeded GameSession(<DQN agent>, DrunkHamster x 3)
      dqn_weights.npz      training sessions of DQNVanilla, DDQNAgent,
                           DQN_PRBAgent and DDQN_PRBAgent (default epsilon
                           schedule, and a constant epsilon of 0.3): per step
                           the move, info["value"] and epsilon; the loss of
                           every learn(); the PER tree indices sampled;
                           initial and final weights
  F17 dqn_variant_games.json  the F16 recipe for DuellingDQNAgent,
      dqn_variant_weights.npz   DuellingDDQNAgent, DuellingDDQN_PRBAgent and
                           D3QN_PRB_NStep(n_steps=3); for the n-step sessions
                           also, for the first two games, every learn call's
                           (state, reward, action, next_state, done) and the
                           transitions the replay stored, in store order, with
                           the reward as float64; the prioritised
                           sessions also reject seeds whose importance
                           weights hinge on a near-zero TD error
                           (DQNVAR_MIN_LEAF)
  F18 dqn_noisy_games.json  the same recipe for Noisy_DQN, Noisy_D3QN and
      dqn_noisy_weights.npz   Noisy_D3QN_PRB_NStep(n_steps=3), one session
                           each: per step the move and info["value"] (no
                           epsilon), the losses, the PER indices, the weights
                           without the epsilon buffers; the gap of a decision
                           is taken over scores[legal].  torch's CPU generator
                           drives the weights and every noise draw

F15 / F16 pin the reference's *Python* semantics of the prioritised replay:
with the stand-in numba.jit the sampler `_get_leaf_ids` runs as plain Python
and draws from Python's global `random`.  Under real numba the jitted sampler
draws from numba's own generator, which `random.seed` does not reach, so the
reference is not reproducible there at all.
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

REF = "/root/reference"

_STUBS = {
    "gym/__init__.py": "class Env:\n    def __init__(self):\n        pass\nfrom . import spaces\n",
    "gym/spaces.py": (
        "class Discrete:\n    def __init__(self, n):\n        self.n = n\n"
        "class Box:\n    def __init__(self, low, high, shape, dtype=None):\n"
        "        self.low, self.high, self.shape, self.dtype = low, high, shape, dtype\n"
    ),
    "numba/__init__.py": (
        "def jit(*a, **k):\n    if a and callable(a[0]):\n        return a[0]\n    return lambda f: f\n"
    ),
    "multi_elo/__init__.py": (
        "class EloPlayer:\n    def __init__(self, place, elo):\n        self.place, self.elo = place, elo\n"
        "def calc_elo(players, k):\n    raise NotImplementedError('multi_elo is not installed')\n"
    ),
}


def import_reference():
    d = tempfile.mkdtemp(prefix="sechs_stubs_")
    for rel, text in _STUBS.items():
        p = os.path.join(d, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as f:
            f.write(text)
    sys.path.insert(0, d)
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import logging

    logging.disable(logging.CRITICAL)
    import rl_6_nimmt  # noqa: F401

    return rl_6_nimmt


# ----------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------
def board_of(env):
    return [[int(c) for c in row] for row in env._board]


def hands_of(env):
    return [[int(c) for c in h] for h in env._hands]


def obs_of(states):
    return [[int(v) for v in s] for s in states]


# ----------------------------------------------------------------------------
# F0: numpy legacy MT19937
# ----------------------------------------------------------------------------
def gen_mt(out):
    seeds = [0, 1, 2, 5, 42, 1234, 65535, 2**31 - 1, 2**32 - 1]
    rec = {"seeds": [], "shuffles": [], "choices": []}
    for s in seeds:
        np.random.seed(s)
        st = np.random.get_state()
        key = [int(x) for x in st[1]]
        rec["seeds"].append({"seed": s, "key_head": key[:8], "key_tail": key[-8:], "pos": int(st[2])})
        np.random.seed(s)
        raw = [int(x) for x in np.random.randint(0, 2**32, size=700, dtype=np.uint64)]
        rec["seeds"][-1]["raw_u32"] = raw  # legacy full-range draws == raw genrand_int32 outputs? verified below
    for s in list(range(40)) + [65535, 99991]:
        np.random.seed(s)
        deck = np.arange(104, dtype=np.int32)
        np.random.shuffle(deck)
        deck2 = np.arange(57, dtype=np.int32)
        np.random.shuffle(deck2)
        rec["shuffles"].append({"seed": s, "deck104_then_deck57": [int(x) for x in deck] + [int(x) for x in deck2]})
    for s in range(20):
        np.random.seed(s)
        seq = []
        for n in [10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 17, 33, 64, 65, 100]:
            arr = np.arange(n, dtype=np.int32) * 3 + 1
            seq.append([n, int(np.random.choice(arr, size=1)[0])])
        rec["choices"].append({"seed": s, "n_and_pick": seq})
    with open(os.path.join(out, "mt19937.json"), "w") as f:
        json.dump(rec, f)


# ----------------------------------------------------------------------------
# F1: notebook traces
# ----------------------------------------------------------------------------
_CARD = re.compile(r"\s*(\d+)([ .:+#])")


def _parse_cards(text):
    cards = []
    for tok in re.findall(r"(\d+)[ .:+#]?", text):
        cards.append(int(tok) - 1)
    return cards


def parse_notebook_games(ref):
    from rl_6_nimmt.env import SechsNimmtEnv

    nb = json.load(open(os.path.join(REF, "experiments/simple_tournament.ipynb")))
    games = []
    for cell in nb["cells"]:
        if cell.get("cell_type") != "code":
            continue
        text = "".join(
            "".join(o.get("text", "")) for o in cell.get("outputs", []) if o.get("output_type") == "stream"
        )
        if "Dealing cards" not in text:
            continue
        for chunk in text.split("Dealing cards")[1:]:
            lines = chunk.split("\n")
            board, hands, names = [], [], []
            i = 0
            while "Board:" not in lines[i]:
                i += 1
            i += 1
            while "Players:" not in lines[i]:
                row = lines[i].split("_")[0].split("*")[0]
                board.append(_parse_cards(row))
                i += 1
            i += 1
            while lines[i].startswith("  ") and "(player" in lines[i]:
                name = lines[i].split("(player")[0].strip()
                names.append(name)
                hand_txt = lines[i].split("cards", 1)[1]
                hands.append(_parse_cards(hand_txt))
                i += 1
            plays = []
            for ln in lines[i:]:
                m = re.search(r"\(player (\d+)\) plays card (\d+)", ln)
                if m:
                    plays.append((int(m.group(1)) - 1, int(m.group(2)) - 1))
                if "The game is over" in ln:
                    break
            final = None
            # final scores from the last rendered "Players:" block
            score_re = re.compile(r"\(player (\d+)\):\s+(-?\d+) Hornochsen")
            last = {}
            for ln in lines:
                m = score_re.search(ln)
                if m:
                    last[int(m.group(1)) - 1] = int(m.group(2))
                if "The game is over" in ln:
                    break
            final = [last[p] for p in range(len(names))]
            n = len(names)
            # plays are logged in ascending card order per step; regroup by step
            steps = []
            for k in range(0, len(plays), n):
                acts = [None] * n
                for p, c in plays[k : k + n]:
                    acts[p] = c
                steps.append(acts)
            games.append({"names": names, "board": board, "hands": hands, "actions": steps, "final_penalties": final})
    # replay through the reference env to record per-step expected outputs
    for g in games:
        env = SechsNimmtEnv(len(g["names"]), verbose=False)
        states, legal = env.reset_to([list(r) for r in g["board"]], [list(h) for h in g["hands"]])
        g["obs0"] = obs_of(states)
        recs = []
        scores = np.zeros(len(g["names"]), dtype=np.int64)
        for acts in g["actions"]:
            (states, legal), rew, done, _ = env.step(list(acts))
            scores += rew
            recs.append({"rewards": [int(r) for r in rew], "done": bool(done), "board": board_of(env), "obs": obs_of(states)})
        g["steps"] = recs
        g["final_scores"] = [int(x) for x in scores]
        assert [int(x) for x in env._scores] == g["final_penalties"], (env._scores, g["final_penalties"])
    return games


def gen_notebook(ref, out):
    games = parse_notebook_games(ref)
    assert len(games) == 5, len(games)
    with open(os.path.join(out, "notebook_games.json"), "w") as f:
        json.dump({"source": "experiments/simple_tournament.ipynb rendered DEBUG logs", "games": games}, f)


# ----------------------------------------------------------------------------
# F2: seeded random games
# ----------------------------------------------------------------------------
def play_recorded(env, agents):
    """Mirror of GameSession.play_game's RNG-consuming call order (play.py:23-75)."""
    states, legal = env.reset()
    deal = (board_of(env), hands_of(env))
    obs = [obs_of(states)]
    acts, rews, dones = [], [], []
    done = False
    while not done:
        a = []
        for agent, s, l in zip(agents, states, legal):
            action, _ = agent(s, legal_actions=l)
            a.append(int(action))
        (states, legal), r, done, _ = env.step(a)
        acts.append(a)
        rews.append([int(x) for x in r])
        dones.append(bool(done))
        obs.append(obs_of(states))
    return deal, acts, rews, dones, obs


def gen_random_games(ref, out):
    from rl_6_nimmt.env import SechsNimmtEnv
    from rl_6_nimmt.play import GameSession
    from rl_6_nimmt.agents import DrunkHamster

    arrays = {}
    meta = []
    configs = []
    for n in range(1, 11):
        configs.append((n, 104, True, 60 if n == 4 else 12))
    configs += [(2, 24, True, 8), (3, 40, True, 8), (4, 80, True, 6), (4, 104, False, 8), (2, 104, False, 4)]
    for ci, (n, c, summ, nseeds) in enumerate(configs):
        L = 10 + 1 + (12 if summ else 0) + 24
        decks_board, hands_all, acts_all, rews_all, obs_all, res_all = [], [], [], [], [], []
        for s in range(nseeds):
            np.random.seed(s)
            env = SechsNimmtEnv(n, num_cards=c, include_summaries=summ, verbose=False)
            agents = [DrunkHamster() for _ in range(n)]
            deal, acts, rews, dones, obs = play_recorded(env, agents)
            assert dones == [False] * 9 + [True]
            res = np.sum(np.array(rews), axis=0)
            if summ and c == 104:
                # cross-check against the real GameSession harness (play.py)
                np.random.seed(s)
                sess = GameSession(*[DrunkHamster() for _ in range(n)])
                sess.play_game()
                assert [int(x) for x in sess.results[0]] == [int(x) for x in res]
            decks_board.append([r[0] for r in deal[0]])
            hands_all.append(deal[1])
            acts_all.append(acts)
            rews_all.append(rews)
            obs_all.append(obs)
            res_all.append([int(x) for x in res])
        key = f"c{ci}"
        arrays[key + "_board0"] = np.array(decks_board, dtype=np.int16)  # [S,4]
        arrays[key + "_hands0"] = np.array(hands_all, dtype=np.int16)  # [S,N,10]
        arrays[key + "_actions"] = np.array(acts_all, dtype=np.int16)  # [S,10,N]
        arrays[key + "_rewards"] = np.array(rews_all, dtype=np.int16)  # [S,10,N]
        arrays[key + "_obs"] = np.array(obs_all, dtype=np.int8)  # [S,11,N,L]
        arrays[key + "_results"] = np.array(res_all, dtype=np.int16)  # [S,N]
        meta.append({"key": key, "num_players": n, "num_cards": c, "include_summaries": summ, "seeds": nseeds, "obs_len": L})
    np.savez_compressed(os.path.join(out, "random_games.npz"), **arrays)
    with open(os.path.join(out, "random_games_meta.json"), "w") as f:
        json.dump(
            {
                "protocol": "np.random.seed(s); env=SechsNimmtEnv(N, num_cards=C, include_summaries=S); "
                "GameSession(DrunkHamster()*N).play_game() call order; obs[0] = reset obs, obs[t+1] = obs after step t",
                "configs": meta,
            },
            f,
        )

    # multi-episode sessions: the deal of game e+1 continues the RNG stream after game e
    sessions = []
    for n, seeds, eps in [(4, list(range(12)) + [65535], 8), (2, list(range(4)), 5), (3, [7, 8], 5), (10, [3], 4)]:
        for s in seeds:
            np.random.seed(s)
            sess = GameSession(*[DrunkHamster() for _ in range(n)])
            for _ in range(eps):
                sess.play_game()
            sessions.append({"num_players": n, "seed": s, "results": [[int(x) for x in r] for r in sess.results]})
    # long sessions for a few bench lanes (bench: game g seeded g, 100 episodes back to back)
    for s in [0, 1, 2, 4097, 65535]:
        np.random.seed(s)
        sess = GameSession(*[DrunkHamster() for _ in range(4)])
        for _ in range(100):
            sess.play_game()
        tot = np.sum(np.array(sess.results), axis=0)
        sessions.append(
            {
                "num_players": 4,
                "seed": s,
                "episodes": 100,
                "results_last": [int(x) for x in sess.results[-1]],
                "results_sum": [int(x) for x in tot],
            }
        )
    with open(os.path.join(out, "random_sessions.json"), "w") as f:
        json.dump({"protocol": "np.random.seed(s); sess=GameSession(DrunkHamster()*N); sess.play_game() x episodes", "sessions": sessions}, f)


# ----------------------------------------------------------------------------
# F3: edge cases through reset_to
# ----------------------------------------------------------------------------
def _one_step_case(SechsNimmtEnv, InvalidMoveException, board, hands, actions, label, summ=True):
    n = len(hands)
    env = SechsNimmtEnv(n, include_summaries=summ, verbose=False)
    states0, legal0 = env.reset_to([list(r) for r in board], [list(h) for h in hands])
    case = {"label": label, "board": board, "hands": hands, "actions": actions, "include_summaries": summ, "obs0": obs_of(states0)}
    try:
        (states, legal), rew, done, _ = env.step(list(actions))
        case["expect"] = {
            "rewards": [int(x) for x in rew],
            "done": bool(done),
            "board": board_of(env),
            "hands": hands_of(env),
            "scores": [int(x) for x in env._scores],
            "obs": obs_of(states),
            "legal": [[int(c) for c in l] for l in legal],
        }
    except InvalidMoveException as e:
        case["error"] = {"type": "InvalidMoveException", "message": str(e)}
    except AssertionError:
        case["error"] = {"type": "AssertionError", "message": ""}
    return case


def gen_edge_cases(ref, out):
    from rl_6_nimmt.env import SechsNimmtEnv, InvalidMoveException

    cases = []
    add = lambda *a, **k: cases.append(_one_step_case(SechsNimmtEnv, InvalidMoveException, *a, **k))
    # crafted
    add([[10], [20], [30], [40]], [[5], [6]], [5, 6], "double undercut, equal row values -> lowest row index first")
    add([[10, 11], [20], [30, 31], [40]], [[5, 50], [6, 51]], [5, 6], "undercut picks min heads row (row 1)")
    add([[10, 11, 12, 13, 14], [20], [30], [40]], [[15, 0], [16, 1]], [15, 16], "6th card take then append to new row")
    add([[10, 11, 12, 13, 14], [20, 21, 22, 23, 24], [30], [40]], [[15, 0], [25, 1], [26, 2]], [15, 25, 26], "two takes in one step")
    add([[50, 51, 52, 53], [60], [70], [80]], [[54, 1], [55, 2]], [54, 55], "card 55 (idx 54, 7 heads) completes row then 6th takes it")
    add([[50, 51, 52, 53], [60], [70], [80]], [[54, 1], [56, 2], [57, 3]], [54, 56, 57], "6th card on a row a lower card extended this step")
    add([[54], [10], [21], [98]], [[0], [1], [2], [3]], [0, 1, 2, 3], "four undercuts in one step")
    add([[54, 64, 74, 84, 94], [10, 20, 30, 40, 43], [9], [8]], [[95, 0], [44, 1], [3, 2], [2, 5]], [95, 44, 3, 2], "big penalties")
    add([[10], [20], [30], [40]], [[5, 6], [7, 8]], [6, 9], "invalid move by player 2")
    add([[10], [20], [30], [40]], [[5, 6], [7, 8]], [99, 7], "invalid move by player 1")
    add([[10], [20], [30], [40]], [[5, 6], [7, 8]], [5], "wrong number of actions")
    add([[10], [20], [30], [40]], [[5], [7]], [5, 7], "last card -> done", summ=False)
    # N = 10 with the whole deck in play
    rng = np.random.RandomState(1234)
    deck = list(rng.permutation(104))
    hands = [sorted(int(c) for c in deck[10 * p : 10 * p + 10]) for p in range(10)]
    board = [[int(deck[103 - r])] for r in range(4)]
    add(board, hands, [h[rng.randint(len(h))] for h in hands], "N=10 full deck first step")
    # random positions: rows of 1..5 cards, hands of n cards
    rng = np.random.RandomState(20251015)
    for k in range(320):
        n_players = int(rng.choice([2, 3, 4, 4, 4, 5, 6, 8, 10]))
        n = int(rng.randint(1, 11))
        lens = [int(rng.randint(1, 6)) for _ in range(4)]
        need = sum(lens) + n_players * n
        if need > 104:
            continue
        perm = [int(c) for c in rng.permutation(104)[:need]]
        board = []
        pos = 0
        for L in lens:
            board.append(sorted(perm[pos : pos + L]) if rng.rand() < 0.8 else perm[pos : pos + L])
            pos += L
        hands = []
        for p in range(n_players):
            hands.append(sorted(perm[pos : pos + n]))
            pos += n
        actions = [h[int(rng.randint(len(h)))] for h in hands]
        if rng.rand() < 0.03:
            actions[int(rng.randint(n_players))] = int(rng.randint(0, 104))
        add(board, hands, actions, f"random #{k}", summ=bool(rng.rand() < 0.9))
    with open(os.path.join(out, "edge_cases.json"), "w") as f:
        json.dump({"protocol": "env=SechsNimmtEnv(N, include_summaries=S); env.reset_to(board, hands); env.step(actions)", "cases": cases}, f)


# ----------------------------------------------------------------------------
# F4: seeded MCS games
# ----------------------------------------------------------------------------
def gen_mcs(ref, out):
    from rl_6_nimmt.env import SechsNimmtEnv
    from rl_6_nimmt.agents import DrunkHamster, MCSAgent
    from rl_6_nimmt.play import GameSession

    games = []
    specs = []
    specs += [("MRRR", 4, 100, 10, s) for s in range(6)]
    specs += [("MR", 2, 100, 10, s) for s in range(3)]
    specs += [("MMRR", 4, 40, 4, s) for s in range(3)]
    specs += [("RMR", 3, 30, 10, s) for s in range(3)]
    specs += [("MRRR", 4, 200, 10, s) for s in range(2)]
    t0 = time.time()
    for seats, n, mc_max, mc_per_card, s in specs:
        agents = [MCSAgent(mc_max=mc_max, mc_per_card=mc_per_card) if ch == "M" else DrunkHamster() for ch in seats]
        np.random.seed(s)
        env = SechsNimmtEnv(n, verbose=False)
        try:
            deal, acts, rews, dones, obs = play_recorded_tensor(env, agents)
            rec = {"seats": seats, "mc_max": mc_max, "mc_per_card": mc_per_card, "seed": s, "board0": deal[0], "hands0": deal[1], "actions": acts, "rewards": rews}
        except IndexError:
            rec = {"seats": seats, "mc_max": mc_max, "mc_per_card": mc_per_card, "seed": s, "error": "IndexError (mcts.py:170 debug f-string, quirk Q6)"}
        # cross-check with the real harness
        if "error" not in rec:
            agents = [MCSAgent(mc_max=mc_max, mc_per_card=mc_per_card) if ch == "M" else DrunkHamster() for ch in seats]
            np.random.seed(s)
            sess = GameSession(*agents)
            sess.play_game()
            assert [int(x) for x in sess.results[0]] == [int(x) for x in np.sum(np.array(rec["rewards"]), axis=0)]
            rec["results"] = [int(x) for x in sess.results[0]]
        games.append(rec)
        print(f"  mcs {seats} mc_max={mc_max} seed={s}: {time.time() - t0:.1f}s", flush=True)
    with open(os.path.join(out, "mcs_games.json"), "w") as f:
        json.dump({"protocol": "np.random.seed(s); GameSession(*agents).play_game(); M=MCSAgent(mc_max, mc_per_card), R=DrunkHamster", "games": games}, f)


def play_recorded_tensor(env, agents):
    """Same as play_recorded but hands agents float tensors like GameSession._tensorize (play.py:77-78)."""
    import torch

    states, legal = env.reset()
    deal = (board_of(env), hands_of(env))
    tens = lambda st: [torch.tensor(x).to(torch.device("cpu"), torch.float) for x in st]
    states = tens(states)
    acts, rews, dones = [], [], []
    done = False
    while not done:
        a = []
        for agent, s, l in zip(agents, states, legal):
            action, _ = agent(s, legal_actions=l)
            a.append(int(action))
        (states, legal), r, done, _ = env.step(a)
        states = tens(states)
        acts.append(a)
        rews.append([int(x) for x in r])
        dones.append(bool(done))
    return deal, acts, rews, dones, None


# ----------------------------------------------------------------------------
# F5/F6/F8: PUCT math, normalisation, policy
# ----------------------------------------------------------------------------
def gen_puct(ref, out):
    import torch
    from rl_6_nimmt.agents import PUCTAgent
    from rl_6_nimmt.utils.preprocessing import SechsNimmtStateNormalization

    torch.manual_seed(0)
    agent = PUCTAgent()
    rng = np.random.RandomState(7)
    cases = []
    for k in range(300):
        n = int(rng.randint(2, 11))
        legal = sorted(int(c) for c in rng.permutation(104)[:n])
        total = int(rng.choice([0, 3, 9, 10, 11, 40, 200]))
        outcomes = {a: [] for a in legal}
        mode = k % 5
        for _ in range(total):
            a = legal[int(rng.randint(n))]
            if mode == 0:
                outcomes[a].append(-7.0)  # max == min  -> NaN q (quirk Q7)
            else:
                outcomes[a].append(float(-rng.randint(0, 40)))
        p = rng.rand(n).astype(np.float32) + 1e-3
        p = p / p.sum()
        probs = torch.tensor(p)
        with np.errstate(all="ignore"):
            pucts = agent._compute_pucts(legal, outcomes, probs)
            nq = agent._normalize_q(outcomes)
        best, choice = -float("inf"), 0
        for i, v in enumerate(pucts):
            if v > best:
                best, choice = v, i
        cases.append(
            {
                "legal": legal,
                "outcomes": [outcomes[a] for a in legal],
                "probs": [float(x) for x in p],
                "pucts": [None if np.isnan(x) else float(x) for x in pucts],
                "normalize_q": [float(x) for x in nq],
                "choice": choice,
            }
        )
    with open(os.path.join(out, "puct_math.json"), "w") as f:
        json.dump({"c_puct": 2.0, "cases": cases}, f)

    # F6 normalisation
    norm = SechsNimmtStateNormalization(action=True)
    norm0 = SechsNimmtStateNormalization(action=False)
    x = np.concatenate(
        [rng.randint(-1, 104, size=(64, 1 + 10)), rng.randint(1, 11, size=(64, 1)), rng.randint(-1, 104, size=(64, 36))], axis=1
    ).astype(np.float32)
    y = norm(torch.tensor(x)).numpy()
    y0 = norm0(torch.tensor(x[:, 1:])).numpy()
    with open(os.path.join(out, "normalization.json"), "w") as f:
        json.dump({"x_with_action": x.tolist(), "y_with_action": y.tolist(), "y_without_action": y0.tolist()}, f)

    # F8 policy forward with fixed weights
    from rl_6_nimmt.env import SechsNimmtEnv

    arrays = {k: v.detach().numpy().astype(np.float32) for k, v in agent.actor.state_dict().items()}
    names = sorted(arrays)
    env = SechsNimmtEnv(4, verbose=False)
    np.random.seed(3)
    states, legal = env.reset()
    xs, ps = [], []
    for p in range(4):
        st = torch.tensor(states[p]).to(torch.float)
        with torch.no_grad():
            pr = agent._compute_policy(legal[p], st).numpy()
        xs.append(np.array(states[p], dtype=np.int16))
        ps.append(pr.astype(np.float32))
    arrays["states"] = np.stack(xs)
    arrays["legal"] = np.array(legal, dtype=np.int16)
    arrays["probs"] = np.stack(ps)
    np.savez_compressed(os.path.join(out, "puct_policy.npz"), **arrays)
    with open(os.path.join(out, "puct_policy_meta.json"), "w") as f:
        json.dump({"weights": names, "init": "torch.manual_seed(0); PUCTAgent()"}, f)


# ----------------------------------------------------------------------------
# F9: PUCTCustomedAgent (policy + value head, no rollouts) in training sessions
# ----------------------------------------------------------------------------
def gen_customed(ref, out):
    import torch
    from rl_6_nimmt.agents import DrunkHamster, PUCTCustomedAgent
    from rl_6_nimmt.play import GameSession

    specs = [("CRRR", s, 2) for s in range(4)] + [("CR", 7, 2), ("RCR", 11, 1), ("CC", 5, 2)]
    sessions, arrays = [], {}
    for si, (seats, seed, n_games) in enumerate(specs):
        torch.manual_seed(seed)
        agents = [PUCTCustomedAgent(mc_max=200) if ch == "C" else DrunkHamster() for ch in seats]
        for a, ch in zip(agents, seats):
            if ch == "C":
                a.train()
        trace = {i: {"info": [], "loss": []} for i, ch in enumerate(seats) if ch == "C"}
        for i in trace:
            ag = agents[i]
            for k, v in ag.actor.state_dict().items():
                arrays[f"s{si}_a{i}_init_{k}"] = v.detach().numpy().astype(np.float32)
            fwd, lrn = ag.forward, ag.learn

            def fwd_rec(state, legal_actions, *a, _fwd=fwd, _i=i, **k):
                act, info = _fwd(state, legal_actions, *a, **k)
                trace[_i]["info"].append([int(act), float(info["log_prob"]), float(info["outcome"])])
                return act, info

            def lrn_rec(*a, _lrn=lrn, _i=i, **k):
                loss = _lrn(*a, **k)
                if k.get("episode_end"):
                    trace[_i]["loss"].append(float(loss))
                return loss

            ag.forward, ag.learn = fwd_rec, lrn_rec
        np.random.seed(seed)
        sess = GameSession(*agents)
        for _ in range(n_games):
            sess.play_game()
        for i in trace:
            for k, v in agents[i].actor.state_dict().items():
                arrays[f"s{si}_a{i}_final_{k}"] = v.detach().numpy().astype(np.float32)
        sessions.append({"seats": seats, "seed": seed, "games": n_games,
                         "results": [[int(x) for x in r] for r in sess.results],
                         "trace": {str(i): t for i, t in trace.items()}})
    np.savez_compressed(os.path.join(out, "customed_weights.npz"), **arrays)
    with open(os.path.join(out, "customed_games.json"), "w") as f:
        json.dump({"protocol": "torch.manual_seed(seed); agents (C = PUCTCustomedAgent(mc_max=200) in train mode, "
                               "R = DrunkHamster); np.random.seed(seed); GameSession(*agents).play_game() x games. "
                               "trace[seat].info = per forward [action, log_prob, outcome]; loss = learn() at episode end",
                   "sessions": sessions}, f)


# ----------------------------------------------------------------------------
# F10: BatchedReinforceAgent (REINFORCE) in training sessions
# ----------------------------------------------------------------------------
def gen_reinforce(ref, out):
    import torch
    from rl_6_nimmt.agents import BatchedReinforceAgent, DrunkHamster
    from rl_6_nimmt.play import GameSession

    specs = [("PRRR", 0, 3, {}), ("PR", 4, 2, {"r_factor": 0.1, "entropy_weight": 0.05}),
             ("PP", 9, 2, {"gamma": 0.9}), ("RPRRP", 2, 1, {})]
    sessions, arrays = [], {}
    for si, (seats, seed, n_games, kw) in enumerate(specs):
        torch.manual_seed(seed)
        agents = [BatchedReinforceAgent(**kw) if ch == "P" else DrunkHamster() for ch in seats]
        trace = {}
        for i, ch in enumerate(seats):
            if ch != "P":
                continue
            ag = agents[i]
            ag.train()
            if si == 0:
                for k, v in ag.actor.state_dict().items():
                    arrays[f"s{si}_a{i}_init_{k}"] = v.detach().numpy().astype(np.float32)
            trace[i] = {"info": [], "loss": []}
            fwd, lrn = ag.forward, ag.learn

            def fwd_rec(state, legal_actions, *a, _fwd=fwd, _i=i, **k):
                act, info = _fwd(state, legal_actions, *a, **k)
                trace[_i]["info"].append([int(act), float(info["log_prob"]), float(info["entropy"])])
                return act, info

            def lrn_rec(*a, _lrn=lrn, _i=i, **k):
                losses = _lrn(*a, **k)
                if k.get("episode_end"):
                    trace[_i]["loss"].append([float(x) for x in losses])
                return losses

            ag.forward, ag.learn = fwd_rec, lrn_rec
        np.random.seed(seed)
        sess = GameSession(*agents)
        for _ in range(n_games):
            sess.play_game()
        for i in trace:
            for k, v in agents[i].actor.state_dict().items():
                arrays[f"s{si}_a{i}_final_{k}"] = v.detach().numpy().astype(np.float32)
        sessions.append({"seats": seats, "seed": seed, "games": n_games, "kwargs": kw,
                         "results": [[int(x) for x in r] for r in sess.results],
                         "trace": {str(i): t for i, t in trace.items()}})
    np.savez_compressed(os.path.join(out, "reinforce_weights.npz"), **arrays)
    with open(os.path.join(out, "reinforce_games.json"), "w") as f:
        json.dump({"protocol": "torch.manual_seed(seed); agents (P = BatchedReinforceAgent(**kwargs) in train mode, "
                               "R = DrunkHamster); np.random.seed(seed); GameSession(*agents).play_game() x games. "
                               "trace[seat].info = per forward [action, log_prob, entropy]; loss = learn() at "
                               "episode end ([actor, 0, entropy])",
                   "sessions": sessions}, f)


# ----------------------------------------------------------------------------
# F12: BatchedACERAgent (ACER) in training sessions
# ----------------------------------------------------------------------------
ACER_SPECS = [("ARRR", 0, 5, {"warmup": 2, "minibatch": 2}),
              ("AR", 3, 4, {"rollout_len": 4, "warmup": 3, "minibatch": 2, "r_factor": 0.5}),
              ("AA", 6, 3, {"warmup": 1, "minibatch": 1, "truncate": 0.5, "critic_weight": 0.5}),
              ("ARR", 8, 6, {"history_length": 3, "warmup": 1, "minibatch": 2, "rollout_len": 3, "gamma": 0.9})]


def gen_acer(ref, out):
    import random

    import torch
    from rl_6_nimmt.agents import BatchedACERAgent, DrunkHamster
    from rl_6_nimmt.play import GameSession

    sessions, arrays = [], {}
    for si, (seats, seed, n_games, kw) in enumerate(ACER_SPECS):
        torch.manual_seed(seed)
        agents = [BatchedACERAgent(**kw) if ch == "A" else DrunkHamster() for ch in seats]
        trace = {}
        for i, ch in enumerate(seats):
            if ch != "A":
                continue
            ag = agents[i]
            ag.train()
            for k, v in ag.actor_critic.state_dict().items():
                arrays[f"s{si}_a{i}_init_{k}"] = v.detach().numpy().astype(np.float32)
            trace[i] = {"steps": [], "losses": []}
            fwd, lrn, trn = ag.forward, ag.learn, ag._train

            def fwd_rec(state, legal_actions, *a, _fwd=fwd, _i=i, **k):
                act, info = _fwd(state, legal_actions, *a, **k)
                trace[_i]["steps"].append({"obs": [int(x) for x in state.tolist()], "legal": [int(x) for x in legal_actions],
                                           "action": int(act), "log_prob": float(info["log_prob"]),
                                           "value": float(info["value"])})
                return act, info

            def lrn_rec(*a, _lrn=lrn, _i=i, **k):
                st = trace[_i]["steps"][-1]
                st["next_reward"], st["done"] = int(k["next_reward"]), bool(k["done"])
                return _lrn(*a, **k)

            def trn_rec(on_policy=True, _trn=trn, _i=i):
                losses = _trn(on_policy)
                trace[_i]["losses"].append([len(trace[_i]["steps"]), bool(on_policy)] + [float(x) for x in losses])
                return losses

            ag.forward, ag.learn, ag._train = fwd_rec, lrn_rec, trn_rec
        np.random.seed(seed)
        random.seed(seed)
        sess = GameSession(*agents)
        for _ in range(n_games):
            sess.play_game()
        for i in trace:
            for k, v in agents[i].actor_critic.state_dict().items():
                arrays[f"s{si}_a{i}_final_{k}"] = v.detach().numpy().astype(np.float32)
        sessions.append({"seats": seats, "seed": seed, "games": n_games, "kwargs": kw,
                         "results": [[int(x) for x in r] for r in sess.results],
                         "trace": {str(i): t for i, t in trace.items()}})
    np.savez_compressed(os.path.join(out, "acer_weights.npz"), **arrays)
    with open(os.path.join(out, "acer_games.json"), "w") as f:
        json.dump({"protocol": "torch.manual_seed(seed); agents (A = BatchedACERAgent(**kwargs) in train mode, "
                               "R = DrunkHamster); np.random.seed(seed); random.seed(seed); "
                               "GameSession(*agents).play_game() x games. trace[seat].steps = per forward the obs, legal "
                               "cards, action, log_prob, value, and the next_reward/done learn() received; losses = "
                               "per _train call [steps so far, on_policy, actor, correction, critic]",
                   "sessions": sessions}, f)


# ----------------------------------------------------------------------------
# F7: tournament positions
# ----------------------------------------------------------------------------
def gen_positions(ref, out):
    from rl_6_nimmt.tournament import Tournament

    rng = np.random.RandomState(11)
    cases = []
    for k in range(200):
        n = int(rng.randint(2, 7))
        scores = -rng.randint(0, 8 if k % 3 == 0 else 40, size=n)
        scores = scores.astype(np.int32)
        rel = Tournament._compute_relative_positions(scores)
        ab = Tournament._compute_absolute_positions(scores)
        cases.append({"scores": [int(s) for s in scores], "relative": [float(v) for v in rel], "absolute": [float(v) for v in ab], "winner_index": int(np.argmax(scores))})
    with open(os.path.join(out, "positions.json"), "w") as f:
        json.dump({"cases": cases}, f)


def _tournament(ref, specs, min_players, max_players):
    from rl_6_nimmt.tournament import Tournament

    t = Tournament(min_players=min_players, max_players=max_players)
    for name, agent in specs:
        t.add_player(name, agent)
    # multi_elo is absent from this image: Elo is not pinned, the rest is
    t._compute_elos = lambda names, scores: [t.elos[n][-1] for n in names]
    return t


def _play_recorded_games(t, games):
    recs = []
    for _ in range(games):
        names, agents = t._choose_players(None)
        from rl_6_nimmt.play import GameSession

        sess = GameSession(*agents)
        sess.play_game(render=False)
        scores = sess.results[0]
        t.score_game(names, scores)
        recs.append({"names": list(names), "results": [int(x) for x in scores],
                     "relative": [float(v) for v in t._compute_relative_positions(scores)],
                     "winner": names[int(np.argmax(scores))]})
    return recs


def _tallies(t):
    return {n: {"played_games": int(t.played_games[n]), "scores": [int(x) for x in t.tournament_scores[n]],
                "positions": [float(x) for x in t.tournament_positions[n]],
                "wins": [float(x) for x in t.tournament_wins[n]]} for n in t.agents}


def gen_tournament(ref, out):
    """F11.  Each record replays `np.random.seed(seed)` + Tournament(...) +
    `play_game()` x games in the reference, where play_game() is
    _choose_players (num_players = choice(range(min, max+1)), then
    choice(len(active), num_players, replace=False)), GameSession(*agents)
    .play_game() and score_game() -- the same global numpy stream throughout
    (tournament.py:132-177)."""
    from rl_6_nimmt.agents import DrunkHamster, MCSAgent

    dropin = []
    mc_max, mc_per_card = 100, 10  # fewer playouts leave moves unsampled -> the reference's IndexError (Q6)
    for seed0, kinds, games in ((0, "RRMR", 5), (10, "RMRRR", 5), (20, "MRR", 4)):
        hi = min(4, len(kinds))
        for seed in range(seed0, seed0 + 10):  # the first seed whose league avoids quirk Q6
            np.random.seed(seed)
            specs = [(f"{k}{i}", MCSAgent(mc_max=mc_max, mc_per_card=mc_per_card) if k == "M" else DrunkHamster())
                     for i, k in enumerate(kinds)]
            t = _tournament(ref, specs, 2, hi)
            try:
                recs = _play_recorded_games(t, games)
            except IndexError:
                continue
            break
        dropin.append({"seed": seed, "agents": [n for n, _ in specs], "kinds": kinds, "min_players": 2,
                       "max_players": hi, "mc_max": mc_max, "mc_per_card": mc_per_card, "games": recs,
                       "tallies": _tallies(t), "total_games": int(t.total_games)})
        print(f"  tournament (drop-in) seed={seed} {kinds}: {len(recs)} games", flush=True)
    league = []
    for K, lo, hi, base, slots, games in ((5, 2, 4, 1000, 48, 4), (6, 4, 4, 2000, 16, 3), (3, 2, 3, 3000, 16, 3)):
        for j in range(slots):
            np.random.seed(base + j)
            specs = [(f"a{i}", DrunkHamster()) for i in range(K)]
            t = _tournament(ref, specs, lo, hi)
            recs = _play_recorded_games(t, games)
            league.append({"seed": base + j, "num_agents": K, "min_players": lo, "max_players": hi,
                           "seats": [[int(n[1:]) for n in r["names"]] for r in recs],
                           "results": [r["results"] for r in recs]})
    with open(os.path.join(out, "tournament_games.json"), "w") as f:
        json.dump({"protocol": "np.random.seed(seed); t = Tournament(min_players, max_players); add_player(name, agent) "
                               "for each agent; t.play_game() x games; Tournament._compute_elos replaced by a no-op "
                               "(multi_elo absent); M = MCSAgent(mc_max, mc_per_card), R = DrunkHamster; league: K "
                               "DrunkHamster agents a0..a{K-1}, seats = agent indices in seat order",
                   "dropin": dropin, "league": league}, f)


def _restated_elo():
    """the build's multi_elo restatement (rl-6-nimmt_amd/rl_6_nimmt/elo.py),
    loaded by path: multi_elo is absent, so F13's Elo values are that
    restatement's (Elo arithmetic parity stays unpinned), while what F13 pins
    -- evolve's ranking, cloning and pruning over them -- is the reference's"""
    import importlib.util

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rl-6-nimmt_amd", "rl_6_nimmt", "elo.py")
    spec = importlib.util.spec_from_file_location("sechs_elo_restated", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _roster(t):
    """the reference tournament's roster in its dict order, with every tally"""
    return [{"name": n, "active": bool(t.active[n]), "descendant": t.descendants[n],
             "played_games": int(t.played_games[n]), "scores": [int(x) for x in t.tournament_scores[n]],
             "positions": [float(x) for x in t.tournament_positions[n]],
             "wins": [float(x) for x in t.tournament_wins[n]], "elo": float(t.elos[n][-1]),
             "elos": [float(x) for x in t.elos[n]]} for n in t.agents]


def gen_evolve(ref, out):
    """F13.  Seeded reference tournaments of DrunkHamster agents with
    `evolve` between blocks of games (tournament.py:54-130): np.random.seed(
    seed); Tournament(lo, hi); add_player a0..a{K-1}; then per block
    play_game() x games followed by evolve(copies, max_players,
    max_per_descendant, metric).  copy_player round-trips the agent through
    temp_model.pt in the working directory (run here in a temporary one;
    torch.load of that file, which torch.save wrote a line before in this
    process, needs weights_only=False on torch >= 2.6).  Elo: the build's
    restatement of multi_elo stands in (see _restated_elo).  Recorded: every
    game (seat names, results) and the roster after each evolve (dict order,
    active flags, families, tallies, Elo), plus the ranking keys."""
    import functools

    import torch
    from rl_6_nimmt.agents import DrunkHamster
    from rl_6_nimmt.tournament import Tournament

    E = _restated_elo()
    cases_in = [
        # seed, K, lo, hi, [(games, evolve kwargs or None)]
        (500, 5, 2, 4, [(6, dict(copies=(2,), max_players=None, max_per_descendant=2, metric="elo")),
                        (6, dict(copies=(2, 1), max_players=5, max_per_descendant=2, metric="tournament_scores")),
                        (4, None)]),
        (501, 5, 2, 4, [(8, dict(copies=(2,), max_players=4, max_per_descendant=2, metric="tournament_positions")),
                        (8, dict(copies=(3,), max_players=6, max_per_descendant=1, metric="tournament_wins")),
                        (4, None)]),
        (502, 6, 3, 4, [(10, dict(copies=(2, 2), max_players=None, max_per_descendant=None, metric="tournament_wins")),
                        (6, dict(copies=(1,), max_players=5, max_per_descendant=3, metric="elo")),
                        (5, dict(copies=(2,), max_players=6, max_per_descendant=2, metric="tournament_positions")),
                        (3, None)]),
        (503, 4, 2, 3, [(12, dict(copies=(2,), max_players=None, max_per_descendant=2, metric="tournament_positions")),
                        (7, dict(copies=(), max_players=4, max_per_descendant=1, metric="tournament_scores")),
                        (4, None)]),
        (504, 8, 2, 4, [(16, dict(copies=(2, 2, 1), max_players=7, max_per_descendant=2, metric="elo")),
                        (10, dict(copies=(2,), max_players=None, max_per_descendant=1, metric="tournament_scores")),
                        (5, None)]),
    ]
    real_load = torch.load
    cwd = os.getcwd()
    tmp = tempfile.mkdtemp(prefix="sechs_evolve_")
    cases = []
    try:
        os.chdir(tmp)
        torch.load = functools.partial(real_load, weights_only=False)
        for seed, K, lo, hi, blocks in cases_in:
            np.random.seed(seed)
            t = Tournament(min_players=lo, max_players=hi)
            for i in range(K):
                t.add_player(f"a{i}", DrunkHamster())

            def elos(names, scores, t=t):
                places = t._compute_absolute_positions(scores)
                return E.calc_elo([E.EloPlayer(place=pl, elo=t.elos[n][-1]) for pl, n in zip(places, names)], t.elo_k)

            t._compute_elos = elos
            rec = []
            for games, ev in blocks:
                played = _play_recorded_games(t, games)
                entry = {"games": played}
                if ev is not None:
                    entry["evolve"] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in ev.items()}
                    entry["before"] = _roster(t)
                    t.evolve(**ev)
                    entry["after"] = _roster(t)
                rec.append(entry)
            cases.append({"seed": seed, "num_agents": K, "min_players": lo, "max_players": hi, "blocks": rec,
                          "total_games": int(t.total_games)})
            print(f"  evolve seed={seed}: roster {[r['name'] for r in _roster(t) if r['active']]}", flush=True)
    finally:
        torch.load = real_load
        os.chdir(cwd)
    with open(os.path.join(out, "evolve_games.json"), "w") as f:
        json.dump({"protocol": "np.random.seed(seed); t = Tournament(min_players, max_players); add_player(a{i}, "
                               "DrunkHamster()) for i < num_agents; per block: t.play_game() x len(games), then "
                               "t.evolve(**evolve) when given; Elo by the build's multi_elo restatement (elo.py); "
                               "rosters in the reference's dict order", "cases": cases}, f)


# ----------------------------------------------------------------------------
# F15: PriorityReplayBuffer traces
# ----------------------------------------------------------------------------
PER_SHAPES = [(5, 3, 4, 40), (8, 8, 8, 40), (100, 60, 10, 120), (100, 250, 16, 120)]  # (cap, nstore, n, rounds)
PER_MARGIN = 1e-10  # of the total priority


def _per_margin(tree, n, us):
    """smallest |v - threshold| / total over the descents of sample(n) with uniforms us"""
    total = tree[0]
    seg = total / n
    worst = float("inf")
    for i, u in enumerate(us):
        v = seg * i + u * seg
        node = 0
        while 2 * node + 1 < len(tree):
            left = tree[2 * node + 1]
            worst = min(worst, abs(v - left) / total)
            if v <= left:
                node = 2 * node + 1
            else:
                v -= left
                node = 2 * node + 2
    return worst


def _recorded_sample(buf, n, sample=None):
    """buf.sample(n) and the uniforms it drew from Python's `random`, and the descents' margin"""
    import random

    tree = buf.tree.tree.copy()
    before = random.getstate()
    out = (sample or buf.sample)(n)
    after = random.getstate()
    random.setstate(before)
    us = [random.random() for _ in range(n)]
    assert random.getstate() == after, "sample(n) drew something other than n uniforms"
    return out, us, _per_margin(tree, n, us), tree


def gen_per(ref, out):
    import random

    from rl_6_nimmt.utils.replay_buffer import PriorityReplayBuffer

    traces, arrays = [], {}
    for cap, nstore, n, rounds in PER_SHAPES:
        random.seed(cap)
        np.random.seed(cap)
        buf = PriorityReplayBuffer(max_length=cap)
        stores = 0
        for _ in range(nstore):
            buf.store(k=stores)
            stores += 1
        rec, snaps, repeats, worst = [], {}, 0, float("inf")
        for r in range(rounds):
            buf.store(k=stores)
            stores += 1
            (idx, weights, batch), us, margin, tree = _recorded_sample(buf, n)
            worst = min(worst, margin)
            repeats += len(set(idx.tolist())) < n
            errors = np.random.random_sample(n) * 1.5
            sent = errors.copy()  # batch_update adds epsilon in place
            buf.batch_update(idx, sent)
            rec.append({"u": us, "errors": errors, "idx": [int(x) for x in idx], "weights": weights,
                        "priorities": tree[idx], "beta": float(buf.beta), "len": len(buf)})
            if (r + 1) % 20 == 0 or r == rounds - 1:
                snaps[r] = buf.tree.tree.copy()
        assert worst >= PER_MARGIN, f"capacity {cap}: a descent within {worst} of a threshold"
        assert repeats >= 1, f"capacity {cap}: no round sampled an index twice"
        ti = len(traces)
        for key in ("u", "errors", "weights", "priorities", "beta"):
            arrays[f"t{ti}_{key}"] = np.array([rd[key] for rd in rec], dtype=np.float64)
        arrays[f"t{ti}_tree"] = np.stack([snaps[r] for r in sorted(snaps)])
        arrays[f"t{ti}_idx"] = np.array([rd["idx"] for rd in rec], dtype=np.int64)
        arrays[f"t{ti}_len"] = np.array([rd["len"] for rd in rec], dtype=np.int64)
        traces.append({"capacity": cap, "nstore": nstore, "n": n, "rounds": rounds,
                       "snapshots": sorted(snaps), "min_margin": worst, "rounds_with_repeats": int(repeats)})
    np.savez_compressed(os.path.join(out, "per_traces.npz"), **arrays)
    with open(os.path.join(out, "per_traces.json"), "w") as f:
        json.dump({"protocol": "random.seed(cap); np.random.seed(cap); buf = PriorityReplayBuffer(cap); nstore x "
                               "store(k=<store count>); per round: store, sample(n), batch_update(idx, errors) with "
                               "errors = np.random.random_sample(n) * 1.5.  per_traces.npz, t<i>_*, [round][...]: idx = "
                               "the tree indices sampled, len = len(buf) (int64); f64: u = the uniforms sample drew from random.random(), errors "
                               "(before epsilon is added), weights, priorities = the leaves sampled, beta; tree = all "
                               "nodes after each round of `snapshots`.  min_margin = smallest |v - threshold| / total "
                               "over all descents (asserted >= 1e-10).  Python semantics of the sampler (numba.jit is "
                               "a no-op here)",
                   "traces": traces}, f)


# ----------------------------------------------------------------------------
# F16: the DQN agents in training sessions
# ----------------------------------------------------------------------------
DQN_CLASSES = ["DQNVanilla", "DDQNAgent", "DQN_PRBAgent", "DDQN_PRBAgent"]
DQN_KW = {"history_length": 256, "minibatch": 16}
DQN_GAMES = 6
DQN_GAP = 1e-3
# the agents' priorities are float32 (numpy keeps the tensor's dtype through the power): two libm's powf may
# differ by an ulp, 6e-8 of a leaf, so the sessions keep well clear of that, not just of PER_MARGIN
DQN_MARGIN = 1e-6


def _dqn_session(cls_name, seed, eps_const, extra_kw=None, record_games=0, min_leaf=None):
    """one seeded session, or None if the seed is too close to a tie.  record_games: also return the learn
    calls and the replay's stored transitions of that many first games (a fifth element).  min_leaf: reject
    the seed as well when a PER sample finds a smaller minimum leaf among the held items (DQNVAR_MIN_LEAF)"""
    import random

    import torch
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.play import GameSession

    torch.manual_seed(seed)
    kw = dict(DQN_KW, **(extra_kw or {}))
    if eps_const is not None:
        kw["eps_func"] = lambda episode, _c=eps_const: _c
    ag = getattr(A, cls_name)(**kw)
    agents = [ag] + [A.DrunkHamster() for _ in range(3)]
    ag.train()
    init = {k: v.detach().numpy().astype(np.float32).copy() for k, v in ag.state_dict().items()}
    tr = {"steps": [], "losses": [], "per_idx": []}
    worst = {"gap": float("inf"), "margin": float("inf"), "leaf": float("inf")}
    sel, lrn = ag._action_selection, ag.learn

    def sel_rec(scores, **k):
        act, info = sel(scores, **k)
        if info["value"] != -1:  # greedy: `scores` is masked in place by now
            top = np.sort(scores.numpy()[list(k["legal_actions"])])[::-1]
            if len(top) > 1:
                worst["gap"] = min(worst["gap"], float(top[0] - top[1]))
        tr["steps"].append([int(act), float(info["value"]), float(info["eps"])])
        return act, info

    def lrn_rec(*a, **k):
        loss = lrn(*a, **k)
        tr["losses"].append(float(loss[0]))
        return loss

    ag._action_selection, ag.learn = sel_rec, lrn_rec
    game = {"i": 0}
    calls, stored = [[] for _ in range(record_games)], [[] for _ in range(record_games)]
    if record_games:
        def ints(x):
            v = np.asarray(x, dtype=np.float64)
            assert np.array_equal(v, np.round(v))
            return [int(t) for t in v]

        def transition(k):
            return {"state": ints(k["state"]), "reward": float(k["reward"]), "action": int(k["action"]),
                    "next_state": ints(k["next_state"]), "done": bool(k["done"])}

        def lrn_calls(state, reward, action, done, next_state, *a, **k):
            if game["i"] < record_games:
                calls[game["i"]].append(transition(dict(state=state, reward=reward, action=action,
                                                        next_state=next_state, done=done)))
            return lrn_rec(state, reward, action, done, next_state, *a, **k)

        hist_store = ag.history.store

        def store_rec(**k):
            if game["i"] < record_games:
                assert isinstance(k["reward"], float)
                stored[game["i"]].append(transition(k))
            return hist_store(**k)

        ag.learn, ag.history.store = lrn_calls, store_rec
    prb = "PRB" in cls_name or "D3QN" in cls_name
    if prb:
        buf = ag.history
        smp = buf.sample

        def smp_rec(n):
            first = len(buf.tree.tree) - buf.tree.capacity
            worst["leaf"] = min(worst["leaf"], float(np.min(buf.tree.tree[first: first + buf.tree.num_items])))
            res, us, margin, _ = _recorded_sample(buf, n, smp)
            worst["margin"] = min(worst["margin"], margin)
            tr["per_idx"].append([int(x) for x in res[0]])
            return res

        buf.sample = smp_rec
    np.random.seed(seed)
    random.seed(seed)
    sess = GameSession(*agents)
    for gi in range(DQN_GAMES):
        game["i"] = gi
        sess.play_game()
    if worst["gap"] < DQN_GAP or worst["margin"] < DQN_MARGIN:
        return None
    if min_leaf is not None and worst["leaf"] < min_leaf:
        return None
    final = {k: v.detach().numpy().astype(np.float32).copy() for k, v in ag.state_dict().items()}
    kw_json = dict(DQN_KW, **(extra_kw or {}))
    rec = {"agent": cls_name, "seed": seed, "games": DQN_GAMES, "kwargs": kw_json, "eps_const": eps_const,
           "results": [[int(x) for x in r] for r in sess.results],            "greedy_steps": int(sum(1 for s in tr["steps"] if s[1] != -1)),
           "min_gap": None if worst["gap"] == float("inf") else worst["gap"]}
    if prb:
        rec.update(beta=float(ag.history.beta), total_priority=float(ag.history.tree.total_priority),
                   len=len(ag.history), min_margin=worst["margin"])
        if min_leaf is not None:
            rec.update(min_leaf=worst["leaf"])
    series = {"actions": np.array([s[0] for s in tr["steps"]], dtype=np.int64),
              "values": np.array([s[1] for s in tr["steps"]]), "eps": np.array([s[2] for s in tr["steps"]]),
              "losses": np.array(tr["losses"])}
    if prb:
        series["per_idx"] = np.array(tr["per_idx"], dtype=np.int64)
    if record_games:
        return rec, init, final, series, {"learn_calls": calls, "stored": stored}
    return rec, init, final, series


def gen_dqn(ref, out):
    sessions, arrays = [], {}
    for ci, cls_name in enumerate(DQN_CLASSES):
        for eps_const in (None, 0.3):
            seed = 10 * ci + (5 if eps_const else 0)
            while True:
                got = _dqn_session(cls_name, seed, eps_const)
                if got is not None:
                    break
                seed += 100  # rejected: a near-tie between the two best legal Q values or at a tree threshold
            rec, init, final, series = got
            si = len(sessions)
            for k, v in series.items():
                arrays[f"s{si}_{k}"] = v
            for k, v in init.items():
                arrays[f"s{si}_init_{k}"] = v
            for k, v in final.items():
                arrays[f"s{si}_final_{k}"] = v
            sessions.append(rec)
    np.savez_compressed(os.path.join(out, "dqn_weights.npz"), **arrays)
    with open(os.path.join(out, "dqn_games.json"), "w") as f:
        json.dump({"protocol": "torch.manual_seed(seed); agent = <agent>(**kwargs[, eps_func = constant eps_const]); "
                               "three DrunkHamster; agent.train(); np.random.seed(seed); random.seed(seed); "
                               "GameSession(agent, hamsters...).play_game() x games.  dqn_weights.npz: s<i>_actions / _values / _eps = "
                               "the move, info.value and info.eps of every forward, s<i>_losses = learn()[0] per "
                               "step, s<i>_per_idx = the tree indices of every PER sample; here beta / total_priority / len = the replay at the end.  Seeds with a greedy "
                               "decision whose two best legal Q values are within 1e-3 (min_gap), or a PER descent "
                               "within 1e-6 x total of a threshold (min_margin; float32 priorities), were rejected.  Weights: "
                               "dqn_weights.npz s<i>_init_* / s<i>_final_* (agent.state_dict()).  Python semantics of "
                               "the PER sampler (numba.jit is a no-op here)",
                   "sessions": sessions}, f)


# ----------------------------------------------------------------------------
# F17: the duelling and n-step DQN agents in training sessions
# ----------------------------------------------------------------------------
DQNVAR_CLASSES = [("DuellingDQNAgent", {}), ("DuellingDDQNAgent", {}), ("DuellingDDQN_PRBAgent", {}),
                  ("D3QN_PRB_NStep", {"n_steps": 3})]
DQNVAR_RECORD_GAMES = 2
# A third rejection rule for the prioritised sessions.  Every importance weight of a sample is divided by the
# largest one, (min leaf / total) ** -beta (replay_buffer.py:165,180), and a leaf is (|q - target| + 0.01) ** 0.6:
# when the smallest held leaf comes from a TD error that nearly cancels, fp32 rounding on another CPU moves every
# weight of the minibatch, and with them the loss, with d ln(loss) = beta * 0.6 * d|err| / (|err| + 0.01) and
# beta < 0.45 in six games.  The floor of a leaf is 0.01 ** 0.6 = 0.063 and most seeds come within 0.07..0.13 of
# it.  The sessions' losses are compared to a relative 1e-3; allowing the Q values (magnitudes up to 32 here) a
# drift of 40 fp32 ulps = 1.5e-4 by the end of a session -- rounding amplified by sixty Adam steps -- asks for
# |err| + 0.01 >= 0.45 * 0.6 * 1.5e-4 / 1e-3 = 0.041, i.e. leaf >= 0.041 ** 0.6 = 0.147; about one seed in six
# qualifies.  (Seed 20 of DuellingDDQN_PRBAgent held a leaf of 0.077, from |err| = 0.004: the reference itself
# moved its last four losses by 7e-5 under a 1e-6 change of one initial weight.)
DQNVAR_MIN_LEAF = 0.15


def gen_dqnvar(ref, out):
    sessions, arrays = [], {}
    for ci, (cls_name, extra) in enumerate(DQNVAR_CLASSES):
        nstep = "n_steps" in extra
        for eps_const in (None, 0.3):
            seed = 10 * ci + (5 if eps_const else 0)
            while True:
                got = _dqn_session(cls_name, seed, eps_const, extra_kw=extra,
                                   record_games=DQNVAR_RECORD_GAMES if nstep else 0,
                                   min_leaf=DQNVAR_MIN_LEAF if "PRB" in cls_name else None)
                if got is not None:
                    break
                seed += 100  # rejected, by the F16 rules or DQNVAR_MIN_LEAF
            rec, init, final, series = got[:4]
            if nstep:
                rec.update(got[4])
            si = len(sessions)
            for k, v in series.items():
                arrays[f"s{si}_{k}"] = v
            for k, v in init.items():
                if k.startswith("dqn_net_target."):  # the local net's copy (soft_update with tau = 1): not stored
                    assert np.array_equal(v, init[k.replace("dqn_net_target.", "dqn_net_local.", 1)])
                    continue
                arrays[f"s{si}_init_{k}"] = v
            for k, v in final.items():
                arrays[f"s{si}_final_{k}"] = v
            sessions.append(rec)
    np.savez_compressed(os.path.join(out, "dqn_variant_weights.npz"), **arrays)
    with open(os.path.join(out, "dqn_variant_games.json"), "w") as f:
        json.dump({"protocol": "dqn_games.json's protocol and rejection rules for DuellingDQNAgent, DuellingDDQNAgent, "
                               "DuellingDDQN_PRBAgent and D3QN_PRB_NStep (kwargs holds n_steps); arrays in "
                               "dqn_variant_weights.npz under the same names (the prioritised sessions also reject a seed whose smallest held leaf at "
                               "any sample is below 0.15 (min_leaf): an ill-conditioned weight normalisation), without s<i>_init_dqn_net_target.* (equal to "
                               "s<i>_init_dqn_net_local.*).  The n-step sessions also hold, for the "
                               "first two games: learn_calls[game] = the (state, reward, action, next_state, done) of "
                               "every learn() call, stored[game] = the transitions the replay's store() received, in "
                               "store order, the reward a float64 (Python float)",
                   "sessions": sessions}, f)


# ----------------------------------------------------------------------------
# F18: the noisy DQN agents in training sessions
# ----------------------------------------------------------------------------
DQNNOISY_CLASSES = [("Noisy_DQN", {}), ("Noisy_D3QN", {}), ("Noisy_D3QN_PRB_NStep", {"n_steps": 3})]


def _noisy_session(cls_name, seed, extra_kw):
    """_dqn_session for the noisy agents: info has no "eps" and the scores are not masked in place, so the gap is
    taken between the two best of scores[legal]; the same rejection rules.  torch's CPU generator drives the
    initial weights and every noise draw."""
    import random

    import torch
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.play import GameSession

    torch.manual_seed(seed)
    kw = dict(DQN_KW, **extra_kw)
    ag = getattr(A, cls_name)(**kw)
    agents = [ag] + [A.DrunkHamster() for _ in range(3)]
    ag.train()

    def weights():  # the epsilon buffers are redrawn by every forward: not part of the record
        return {k: v.detach().numpy().astype(np.float32).copy() for k, v in ag.state_dict().items()
                if ".epsilon_" not in k}

    init = weights()
    tr = {"steps": [], "losses": [], "per_idx": []}
    worst = {"gap": float("inf"), "margin": float("inf"), "leaf": float("inf")}
    sel, lrn = ag._action_selection, ag.learn

    def sel_rec(scores, **k):
        act, info = sel(scores, **k)
        assert set(info) == {"value"}
        top = np.sort(scores.numpy()[list(k["legal_actions"])])[::-1]
        if len(top) > 1:
            worst["gap"] = min(worst["gap"], float(top[0] - top[1]))
        tr["steps"].append([int(act), float(info["value"])])
        return act, info

    def lrn_rec(*a, **k):
        loss = lrn(*a, **k)
        tr["losses"].append(float(loss[0]))
        return loss

    ag._action_selection, ag.learn = sel_rec, lrn_rec
    prb = "PRB" in cls_name
    if prb:
        buf = ag.history
        smp = buf.sample

        def smp_rec(n):
            first = len(buf.tree.tree) - buf.tree.capacity
            worst["leaf"] = min(worst["leaf"], float(np.min(buf.tree.tree[first: first + buf.tree.num_items])))
            res, us, margin, _ = _recorded_sample(buf, n, smp)
            worst["margin"] = min(worst["margin"], margin)
            tr["per_idx"].append([int(x) for x in res[0]])
            return res

        buf.sample = smp_rec
    np.random.seed(seed)
    random.seed(seed)
    sess = GameSession(*agents)
    for _ in range(DQN_GAMES):
        sess.play_game()
    if worst["gap"] < DQN_GAP or worst["margin"] < DQN_MARGIN or (prb and worst["leaf"] < DQNVAR_MIN_LEAF):
        return None
    final = weights()
    rec = {"agent": cls_name, "seed": seed, "games": DQN_GAMES, "kwargs": kw, "results": [[int(x) for x in r] for r in sess.results],
           "min_gap": worst["gap"]}
    if prb:
        rec.update(beta=float(ag.history.beta), total_priority=float(ag.history.tree.total_priority),
                   len=len(ag.history), min_margin=worst["margin"], min_leaf=worst["leaf"])
    series = {"actions": np.array([s[0] for s in tr["steps"]], dtype=np.int64),
              "values": np.array([s[1] for s in tr["steps"]]), "losses": np.array(tr["losses"])}
    if prb:
        series["per_idx"] = np.array(tr["per_idx"], dtype=np.int64)
    return rec, init, final, series


def gen_dqnnoisy(ref, out):
    sessions, arrays = [], {}
    for ci, (cls_name, extra) in enumerate(DQNNOISY_CLASSES):
        seed = 10 * ci
        while True:
            got = _noisy_session(cls_name, seed, extra)
            if got is not None:
                break
            seed += 100  # rejected, by the F16 rules or DQNVAR_MIN_LEAF
        rec, init, final, series = got
        si = len(sessions)
        for k, v in series.items():
            arrays[f"s{si}_{k}"] = v
        for k, v in init.items():
            if k.startswith("dqn_net_target."):  # the local net's copy (soft_update with tau = 1): not stored
                assert np.array_equal(v, init[k.replace("dqn_net_target.", "dqn_net_local.", 1)])
                continue
            arrays[f"s{si}_init_{k}"] = v
        for k, v in final.items():
            arrays[f"s{si}_final_{k}"] = v
        sessions.append(rec)
    np.savez_compressed(os.path.join(out, "dqn_noisy_weights.npz"), **arrays)
    with open(os.path.join(out, "dqn_noisy_games.json"), "w") as f:
        json.dump({"protocol": "dqn_games.json's protocol for Noisy_DQN, Noisy_D3QN and Noisy_D3QN_PRB_NStep (kwargs holds "
                               "n_steps; no eps_func): torch.manual_seed(seed) drives the initial weights and every noise "
                               "draw of the session.  dqn_noisy_weights.npz: s<i>_actions / _values = the move and "
                               "info.value of every forward (info has no eps), s<i>_losses, s<i>_per_idx (the "
                               "prioritised session), s<i>_init_* / s<i>_final_* = agent.state_dict() without the "
                               "epsilon_input / epsilon_output buffers and without s<i>_init_dqn_net_target.* (equal to "
                               "s<i>_init_dqn_net_local.*).  Rejected seeds: a decision whose two best of scores[legal] "
                               "are within 1e-3 (min_gap), a PER descent within 1e-6 x total of a threshold "
                               "(min_margin), a smallest held leaf below 0.15 at any sample (min_leaf)",
                   "sessions": sessions}, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    ref = import_reference()
    steps = [
        ("mt", gen_mt),
        ("notebook", gen_notebook),
        ("random", gen_random_games),
        ("edge", gen_edge_cases),
        ("puct", gen_puct),
        ("positions", gen_positions),
        ("mcs", gen_mcs),
        ("customed", gen_customed),
        ("reinforce", gen_reinforce),
        ("acer", gen_acer),
        ("tournament", gen_tournament),
        ("evolve", gen_evolve),
        ("per", gen_per),
        ("dqn", gen_dqn),
        ("dqnvar", gen_dqnvar),
        ("dqnnoisy", gen_dqnnoisy),
    ]
    for name, fn in steps:
        if args.only and name not in args.only.split(","):
            continue
        t = time.time()
        if fn is gen_mt:
            fn(out)
        else:
            fn(ref, out)
        print(f"{name}: {time.time() - t:.1f}s", flush=True)


if __name__ == "__main__":
    main()
