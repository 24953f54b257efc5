"""Host model of a Philox tournament handle playing a mixed league: the stream
law of include/sechs.h (at sn_league_step), written over what oracle/oracle.py
exposes -- Rng(RNG_PHILOX, key, stream) with interval / shuffle / s.ctr, Game
with reset / set_position / step / random_action, and mcs_memorize.

`league` is oracle.league_records' loop with three changes: the slot's stream
is Rng(RNG_PHILOX, seed, game_offset + j); MCS seats search by the law (one
Philox stream per playout, `search`); EXTERNAL seats take given cards.
"""
import math
from fractions import Fraction

import numpy as np

from oracle import oracle as O

MCS_KEY = 0x4D435331
M32 = 0xFFFFFFFF


def mcs_key(seed, c0):
    """the 64-bit key (lo | hi << 32) of the decisions of a step that began at main counter c0"""
    lo = (seed & M32) ^ (c0 & M32)
    hi = ((seed >> 32) & M32) ^ ((c0 >> 32) & M32) ^ MCS_KEY
    return lo | (hi << 32)


def mcs_stream(gid, p, n, j=0):
    """the stream word of playout j of seat p of game gid deciding at a hand of n cards"""
    return ((gid & M32) << 32) | (p << 28) | (j << 8) | n


def num_playouts(n, mc_per_card, mc_max):
    return min(mc_max, mc_per_card * math.factorial(n))


def search(board, hand, avail, k, mc_per_card, mc_max, key, stream0, streams=None):
    """One MCS decision of a k-player game: board = the rows' card lists, hand = the
    legal cards (n >= 2), avail = the card memory, (key, stream0) = the decision's
    Philox key and its stream word with j = 0.  Returns (card, q6, sums [10],
    counts [10]); card = -1 with zeroed sums where the hand is empty or the memory
    does not hold (k - 1) n <= A <= 104 cards.  streams: a list that collects
    every playout's (key, stream)."""
    hand, avail = sorted(int(c) for c in hand), sorted(int(c) for c in avail)
    n, A = len(hand), len(avail)
    sums, counts = np.zeros(O.HAND, dtype=np.int32), np.zeros(O.HAND, dtype=np.int32)
    if n == 0 or A < (k - 1) * n or A > O.MAX_CARDS:
        return -1, False, sums, counts
    for j in range(num_playouts(n, mc_per_card, mc_max)):
        stream = stream0 | (j << 8)
        if streams is not None:
            streams.append((key, stream))
        rng = O.Rng(O.RNG_PHILOX, key, stream)
        cards = rng.shuffle(np.array(avail, dtype=np.int32))  # ascending memory, numpy's shuffle
        g = O.Game(k)
        g.set_position(board, [hand] + [sorted(int(c) for c in cards[(q - 1) * n: q * n]) for q in range(1, k)])
        first, outcome = None, 0
        for _ in range(n):
            acts = [g.random_action(rng, q) for q in range(k)]  # idx = random_interval(cards left - 1), seat order
            if first is None:
                first = acts[0]
            bad, rew = g.step(acts)
            assert bad < 0
            outcome += int(rew[0])  # rewards are -penalties
        i = hand.index(first)
        sums[i] += outcome
        counts[i] += 1
    # _choose_action_from_outcomes: best mean in legal order, strict '>'; a move without a playout never wins
    best, best_mean, q6 = 0, None, False
    for i in range(n):
        if counts[i] == 0:
            q6 = True
            continue
        mean = Fraction(int(sums[i]), int(counts[i]))
        if best_mean is None or mean > best_mean:
            best, best_mean = i, mean
    return hand[best], q6, sums, counts


def league(kinds, min_players, max_players, mc_per_card=10, mc_max=100, seed=0, game_offset=0, slots=1, games=1,
           external=None):
    """kinds: one of 'R' (DrunkHamster), 'M' (MCSAgent) or 'E' (external) per agent;
    mc_per_card / mc_max: scalars or one per agent; external(game, slot, step, seat,
    oracle game) -> the card of an 'E' seat.  Returns a dict:
      records [games, slots, 1 + max_players] int32 in the device's format,
      rewards [10 games, slots, max_players] int32 (0 past k),
      ctr     [slots] the main streams' word counters at the end,
      q6      (slot, game) pairs with an MCS decision where a legal move got no playout,
      streams every playout's (key, stream), in play order,
      main    every slot's main (key, stream)."""
    K, N = len(kinds), int(max_players)
    mpc = np.broadcast_to(np.asarray(mc_per_card, dtype=np.int64), (K,))
    mmx = np.broadcast_to(np.asarray(mc_max, dtype=np.int64), (K,))
    rec = np.zeros((games, slots, 1 + N), dtype=np.int32)
    rewards = np.zeros((O.HAND * games, slots, N), dtype=np.int32)
    ctr = np.zeros(slots, dtype=np.uint64)
    q6_pairs, streams, main = 0, [], []
    for j in range(slots):
        gid = game_offset + j
        rng = O.Rng(O.RNG_PHILOX, seed, gid)
        main.append((seed, gid))
        for e in range(games):
            k = min_players + rng.interval(max_players - min_players)
            seats = [int(a) for a in rng.shuffle(np.arange(K))[:k]]
            g = O.Game(k)
            g.reset(rng)
            mem = [[] for _ in range(k)]
            q6_game = False
            for t in range(O.HAND):
                n = O.HAND - t
                c0 = int(rng.s.ctr)  # as the step begins, before any RANDOM seat of it draws
                acts = []
                for p, a in enumerate(seats):
                    if kinds[a] == "R":
                        acts.append(g.random_action(rng, p))
                    elif kinds[a] == "E":
                        acts.append(int(external(e, j, t, p, g)))
                    else:
                        mem[p] = O.mcs_memorize(mem[p], g, p)
                        if n == 1:
                            acts.append(g.hands[p][0])  # played without a search
                            continue
                        card, q6, _, _ = search(g.board, g.hands[p], mem[p], k, int(mpc[a]), int(mmx[a]),
                                                mcs_key(seed, c0), mcs_stream(gid, p, n), streams)
                        assert card >= 0
                        q6_game |= q6
                        acts.append(card)
                bad, rew = g.step(acts)
                assert bad < 0
                rewards[O.HAND * e + t, j, :k] = rew
            w = k
            for p, a in enumerate(seats):
                w |= a << (4 + 4 * p)
            rec[e, j, 0] = w
            rec[e, j, 1: 1 + k] = [-s for s in g.scores]
            q6_pairs += int(q6_game)
        ctr[j] = int(rng.s.ctr)
    return {"records": rec, "rewards": rewards, "ctr": ctr, "q6": q6_pairs, "streams": streams, "main": main}
