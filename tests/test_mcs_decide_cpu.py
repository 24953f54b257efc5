"""The oracle's one-decision MCS (O.mcs_decide) against numpy itself.

The model below restates MCSAgent._mcts (agents/mcts.py:91-172) in plain
Python on a real np.random.RandomState: set_state sets the stream,
rs.shuffle(list(avail)) deals (mcts.py:116-127), rs.choice(np.array(hand,
np.int32), size=1)[0] picks every seat's move (mcts.py:187-188), and
O.Game.set_position / step play the game.  O.mcs_decide must give the same
per-move sums and counts, card, Q6 flag and final get_state() key and pos.
The GPU tests of the wave kernel (test_gpu_mcs_wave.py) then compare with
O.mcs_decide.
"""
import math
import warnings

import numpy as np
import pytest

from oracle import oracle as O


def model_decide(board, hand, avail, num_players, mc_per_card, mc_max, key, pos):
    rs = np.random.RandomState()
    rs.set_state(("MT19937", np.asarray(key, dtype=np.uint32), int(pos), 0, 0.0))
    hand = list(hand)
    n = len(hand)
    n_mc = min(mc_max, mc_per_card * math.factorial(n))
    outcomes = {a: [] for a in hand}
    for _ in range(n_mc):
        cards = list(avail)
        rs.shuffle(cards)
        hands = [list(hand)]
        for _ in range(num_players - 1):
            hands.append(sorted(cards[:n]))
            del cards[:n]
        G = O.Game(num_players)
        G.set_position(board, hands)
        first, outcome = None, 0
        while not G.done():
            acts = []
            for legal in G.hands:
                a = int(rs.choice(np.array(legal, dtype=np.int32), size=1)[0])
                acts.append(a)
                if first is None:
                    first = a
            bad, rew = G.step(acts)
            assert bad == -1
            outcome += int(rew[0])
        outcomes[first].append(outcome)
    # _choose_action_from_outcomes: np.mean([]) is NaN and never '>'; the
    # reference then raises from its debug line (quirk Q6)
    best, best_mean = hand[0], -float("inf")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for a in hand:
            m = np.mean(outcomes[a])
            if m > best_mean:
                best, best_mean = a, m
    sums = np.zeros(10, dtype=np.int32)
    counts = np.zeros(10, dtype=np.int32)
    for i, a in enumerate(hand):
        sums[i], counts[i] = sum(outcomes[a]), len(outcomes[a])
    st = rs.get_state()
    return best, any(len(o) == 0 for o in outcomes.values()), sums, counts, st[1], int(st[2])


# (num_players, hand size, mc_per_card, mc_max, start pos, seed)
CASES = [
    (2, 10, 10, 100, 0, 11),
    (2, 2, 10, 100, 624, 12),    # n_mc = 20
    (2, 3, 1, 1000, 600, 13),    # n_mc = 3! = 6
    (4, 10, 10, 100, 623, 14),
    (4, 5, 10, 65, 600, 15),
    (4, 2, 0, 50, 0, 16),        # no playout at all
    (8, 10, 10, 100, 600, 17),   # 161 draws per playout
    (8, 4, 1, 1000, 624, 18),    # n_mc = 24
    (8, 2, 10, 30, 623, 19),
    (10, 10, 10, 64, 0, 20),     # 179 draws per playout
    (10, 10, 10, 100, 624, 21),
    (10, 6, 10, 30, 623, 22),
    (10, 2, 1, 1000, 600, 23),   # n_mc = 2
]


@pytest.mark.parametrize("K,n,mpc,mmax,pos,seed", CASES)
def test_mcs_decide_matches_numpy_model(K, n, mpc, mmax, pos, seed):
    board, hand, avail = O.mcs_position(K, n, seed)
    assert len(hand) == n and len(avail) >= (K - 1) * n
    key = np.random.RandomState(1000 + seed).get_state()[1]
    want = model_decide(board, hand, avail, K, mpc, mmax, key, pos)
    got = O.mcs_decide(board, hand, avail, K, mpc, mmax, key, pos)
    assert got[0] == want[0] and got[1] == want[1]
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert int(got[3].sum()) == min(mmax, mpc * math.factorial(n))
    assert np.array_equal(got[4], want[4]) and got[5] == want[5]


def test_cases_cover_q6_and_not_q6():
    seen = set()
    for K, n, mpc, mmax, pos, seed in CASES:
        board, hand, avail = O.mcs_position(K, n, seed)
        key = np.random.RandomState(1000 + seed).get_state()[1]
        seen.add(O.mcs_decide(board, hand, avail, K, mpc, mmax, key, pos)[1])
    assert seen == {False, True}


def test_mcs_decide_edges():
    key = np.random.RandomState(5).get_state()[1]
    # one card: played without a search, nothing drawn (mcts.py:52-53)
    board, hand, avail = O.mcs_position(4, 1, 31)
    card, q6, sums, counts, key2, pos2 = O.mcs_decide(board, hand, avail, 4, 10, 100, key, 77)
    assert card == hand[0] and not q6 and not sums.any() and not counts.any()
    assert np.array_equal(key2, key) and pos2 == 77
    # a memory too small to deal the opponents from: -1, nothing drawn
    board, hand, avail = O.mcs_position(4, 5, 32)
    for short in (avail[:14], []):
        card, q6, sums, counts, key2, pos2 = O.mcs_decide(board, hand, short, 4, 10, 100, key, 77)
        assert card == -1 and not q6 and not sums.any() and not counts.any()
        assert np.array_equal(key2, key) and pos2 == 77
    # exactly enough cards is enough
    assert O.mcs_decide(board, hand, avail[:15], 4, 10, 100, key, 77)[0] in hand


def test_rng_from_numpy_continues_the_stream():
    rs = np.random.RandomState(9)
    rs.random_sample(1000)  # somewhere inside a later round
    st = rs.get_state()
    rng = O.Rng.from_numpy(st[1], st[2])
    want = rs.randint(0, 2**32, size=700, dtype=np.uint32)
    assert [rng.next() for _ in range(700)] == [int(w) for w in want]
