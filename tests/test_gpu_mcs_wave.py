"""The wave MCS decision kernel (sn_mcs_decide_exact, k_mcs_decide_wave)
pinned per decision.

Every case compares everything a decision produces -- actions (the Q6
encoding -(card)-2 included), the per-move sums and counts, and the advanced
numpy (key, pos) -- with the oracle's O.mcs_decide, exactly.  O.mcs_decide
is itself pinned to numpy's RandomState by tests/test_mcs_decide_cpu.py.
Positions come from oracle games (O.mcs_position), streams from
np.random.RandomState(seed).get_state() with pos set on purpose.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5  # what the output buffers hold before a launch


@functools.lru_cache(maxsize=None)
def position(K, n, seed=0):
    return O.mcs_position(K, n, 100 * K + n + 1000 * seed)


@functools.lru_cache(maxsize=None)
def stream_key(seed):
    return np.random.RandomState(seed).get_state()[1].copy()


def avail_words(avail):
    w = np.zeros(4, dtype=np.uint64)
    for c in avail:
        w[c >> 5] |= np.uint64(1) << np.uint64(c & 31)
    return w.astype(np.uint32)


def launch(K, decisions, mc_per_card, mc_max, stats=True):
    """sn_mcs_decide_exact on decisions = [(board, hand, avail, key, pos)]:
    (actions [D], sums [D,10] | None, counts | None, keys [D,624], pos [D])"""
    from rl_6_nimmt import _native as nat

    D = len(decisions)
    board = np.full((D, 4, 6), -1, dtype=np.int8)
    hand = np.full((D, 10), -1, dtype=np.int8)
    words = np.zeros((D, 4), dtype=np.uint32)
    keys = np.zeros((D, 624), dtype=np.uint32)
    pos = np.zeros(D, dtype=np.int32)
    for d, (b, h, av, key, p) in enumerate(decisions):
        for r, row in enumerate(b):
            board[d, r, : len(row)] = row
        hand[d, : len(h)] = sorted(h)
        words[d] = avail_words(av)
        keys[d], pos[d] = key, p
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(a).to(dev)
    d_board, d_hand = up(board), up(hand)
    d_avail, d_keys, d_pos = up(words.view(np.int32)), up(keys.view(np.int32)), up(pos)
    d_act = torch.full((D,), FILL, dtype=torch.int32, device=dev)
    d_sums = torch.full((D, 10), FILL, dtype=torch.int32, device=dev) if stats else None
    d_cnts = torch.full((D, 10), FILL, dtype=torch.int32, device=dev) if stats else None
    nat.check(nat.lib().sn_mcs_decide_exact(dev.index, D, K, nat.ptr(d_board), nat.ptr(d_hand), nat.ptr(d_avail),
                                            mc_per_card, mc_max, nat.ptr(d_keys), nat.ptr(d_pos), nat.ptr(d_act),
                                            nat.ptr(d_sums), nat.ptr(d_cnts), nat.stream_handle(dev)),
              "sn_mcs_decide_exact")
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(d_act), host(d_sums), host(d_cnts), host(d_keys).view(np.uint32), host(d_pos)


def oracle(K, decisions, mc_per_card, mc_max):
    return [O.mcs_decide(b, h, av, K, mc_per_card, mc_max, key, p) for b, h, av, key, p in decisions]


def assert_same(got, refs, what):
    act, sums, cnts, keys, pos = got
    for d, (card, q6, rs, rc, rkey, rpos) in enumerate(refs):
        assert act[d] == (-card - 2 if q6 else card), (what, d, "action")
        if sums is not None:
            assert np.array_equal(sums[d], rs), (what, d, "sums")
            assert np.array_equal(cnts[d], rc), (what, d, "counts")
        assert pos[d] == rpos, (what, d, "pos")
        assert np.array_equal(keys[d], rkey), (what, d, "key")


def test_every_stream_phase():
    """One launch of D = 625: the same 4-player decision from every start pos
    of one key.  The final positions must reach both ends of a round, so both
    exports run: handing back the previous round's key to a consumer that has
    not left it (the straddle) and finishing the current round in place.
    Also: D > 1, and a decision does not depend on its index."""
    board, hand, avail = position(4, 10)
    key = stream_key(2026)  # a key for which the condition below holds (checked on the oracle)
    decisions = [(board, hand, avail, key, p) for p in range(625)]
    refs = oracle(4, decisions, 10, 100)
    ends = np.array([r[5] for r in refs])
    assert ((ends >= 561) & (ends <= 624)).any() and ((ends >= 0) & (ends <= 63)).any()
    got = launch(4, decisions, 10, 100)
    assert_same(got, refs, "phase")


# (mc_per_card, mc_max): playouts as 64 + 36, one full batch, 64 + 1, n! at
# small n, three full batches + 8, a budget small enough for Q6, none at all
BUDGETS = [(10, 100), (10, 64), (10, 65), (1, 1000), (10, 200), (10, 30), (0, 50)]
START_POS = [0, 600, 623, 624, 1, 63, 64, 311, 560, 561]


@pytest.mark.parametrize("K", range(2, 11))
def test_every_player_count_and_hand_size(K):
    """K players, every hand size n = 2..10 under every budget shape, one
    launch per budget.  At n = 10 the memory is fresh (A = 90): a playout
    takes 89 + 9 K draws, more than 160 from K = 8 on.  One of the K = 2
    decisions stops on the last word of a round: numpy's state is then that
    round's key at pos 624, not the next round's at pos 0."""
    q6_seen, ends = set(), set()
    for bi, (mpc, mmax) in enumerate(BUDGETS):
        decisions = []
        for n in range(2, 11):
            board, hand, avail = position(K, n)
            assert len(hand) == n and len(avail) >= (K - 1) * n
            i = bi * 9 + n
            decisions.append((board, hand, avail, stream_key(7000 + 97 * K + i), START_POS[i % len(START_POS)]))
        assert len(decisions[-1][2]) == 90
        refs = oracle(K, decisions, mpc, mmax)
        for n, r in zip(range(2, 11), refs):
            n_mc = min(mmax, mpc * int(np.prod(np.arange(1, n + 1))))
            assert r[0] >= 0 and int(r[3].sum()) == n_mc
            q6_seen.add(r[1])
            ends.add(r[5])
        assert_same(launch(K, decisions, mpc, mmax), refs, (K, mpc, mmax))
    assert q6_seen == {False, True}
    assert K != 2 or 624 in ends


def test_edges():
    """A one-card hand, decisions that break the preconditions, and NULL
    sums / counts, next to ordinary decisions in the same launch."""
    K = 4
    key = stream_key(31)
    board5, hand5, avail5 = position(K, 5)
    board1, hand1, avail1 = position(K, 1)
    assert len(hand1) == 1 and len(avail5) > 15
    decisions = [
        (board5, hand5, avail5, key, 600),
        (board1, hand1, avail1, key, 77),         # n == 1
        (board5, hand5, avail5[:14], key, 600),   # A = 14 < (K - 1) n = 15
        (board5, hand5, avail5[:15], key, 600),   # A = 15: just enough
        (board5, hand5, [], key, 623),            # A = 0
        (board5, hand5, list(range(128)), key, 5),  # more cards than a deck holds
        (board5, hand5, avail5, key, 600),
    ]
    refs = oracle(K, decisions, 10, 100)
    assert [r[0] for r in refs[1:6]] == [hand1[0], -1, refs[3][0], -1, -1] and refs[3][0] in hand5
    got = launch(K, decisions, 10, 100)
    assert_same(got, refs, "edges")
    act, sums, cnts, keys, pos = got
    for d in (1, 2, 4, 5):  # no search: zeroed statistics, the stream bit-unchanged
        assert not sums[d].any() and not cnts[d].any()
        assert np.array_equal(keys[d], key) and pos[d] == decisions[d][4]
    assert act[1] == hand1[0] and act[2] == act[4] == act[5] == -1
    # the neighbours of the refused decisions are the same ordinary decision
    assert act[0] == act[6] and np.array_equal(sums[0], sums[6]) and np.array_equal(keys[0], keys[6])
    assert_same(launch(K, decisions, 10, 100, stats=False), refs, "edges, NULL sums/counts")


@pytest.mark.parametrize("seats,seed", [(8, 5), (10, 6)])
def test_dropin_above_four_seats(seats, seed):
    """GameSession(MCSAgent, DrunkHamster x (seats - 1)), seeded: the moves
    and the results of the oracle's reference-exact game."""
    from rl_6_nimmt import GameSession
    from rl_6_nimmt.agents import DrunkHamster, MCSAgent

    rc, ref_moves, ref_rewards = O.mcs_game("M" + "R" * (seats - 1), 10, 100, seed)
    assert rc == 0
    np.random.seed(seed)
    sess = GameSession(MCSAgent(mc_per_card=10, mc_max=100), *[DrunkHamster() for _ in range(seats - 1)])
    moves, step = [], sess.env.step

    def recording_step(actions):
        moves.append([int(a) for a in actions])
        return step(actions)

    sess.env.step = recording_step
    sess.play_game()
    assert moves == ref_moves.tolist()
    assert sess.results[0].tolist() == ref_rewards.sum(axis=0).tolist()
