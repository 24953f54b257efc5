"""GPU checks of mixed leagues on Philox streams (sn_league_step on a Philox
tournament handle, k_league_mcs_philox, sn_mcs_decide_philox).

The reference is tests/league_philox_model.py, the stream law of
include/sechs.h written over the oracle: the search kernel is compared with it
per decision through the hook, whole league rounds record for record, reward
for reward and counter for counter -- equality is exact throughout.  The last
test holds the Philox league's MCSAgent to the numpy league's (the
reference-exact search, pinned by golden F11) in law: the mean margin over a
DrunkHamster of the two must agree within their standard errors.
"""
import functools
import math

import numpy as np
import pytest
import torch

import league_philox_model as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5  # what the output buffers hold before a launch

# roster (b): a league's player count is at most its agent count (tournament.py:170), so players 2..6 seat six agents
KINDS_B = "RRRMMR"
MPC_B, MMAX_B = [10, 10, 10, 2, 1, 10], [100, 100, 100, 12, 70, 100]


def _league(B, kinds, lo, hi, seed, game_offset=0, rng="philox", fused=False, mpc=None, mmax=None):
    from rl_6_nimmt.agents import DrunkHamster, MCSAgent
    from rl_6_nimmt.league import BatchedTournament

    t = BatchedTournament(B, lo, hi, seed=seed, game_offset=game_offset, rng=rng, fused=fused)
    for i, c in enumerate(kinds):
        t.add_player(f"a{i}", MCSAgent(mc_per_card=mpc[i], mc_max=mmax[i]) if c == "M" else DrunkHamster())
    return t


# ---------------------------------------------------------------- 1. the search kernel through the hook
@functools.lru_cache(maxsize=None)
def position(K, n, dealt):
    """(board, hand, memory).  dealt: the position as dealt (one card a row, a memory of 90 cards) with the hand
    cut to its n lowest cards; else a position n cards into an oracle game (rows of several cards)"""
    if dealt:
        board, hand, avail = O.mcs_position(K, 10, 500 + K)
        assert len(avail) == 90
        return board, sorted(hand)[:n], avail
    return O.mcs_position(K, n, 100 * K + n)


def avail_words(avail):
    w = np.zeros(4, dtype=np.uint64)
    for c in avail:
        w[c >> 5] |= np.uint64(1) << np.uint64(c & 31)
    return w.astype(np.uint32)


def launch(K, decisions, mc_per_card, mc_max):
    """sn_mcs_decide_philox on decisions = [(board, hand, avail, key, stream0)]: (actions [D], sums, counts [D, 10])"""
    from rl_6_nimmt import _native as nat

    D = len(decisions)
    board = np.full((D, 4, 6), -1, dtype=np.int8)
    hand = np.full((D, 10), -1, dtype=np.int8)
    words = np.zeros((D, 4), dtype=np.uint32)
    keys = np.zeros((D, 2), dtype=np.uint32)
    streams = np.zeros(D, dtype=np.uint64)
    for d, (b, h, av, key, s0) in enumerate(decisions):
        for r, row in enumerate(b):
            board[d, r, : len(row)] = row
        hand[d, : len(h)] = sorted(h)
        words[d] = avail_words(av)
        keys[d], streams[d] = (key & M.M32, key >> 32), s0
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(a).to(dev)
    d_board, d_hand, d_avail = up(board), up(hand), up(words.view(np.int32))
    d_keys, d_streams = up(keys.view(np.int32)), up(streams.view(np.int64))
    d_act = torch.full((D,), FILL, dtype=torch.int32, device=dev)
    d_sums = torch.full((D, 10), FILL, dtype=torch.int32, device=dev)
    d_cnts = torch.full((D, 10), FILL, dtype=torch.int32, device=dev)
    nat.check(nat.lib().sn_mcs_decide_philox(dev.index, D, K, nat.ptr(d_board), nat.ptr(d_hand), nat.ptr(d_avail),
                                             mc_per_card, mc_max, nat.ptr(d_keys), nat.ptr(d_streams), nat.ptr(d_act),
                                             nat.ptr(d_sums), nat.ptr(d_cnts), nat.stream_handle(dev)),
              "sn_mcs_decide_philox")
    torch.cuda.synchronize()
    return d_act.cpu().numpy(), d_sums.cpu().numpy(), d_cnts.cpu().numpy()


def assert_same(got, decisions, K, mc_per_card, mc_max, what):
    act, sums, cnts = got
    refs = [M.search(b, h, av, K, mc_per_card, mc_max, key, s0) for b, h, av, key, s0 in decisions]
    for d, (card, q6, rs, rc) in enumerate(refs):
        assert act[d] == (-card - 2 if q6 else card), (what, d, "action")
        assert np.array_equal(sums[d], rs), (what, d, "sums")
        assert np.array_equal(cnts[d], rc), (what, d, "counts")
    return refs


# per hand size n, (mc_per_card, mc_max) -> n_mc: 1 (quirk Q6 is certain); 20 and 60, bound by mc_per_card * n!
# where an n! reaches them (2 * 10, 2 * 30, 6 * 10), else by mc_max; 64 and 65, the lane-round edge; 130, three
# lane rounds
BUDGETS = {
    2: [((1, 1), 1), ((10, 1000), 20), ((30, 1000), 60), ((32, 1000), 64), ((100, 65), 65), ((65, 1000), 130)],
    3: [((1, 1), 1), ((100, 20), 20), ((10, 1000), 60), ((100, 64), 64), ((100, 65), 65), ((100, 130), 130)],
    10: [((1, 1), 1), ((1, 20), 20), ((1, 60), 60), ((1, 64), 64), ((1, 65), 65), ((1, 130), 130)],
}


@pytest.mark.parametrize("K", [2, 6])
def test_search_kernel_equals_the_model_per_decision(K):
    """K in {2, 6} x n in {2, 3, 10} x a memory of (K - 1) n (the least that deals) and of 90 cards x n_mc in
    {1, 20, 60, 64, 65, 130}: actions (the Q6 encoding included), sums and counts, exactly"""
    by_budget = {}
    for n, budgets in BUDGETS.items():
        for (mpc, mmax), n_mc in budgets:
            assert M.num_playouts(n, mpc, mmax) == n_mc
            for dealt in (False, True):
                board, hand, avail = position(K, n, dealt)
                assert len(hand) == n
                av = list(avail) if dealt else sorted(avail)[: (K - 1) * n]
                assert len(av) == (90 if dealt else (K - 1) * n)
                i = len(by_budget.setdefault((mpc, mmax), []))
                key, s0 = M.mcs_key(0xC0FFEE_0000_0000 + 977 * K + n, 1000 * n_mc + i), M.mcs_stream(40 + i, i % K, n)
                by_budget[(mpc, mmax)].append((board, hand, av, key, s0))
    q6_seen, n_cases = set(), 0
    for (mpc, mmax), decisions in by_budget.items():
        refs = assert_same(launch(K, decisions, mpc, mmax), decisions, K, mpc, mmax, (K, mpc, mmax))
        for (b, h, av, key, s0), r in zip(decisions, refs):
            assert r[0] >= 0 and int(r[3].sum()) == M.num_playouts(len(h), mpc, mmax)
            q6_seen.add(r[1])
            if mmax == 1:
                assert r[1]  # one playout, n >= 2 legal moves
        n_cases += len(decisions)
    assert n_cases == 3 * 6 * 2 and q6_seen == {False, True}


def test_search_kernel_refuses_a_memory_one_card_short():
    """(K - 1) n - 1 cards cannot deal the opponents: -1, zeroed sums and counts, the neighbours untouched"""
    K, n = 4, 5
    board, hand, avail = position(K, n, False)
    avail = sorted(avail)
    assert len(avail) > (K - 1) * n
    key, s0 = M.mcs_key(99, 7), M.mcs_stream(3, 1, n)
    decisions = [(board, hand, avail, key, s0), (board, hand, avail[: (K - 1) * n - 1], key, s0),
                 (board, hand, avail, key, s0), (board, hand, avail[: (K - 1) * n], key, s0)]
    got = launch(K, decisions, 10, 100)
    refs = assert_same(got, decisions, K, 10, 100, "short")
    act, sums, cnts = got
    assert act[1] == -1 and refs[1][0] == -1 and not sums[1].any() and not cnts[1].any()
    assert act[0] == act[2] and act[0] != FILL and np.array_equal(sums[0], sums[2]) and np.array_equal(cnts[0], cnts[2])
    assert int(cnts[0].sum()) == 100 and int(cnts[3].sum()) == 100


# ---------------------------------------------------------------- 2. league steps against the model
def _assert_league_equals_model(t, out, games):
    rec, rew = t.play_games(games, rewards=True)
    assert t.mode == "step"
    assert np.array_equal(rec.cpu().numpy(), out["records"])
    assert np.array_equal(rew.cpu().numpy(), out["rewards"])
    assert [t.env.philox_counter(g) for g in range(t.num_slots)] == [int(c) for c in out["ctr"]]
    assert t.q6_slot_rounds == out["q6"]
    return rec


def test_all_hamster_league_steps_equal_the_model_and_the_fused_rollout():
    """(a) five DrunkHamsters, players 2..4, 10 slots, 2 games, game_offset 5: the stepped league against the
    model -- records, per-step rewards, counters, no Q6 -- and the fused rollout's records the same"""
    kw = dict(lo=2, hi=4, seed=0xFEED_0000_0001, game_offset=5)
    out = M.league("RRRRR", 2, 4, seed=kw["seed"], game_offset=5, slots=10, games=2)
    t = _league(10, "RRRRR", fused=False, **kw)
    rec = _assert_league_equals_model(t, out, 2)
    f = _league(10, "RRRRR", fused=True, **kw)
    rec_f = f.play_games(2)
    assert f.mode == "fused" and torch.equal(rec, rec_f)
    t.close(), f.close()


def test_mixed_league_steps_equal_the_model():
    """(b) DrunkHamsters + MCSAgent(2, 12) + MCSAgent(1, 70), players 2..6, 10 slots, 2 games, game_offset 5"""
    seed = 0xFEED_0000_0002
    out = M.league(KINDS_B, 2, 6, MPC_B, MMAX_B, seed=seed, game_offset=5, slots=10, games=2)
    assert out["q6"] > 0 and len(out["streams"]) > 1000  # 12 playouts over up to 10 moves: Q6 occurs
    assert set(np.unique(out["records"][..., 0] & 15)) >= {2, 6}
    t = _league(10, KINDS_B, 2, 6, seed, game_offset=5, mpc=MPC_B, mmax=MMAX_B)
    _assert_league_equals_model(t, out, 2)
    t.close()


# ---------------------------------------------------------------- 3. sharding
def test_mixed_league_is_independent_of_the_sharding():
    """roster (b) at 64 slots = two 32-slot leagues at game_offset 0 and 32, record for record"""
    seed, G = 0xFEED_0000_0003, 2
    whole = _league(64, KINDS_B, 2, 6, seed, game_offset=0, mpc=MPC_B, mmax=MMAX_B)
    rec = whole.play_games(G)
    for off in (0, 32):
        part = _league(32, KINDS_B, 2, 6, seed, game_offset=off, mpc=MPC_B, mmax=MMAX_B)
        assert torch.equal(part.play_games(G), rec[:, off: off + 32]), off
        part.close()
    whole.close()


# ---------------------------------------------------------------- 4. a whole mixed league
def _net_league(slots=96):
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.league import BatchedTournament

    torch.manual_seed(11)
    t = BatchedTournament(slots, 2, 4, seed=3, game_offset=40, rng="philox", fused=False, train=True)
    t.add_player("h")
    t.add_player("m", A.MCSAgent(mc_max=20))
    t.add_player("p", A.PUCTAgent(mc_max=4))
    q = A.DDQN_PRBAgent(history_length=64, minibatch=16)
    q.eps = 0.3
    t.add_player("q", q)
    return t


def test_whole_mixed_league_trains_saves_and_resumes(tmp_path):
    """DrunkHamster, MCS, PUCT and DDQN_PRB seats on Philox, training, 96 slots: 2 rounds (an illegal move of an
    engine would raise), well-formed records, then save / load and one more round, equal to the uninterrupted
    league's bit for bit; the saved handle is the Philox + league snapshot"""
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.league import BatchedTournament, decode_seats, relative_positions

    ref = _net_league()
    ref.play_games(2)
    last = ref.play_games(1)
    t = _net_league()
    rec = t.play_games(2)
    assert t.mode == "step" and t.rng == "philox"
    assert torch.equal(rec, torch.cat([r for r, _ in ref.records])[:2])
    k, ids = decode_seats(rec[..., 0], 4)
    res = rec[..., 1:]
    assert int(k.min()) >= 2 and int(k.max()) <= 4 and int(res.max()) <= 0 and not res[ids < 0].any()
    assert torch.allclose(relative_positions(res, k).sum(-1), k.double() / 2)
    assert all(s > 0 for s in t.agent_stats()[:, 0])
    path = str(tmp_path / "league.pt")
    t.save(path)
    blob = t.state_dict()["env"]["blob"]
    assert blob.numel() == nat.lib().sn_state_bytes(96, 4, nat.SN_RNG_PHILOX, 1, None, None)
    assert blob.numel() < 96 * 200 + 4096  # under 200 B a slot (numpy: 2 496 B of MT19937 state alone)
    u = BatchedTournament.load(path)
    assert u is not t and u.rng == "philox" and u.mode == "step"
    assert torch.equal(u.play_games(1), last)
    assert u.q6_slot_rounds == ref.q6_slot_rounds and u.total_games == ref.total_games
    for x in (ref, t, u):
        x.close()


# ---------------------------------------------------------------- 5. a mid-round snapshot
def _steps(t, n, reset):
    from rl_6_nimmt import _native as nat

    env, L = t.env, nat.lib()
    slots, N, dev = t.num_slots, t.max_players, env.device
    if reset:
        nat.check(L.sn_reset(env._h, None, env._stream()), "sn_reset")
    acts = torch.zeros((slots, N), dtype=torch.int32, device=dev)
    rew = torch.zeros((n, slots, N), dtype=torch.int32, device=dev)
    played = torch.zeros((n, slots, N), dtype=torch.int32, device=dev)
    rec = torch.zeros((slots, 1 + N), dtype=torch.int32, device=dev)
    invalid = torch.zeros((slots,), dtype=torch.int32, device=dev)
    status = torch.zeros((slots,), dtype=torch.int32, device=dev)
    for i in range(n):
        nat.check(L.sn_league_step(env._h, nat.ptr(acts), nat.ptr(rew[i]), nat.ptr(played[i]), nat.ptr(rec),
                                   nat.ptr(invalid), nat.ptr(status), env._stream()), "sn_league_step")
    return rew.cpu(), played.cpu(), rec.cpu(), status.cpu()


def test_philox_tournament_handle_resumes_mid_round():
    """two MCS seats, saved 4 steps into a round and loaded into a freshly configured twin: the twin finishes the
    round as the original does (the searches are keyed by the slot's counter, the seat and the hand size: no
    state of their own), and plays the next round the same"""
    def make():
        t = _league(130, "MRMR", 2, 4, seed=6, game_offset=20, mpc=[10, 10, 2, 10], mmax=[20, 100, 20, 100])
        t._start()
        return t

    a, b = make(), make()
    _steps(a, 4, reset=True)
    sd = a.env.state_dict()
    b.env.load_state_dict(sd)
    ra, rb = _steps(a, 6, reset=False), _steps(b, 6, reset=False)
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)
    assert bool((ra[2][:, 0] != 0).all())  # every slot's game ended and left its record
    assert torch.equal(a.env.state_dict()["blob"], b.env.state_dict()["blob"])
    ra, rb = _steps(a, 10, reset=True), _steps(b, 10, reset=True)
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)
    a.close(), b.close()


# ---------------------------------------------------------------- 6. the same agent in law
def _mcs_margin(rng):
    """d = the MCS agent's result minus its opponent's, over the two-player games that seat it: (mean, standard error)"""
    from rl_6_nimmt.league import decode_seats

    t = _league(4096, "MRR", 2, 2, seed=0xFEED_0000_0006, rng=rng, mpc=[10, 10, 10], mmax=[100, 100, 100])
    rec = t.play_games(1)[0]
    t.close()
    k, ids = decode_seats(rec[:, 0], 2)
    res = rec[:, 1:].double()
    seat = (ids == 0).double()  # [slots, 2]: where agent 0, the MCSAgent, sits
    has = seat.sum(-1) > 0
    d = ((res * seat).sum(-1) - (res * (1 - seat)).sum(-1))[has].cpu().numpy()
    assert len(d) > 2000  # the agent sits in two games of three
    return float(d.mean()), float(d.std(ddof=1) / math.sqrt(len(d)))


def test_philox_mcs_agent_is_the_numpy_one_in_law():
    """MCSAgent(10, 100) against a DrunkHamster, 4 096 two-player games per rng mode: the two mean margins agree
    within 4 combined standard errors, and each exceeds zero by 4 of its own -- the search searches"""
    (m_np, se_np), (m_ph, se_ph) = _mcs_margin("numpy"), _mcs_margin("philox")
    print(f"MCS margin over a DrunkHamster: numpy {m_np:.3f} +- {se_np:.3f}, philox {m_ph:.3f} +- {se_ph:.3f}")
    assert abs(m_np - m_ph) <= 4.0 * math.hypot(se_np, se_ph)
    assert m_np > 4.0 * se_np and m_ph > 4.0 * se_ph
