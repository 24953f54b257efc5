"""Every Philox draw of the decision kernels against a host model, decision by decision.

The epsilon-greedy draws (sn_dqn_select, sn_dqn_select_duel), the policy sample (sn_policy_sample), a rollout's
deal (sn_puct_deal, sn_puct_deal_batch) and its moves (sn_puct_step) all draw from the stream layout of
csrc/sechs_decide.h.  The law tests elsewhere check frequencies and repeatability, which a kernel that dropped the
seat, the game offset, a key word or the step from its stream would still pass.  Here the words are predicted on
the host (rl_6_nimmt/engine.py: decision_words_host) and what each kernel does with them is restated in
tests/decision_models.py: the select and deal models are exact, the sampling models follow the band rule
described there.  Logits, Q values and heads are written by the tests (decision_models.py builds them, so that
test_decision_models_cpu.py can bound the ambiguous share of the very same arrays without a device).

Each sampling test prints `compared / in the band / of those differing from the float64 model` (pytest -s).
"""
import ctypes

import numpy as np
import pytest
import torch

import decision_models as M

pytestmark = pytest.mark.gpu

B, N, MASK = M.B, M.N, M.MASK


# ---------------------------------------------------------------- handles and launches
def _handle(games=B, seats=N, mask=MASK, game_offset=0):
    """an env handle after reset and a bare BatchedEngine on it (the deciding seats, seed and counter of
    _params; no net)"""
    from rl_6_nimmt.engine import BatchedEngine
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(games, seats, seed=3, game_offset=game_offset, rng="philox")
    env.reset()
    return env, BatchedEngine(env, None, seed=M.SEED, seats_mask=mask)


@pytest.fixture(scope="module")
def handle():
    env, eng = _handle()
    yield env, eng
    env.close()


def _params(eng, n, seed, step):
    eng.seed, eng.step_id = seed, step
    return eng._params(n)


def _deciders(env, eng):
    """(flat g * N + p [D], global game id [D], seat [D], hands [D, 10] int64) in decision order"""
    flat = eng.decider_index().cpu().numpy().astype(np.int64)
    g, p = np.divmod(flat, env.num_players)
    gid = (np.uint64(env.game_offset) + g.astype(np.uint64))
    return flat, gid, p, env.hands().cpu().numpy().astype(np.int64).reshape(-1, 10)[flat]


def _outputs(env, D):
    dev = env.device
    return (torch.full((env.num_games, env.num_players), -7, dtype=torch.int32, device=dev),
            torch.full((D,), -7, dtype=torch.int32, device=dev), torch.full((D,), -7.0, dtype=torch.float32, device=dev))


def _check_actions(env, eng, actions, index, flat, hands, what):
    """the deciding seats play the card at `index` of their hand, the other seats' words are not written"""
    a = actions.cpu().numpy().reshape(-1)
    assert np.array_equal(a[flat], hands[np.arange(flat.size), index]), what
    others = np.ones(a.size, dtype=bool)
    others[flat] = False
    assert (a[others] == -7).all(), what


# the Q side of a select: distinct integers per row, so the greedy index is the arg-max of the table over the hand
# in any rounding, and no Q equals the -1 an explored decision reports as its value
def _q_table(D, key):
    rng = np.random.default_rng([7, key])
    return np.stack([rng.permutation(104) for _ in range(D)]).astype(np.float32)


SELECT_KINDS = ("q", "duel_vec", "duel_scalar")


def _select(env, q, D, table, eps, kind):
    """one select launch over the Q table in the kernel's input form: sn_dqn_select on Q = table + 0.5 in a
    padded row (stride 112, the pad would win if it were read); sn_dqn_select_duel on A = table, V = 1000.5,
    16-byte aligned rows (stride 108, A first: the float4 kernel) or stride 105 with V first (scalar loads)"""
    from rl_6_nimmt import _native as nat

    dev, L = env.device, nat.lib()
    actions, index, value = _outputs(env, D)
    t = torch.from_numpy(table).to(dev)
    if kind == "q":
        buf = torch.full((D, 112), 1e9, device=dev)
        buf[:, :104] = t + 0.5
        nat.check(L.sn_dqn_select(env._h, ctypes.byref(q), nat.ptr(buf), 112, float(eps), nat.ptr(actions),
                                  nat.ptr(index), nat.ptr(value), env._stream()), "sn_dqn_select")
    else:
        stride, v_col, a_off = (108, 104, 0) if kind == "duel_vec" else (105, 0, 1)
        buf = torch.full((D, stride), 1e9, device=dev)
        buf[:, a_off:a_off + 104], buf[:, v_col] = t, 1000.5
        assert (buf.data_ptr() + 4 * a_off) % 16 == (0 if kind == "duel_vec" else 4)
        nat.check(L.sn_dqn_select_duel(env._h, ctypes.byref(q), nat.ptr(buf), stride, v_col, a_off, float(eps),
                                       nat.ptr(actions), nat.ptr(index), nat.ptr(value), env._stream()),
                  "sn_dqn_select_duel")
    torch.cuda.synchronize()
    return actions, index.cpu().numpy().astype(np.int64), value.cpu().numpy()


def _check_select(env, eng, n, seed, step, eps, kind, table, what):
    """index, actions and the value == -1 mask of one select launch against select_model, exactly"""
    flat, gid, seat, hands = _deciders(env, eng)
    D = flat.size
    actions, index, value = _select(env, _params(eng, n, seed, step), D, table, eps, kind)
    explore, explored = M.select_model(M.select_words(seed, step, gid, seat), eps, n)
    greedy = table[np.arange(D)[:, None], hands[:, :n]].argmax(axis=1)
    want = np.where(explore, explored, greedy)
    bad = np.nonzero(index != want)[0]
    assert bad.size == 0, (what, "decisions", bad[:8], "got", index[bad[:8]], "model", want[bad[:8]], explore[bad[:8]])
    assert np.array_equal(value == -1.0, explore), what
    _check_actions(env, eng, actions, index, flat, hands, what)
    return explore


def _sample(env, q, D, logits):
    from rl_6_nimmt import _native as nat

    actions, index, _ = _outputs(env, D)
    lg = torch.from_numpy(np.ascontiguousarray(logits)).to(env.device).reshape(-1).contiguous()
    assert lg.dtype == torch.float32 and lg.numel() == D * q.n
    nat.check(nat.lib().sn_policy_sample(env._h, ctypes.byref(q), nat.ptr(lg), nat.ptr(actions), nat.ptr(index), None,
                                         None, env._stream()), "sn_policy_sample")
    torch.cuda.synchronize()
    return actions, index.cpu().numpy().astype(np.int64)


# ---------------------------------------------------------------- the epsilon-greedy draws
@pytest.mark.parametrize("eps", [0.3, 1.0])
@pytest.mark.parametrize("n", [10, 7, 1])
@pytest.mark.parametrize("kind", SELECT_KINDS)
def test_select_draws_equal_the_model(handle, kind, n, eps):
    env, eng = handle
    table = _q_table(B * 2, SELECT_KINDS.index(kind))
    explored = 0
    for step in range(M.SELECT_STEPS):
        explored += int(_check_select(env, eng, n, M.SEED, step, eps, kind, table, (kind, n, eps, step)).sum())
    total = M.SELECT_STEPS * B * 2
    assert explored == total if eps == 1.0 else 0.2 * total < explored < 0.4 * total  # both branches were compared


# ---------------------------------------------------------------- the policy sample
@pytest.mark.parametrize("scale", M.SCALES)
@pytest.mark.parametrize("n", [10, 7, 2, 1])
def test_policy_sample_draws_equal_the_model(handle, n, scale):
    env, eng = handle
    flat, gid, seat, hands = _deciders(env, eng)
    logits, u = M.sample_case(n, scale)
    got = []
    for step in range(M.SAMPLE_STEPS):
        actions, index = _sample(env, _params(eng, n, M.SEED, step), flat.size, logits[step])
        assert index.min() >= 0 and index.max() < n
        _check_actions(env, eng, actions, index, flat, hands, (n, scale, step))
        got.append(index)
    M.check_sample(np.stack(got), logits, u, f"sn_policy_sample n={n} scale={scale}")


# ---------------------------------------------------------------- the key and the stream's fields
@pytest.mark.parametrize("case", range(len(M.KEY_CASES)))
def test_key_and_stream_fields_reach_the_draws(case):
    """both seed words, the decision counter and game_offset + g (its low 32 bits: the third and fourth cases
    wrap inside the handle) as the select and the sample kernels key their draws"""
    seed, step, offset = M.KEY_CASES[case]
    env, eng = _handle(games=M.KEY_GAMES, game_offset=offset)
    flat, gid, seat, hands = _deciders(env, eng)
    want_gid, want_seat, logits, u = M.key_case(case)
    assert np.array_equal(gid, want_gid) and np.array_equal(seat, want_seat)
    if offset == 2**32 - 3:
        assert int((gid >> np.uint64(32)).max()) == 1 and int((gid >> np.uint64(32)).min()) == 0
    table = _q_table(flat.size, 10 + case)
    for eps in (0.3, 1.0):
        _check_select(env, eng, 10, seed, step, eps, "q", table, (case, eps))
    actions, index = _sample(env, _params(eng, 10, seed, step), flat.size, logits)
    _check_actions(env, eng, actions, index, flat, hands, case)
    M.check_sample(index, logits, u, f"key fields {case}")
    env.close()


def test_a_second_handle_continues_the_first_ones_games():
    """8 games at game_offset 8 draw what games 8..15 of a 16-game handle at offset 0 draw: a shard of a league
    explores as its games would in one handle, not as the first shard does"""
    whole, w_eng = _handle(games=16)
    part, p_eng = _handle(games=8, game_offset=8)
    gid, seat, logits, u = M.offset_case()
    table = _q_table(gid.size, 20)
    lo = 8 * 2  # the first decision of game 8
    res = {}
    for name, env, eng, rows in (("whole", whole, w_eng, slice(None)), ("part", part, p_eng, slice(lo, None))):
        flat, g_, s_, hands = _deciders(env, eng)
        assert np.array_equal(g_, gid[rows]) and np.array_equal(s_, seat[rows])
        sel = []
        for eps in (0.3, 1.0):
            q = _params(eng, 10, M.SEED, 7)
            _, index, value = _select(env, q, flat.size, table[rows], eps, "q")
            explore, explored = M.select_model(M.select_words(M.SEED, 7, g_, s_), eps, 10)
            assert np.array_equal(value == -1.0, explore) and np.array_equal(index[explore], explored[explore]), name
            sel.append((np.where(explore, index, -1), explore))
        _, index = _sample(env, _params(eng, 10, M.SEED, 7), flat.size, logits[rows])
        M.check_sample(index, logits[rows], u[rows], f"game offset ({name})")
        res[name] = (sel, index)
    for (wi, we), (pi, pe) in zip(res["whole"][0], res["part"][0]):
        assert np.array_equal(wi[lo:], pi) and np.array_equal(we[lo:], pe)
    assert np.array_equal(res["whole"][1][lo:], res["part"][1])
    assert not np.array_equal(res["whole"][1][:lo], res["part"][1])  # the first shard's draws are others
    whole.close()
    part.close()


# ---------------------------------------------------------------- the decision-list form
def test_decision_list_draws_equal_the_model():
    """a tournament handle: the agent's seats come as a decision list, (g, p) = divmod(dec, N), on games of 2,
    3 and 4 players"""
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.agents import DQNVanilla
    from test_gpu_dqn_batched import _league

    t = _league(DQNVanilla(history_length=1000), train=False, slots=M.LIST_SLOTS)
    t.play_games(1)
    env, eng = t.env, t.engines["Q"]
    nat.check(nat.lib().sn_reset(env._h, None, env._stream()), "sn_reset")  # a fresh seat draw + deal
    t._use_decisions()
    D = eng.D
    dec = eng.dec.cpu().numpy().astype(np.int64)
    flat, gid, seat, hands = _deciders(env, eng)
    assert D > 64 and np.array_equal(flat, dec) and env.num_players == N and env.num_games == M.LIST_SLOTS
    k, _ = t.seats()
    players = k.cpu().numpy()[dec // N]
    assert sorted(set(players.tolist())) == [2, 3, 4] and (seat < players).all()
    assert len(set(seat.tolist())) == N  # the agent sits at every seat somewhere
    q = _params(eng, 10, M.SEED, M.LIST_STEP)
    assert q.num_dec == D and q.dec_list == eng.dec.data_ptr()
    actions, index, value = _select(env, q, D, _q_table(D, 30), 1.0, "q")
    explore, explored = M.select_model(M.select_words(M.SEED, M.LIST_STEP, gid, seat), 1.0, 10)
    assert explore.all() and np.array_equal(index, explored) and (value == -1.0).all()
    _check_actions(env, eng, actions, index, flat, hands, "select")
    _, _, logits, u = M.list_case()
    actions, index = _sample(env, q, D, logits[dec])
    _check_actions(env, eng, actions, index, flat, hands, "sample")
    M.check_sample(index, logits[dec], u[dec], "decision list")
    t.close()


# ---------------------------------------------------------------- the engines' plumbing
def test_reinforce_engine_hands_its_seed_and_counter_to_the_sample():
    """three consecutive BatchedReinforce.decide calls draw at eng.seed and step_id, step_id + 1, step_id + 2
    (here across the 32-bit wrap of the counter); the net's logits are replaced by the test's"""
    from rl_6_nimmt.puct import make_actor
    from rl_6_nimmt.reinforce import BatchedReinforce
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(B, N, seed=3, rng="philox")
    env.reset()
    eng = BatchedReinforce(env, make_actor(), seats_mask=MASK, net_dtype=torch.float32, seed=M.ENGINE_SEED)
    eng.step_id = M.ENGINE_STEP0
    flat, gid, seat, hands = _deciders(env, eng)
    logits, u = M.engine_case()
    handed = iter(torch.from_numpy(logits).to(env.device))
    eng._logits = lambda rows: next(handed).reshape(-1).contiguous()
    got = []
    for i in range(M.ENGINE_CALLS):
        eng.actions.fill_(-7)
        actions = eng.decide(10)
        torch.cuda.synchronize()
        index = eng.best_index[: eng.D].cpu().numpy().astype(np.int64)
        _check_actions(env, eng, actions, index, flat, hands, i)
        got.append(index)
    assert eng.step_id == M.ENGINE_STEP0 + M.ENGINE_CALLS
    M.check_sample(np.stack(got), logits, u, "BatchedReinforce.decide x 3")
    env.close()


def test_dqn_engine_hands_its_seed_counter_and_epsilon_to_the_select():
    """three consecutive BatchedDQN.decide calls at a constant epsilon of 0.5: the explored seats and their
    indices are select_model's at eng.seed and the successive counters, the other seats play the first maximum
    of the Q values the engine handed the kernel"""
    from rl_6_nimmt.dqn import BatchedDQN
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv
    from test_gpu_dqn_batched import _q_net

    env = VecSechsNimmtEnv(B, N, seed=3, rng="philox")
    env.reset()
    eng = BatchedDQN(env, _q_net(0).to(env.device), seats_mask=MASK, net_dtype=torch.float32, seed=M.ENGINE_SEED,
                     capacity=8192, eps_func=lambda episode: 0.5)
    eng.step_id = M.ENGINE_STEP0
    flat, gid, seat, hands = _deciders(env, eng)
    D = flat.size
    seen, q_values = [], eng._q_values

    def spy(states):
        seen.append(q_values(states))
        return seen[-1]

    eng._q_values = spy
    shares = []
    for i in range(M.ENGINE_CALLS):
        eng.actions.fill_(-7)
        actions = eng.decide(10)
        torch.cuda.synchronize()
        assert eng.eps_used == 0.5 and len(seen) == i + 1
        index = eng.best_index[:D].cpu().numpy().astype(np.int64)
        value = eng.value[:D].cpu().numpy()
        qv = seen[i][:, :104].cpu().numpy()
        step = (M.ENGINE_STEP0 + i) & 0xFFFFFFFF
        explore, explored = M.select_model(M.select_words(M.ENGINE_SEED, step, gid, seat), 0.5, 10)
        q_hand = qv[np.arange(D)[:, None], hands]
        want = np.where(explore, explored, q_hand.argmax(axis=1))
        assert np.array_equal(index, want), i
        assert np.array_equal(value, np.where(explore, np.float32(-1.0), q_hand.max(axis=1))), i
        _check_actions(env, eng, actions, index, flat, hands, i)
        shares.append(float(explore.mean()))
    assert all(0.35 < s < 0.65 for s in shares) and eng.step_id == M.ENGINE_STEP0 + M.ENGINE_CALLS
    env.close()


# ---------------------------------------------------------------- a rollout's deal
def _ro_hands(ro, num_seats):
    """the hands of a rollout state's seats: byte k of a seat's three words = its k-th card, 0xFF none ->
    [..., num_seats, 10] int64 with -1 for none"""
    ro = np.ascontiguousarray(ro[..., 8:8 + 3 * num_seats])
    hb = ro.view(np.uint8).reshape(ro.shape[:-1] + (num_seats, 12)).astype(np.int64)
    assert (hb[..., 10:] == 0xFF).all()
    return np.where(hb[..., :10] == 0xFF, -1, hb[..., :10])


def _memory(eng, flat):
    """sn_mcs_memorize's card memory of every decision, read back: sorted card lists"""
    av = eng.avail.cpu().numpy().view(np.uint32)[:, flat]
    return [[c for c in range(128) if (int(av[c >> 5, d]) >> (c & 31)) & 1] for d in range(flat.size)]


def _deal(env, eng, q):
    from rl_6_nimmt import _native as nat

    eng.ro.fill_(-3)
    nat.check(nat.lib().sn_puct_deal(env._h, ctypes.byref(q), env._stream()), "sn_puct_deal")
    torch.cuda.synchronize()
    return eng.ro[: eng.D].cpu().numpy()


DEAL_SINGLE, DEAL_BATCH = (0, 1, 5), (3, 3)  # rollouts of one sn_puct_deal each; r0, nr of sn_puct_deal_batch


def _check_deals(env, eng, n, players, step):
    """rollouts 0, 1, 5 by sn_puct_deal and 3, 4, 5 by one sn_puct_deal_batch: every opponent hand equals
    deal_model's on the memory read back, seat 0 holds the decider's own hand, the batch's rollout 5 is the
    single deal's"""
    from rl_6_nimmt import _native as nat

    seats = env.num_players
    eng.seed, eng.step_id = M.SEED, step
    eng.memorize()
    flat, gid, seat, hands = _deciders(env, eng)
    D = flat.size
    memory = _memory(eng, flat)
    assert (hands[:, :n] >= 0).all() and (hands[:, n:] < 0).all()
    dealt = {r: _deal(env, eng, eng._params(n, rollout=r)) for r in DEAL_SINGLE}
    r0, nr = DEAL_BATCH
    buf = torch.full((nr, D, 48), -3, dtype=torch.int32, device=env.device)
    nat.check(nat.lib().sn_puct_deal_batch(env._h, ctypes.byref(eng._params(n)), r0, nr, buf.data_ptr(), env._stream()),
              "sn_puct_deal_batch")
    torch.cuda.synchronize()
    batch = buf.cpu().numpy()
    assert np.array_equal(batch[5 - r0], dealt[5])
    dealt.update({r0 + i: batch[i] for i in range(nr)})
    for r, ro in sorted(dealt.items()):
        got = _ro_hands(ro, seats)
        assert np.array_equal(got[:, 0], hands), r
        assert (ro[:, 40] == 0).all() and (ro[:, 41] == -1).all(), r
        for d in range(D):
            want = M.deal_model(M.SEED, step, gid[d], seat[d], r, memory[d], n, int(players[d]), seats=seats)
            have = [[int(c) for c in got[d, s] if c >= 0] for s in range(1, seats)]
            assert have == want, (r, d, have, want)
    assert len({dealt[r].tobytes() for r in dealt}) == len(dealt)  # every rollout its own deal


DEAL_SHAPES = {2: 0b11, 4: 0b1001, 10: 0b1000000001}  # seats 0 and N - 1 decide; seat 9 reaches the stream's top bits


@pytest.mark.parametrize("n", [10, 4])
@pytest.mark.parametrize("seats", sorted(DEAL_SHAPES))
def test_deals_equal_the_model(seats, n):
    from test_gpu_puct_players import plain_engine

    env, eng = plain_engine(seats, B, DEAL_SHAPES[seats], 1)
    for t in range(10 - n):  # mid-game: every seat plays its lowest card, the memory follows every step
        eng.memorize()
        _, _, inv = env.step(env.hands()[:, :, 0].to(torch.int32))
        assert bool((inv == -1).all())
    _check_deals(env, eng, n, [seats] * eng.D, step=2**31 + 1)
    env.close()


def test_deal_reads_the_counter_from_device_memory():
    """sn_puct.step_dev overrides sn_puct.step: the deal with the counter in device memory (and another value in
    `step`) is the deal with that counter passed by value, which is the model's"""
    from test_gpu_puct_players import plain_engine

    env, eng = plain_engine(4, B, DEAL_SHAPES[4], 1)
    eng.seed = M.SEED
    eng.memorize()
    flat, gid, seat, hands = _deciders(env, eng)
    memory = _memory(eng, flat)
    step = 2**31 + 5
    eng.step_id = step
    by_value = _deal(env, eng, eng._params(10, rollout=1))
    eng._step_dev.fill_(step - 2**32)  # the same 32 bits as int32
    eng.step_id = 77
    q = eng._params(10, rollout=1, step_dev=True)
    assert q.step == 77 and q.step_dev == eng._step_dev.data_ptr()
    by_device = _deal(env, eng, q)
    assert np.array_equal(by_device, by_value)
    assert not np.array_equal(_deal(env, eng, eng._params(10, rollout=1)), by_value)  # step 77 by value: another deal
    got = _ro_hands(by_device, 4)
    for d in range(flat.size):
        want = M.deal_model(M.SEED, step, gid[d], seat[d], 1, memory[d], 10, 4)
        assert [[int(c) for c in got[d, s] if c >= 0] for s in range(1, 4)] == want, d
    env.close()


def test_deals_on_a_tournament_handle_equal_the_model():
    """a 2..6-player tournament's decision list on an N = 6 handle: a game of k players deals k - 1 opponents,
    the seats past k stay empty"""
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.agents import DrunkHamster, PUCTAgent
    from rl_6_nimmt.league import BatchedTournament

    t = BatchedTournament(53, 2, 6, seed=13)
    t.add_player("P", PUCTAgent(mc_max=12, mc_per_card=3))
    for i in range(5):
        t.add_player(f"R{i}", DrunkHamster())
    t._start()
    env = t.env
    nat.check(nat.lib().sn_reset(env._h, None, env._stream()), "sn_reset")  # a seat draw + deal
    t._use_decisions()
    eng = t.engines["P"]
    k, _ = t.seats()
    players = k.cpu().numpy()[eng.dec.cpu().numpy() // 6]
    assert eng.D > 8 and players.min() == 2 and players.max() == 6
    _check_deals(env, eng, 10, players, step=4)
    t.close()


# ---------------------------------------------------------------- a rollout's moves
@pytest.mark.parametrize("seats", sorted(M.STEP_SHAPES))
def test_lane_step_samples_equal_the_model(monkeypatch, seats):
    """sn_puct_step's one-lane-per-decision kernel at the steps t = 0 and t = 1 of rollout 2, the root sampled
    like every other seat (puct_root = 0): the card a seat played -- its hand before the step minus its hand
    after it -- is the card at step_model's index (the seat-lane and fused forms are tied to this kernel by
    test_gpu_puct_players.py::test_step_forms_agree_under_a_stochastic_policy)"""
    from rl_6_nimmt import _native as nat
    from test_gpu_puct_players import plain_engine, set_form

    set_form(monkeypatch, "lane")
    games, mask = M.STEP_SHAPES[seats]
    env, eng = plain_engine(seats, games, mask, 1)
    eng.seed, eng.step_id = M.STEP_SEED, M.STEP_STEP
    eng.memorize()
    flat, gid, seat, hands = _deciders(env, eng)
    D, L, h, st = flat.size, nat.lib(), env._h, env._stream()
    q = eng._params(10, rollout=M.STEP_ROLLOUT)
    q.puct_root = 0
    nat.check(L.sn_puct_init(h, ctypes.byref(q), nat.ptr(torch.zeros((D, 10), device=env.device)), st), "sn_puct_init")
    before = _ro_hands(_deal(env, eng, q), seats)
    for t, (logits, u) in enumerate(M.step_case(seats)):
        m = 10 - t
        assert logits.shape == (D, seats, m) and (before[..., :m] >= 0).all() and (before[..., m:] < 0).all()
        lg = torch.from_numpy(logits).to(env.device).contiguous()
        nat.check(L.sn_puct_step(h, ctypes.byref(q), nat.ptr(lg), t, m, st), "sn_puct_step")
        torch.cuda.synchronize()
        after = _ro_hands(eng.ro[:D].cpu().numpy(), seats)
        got = np.zeros((D, seats), dtype=np.int64)
        for d in range(D):
            for s in range(seats):
                old, new = before[d, s, :m].tolist(), [c for c in after[d, s].tolist() if c >= 0]
                played = sorted(set(old) - set(new))
                assert len(played) == 1 and len(new) == m - 1 and new == [c for c in old if c != played[0]], (t, d, s)
                got[d, s] = old.index(played[0])
        index, amb, lo, hi = M.step_model(M.STEP_SEED, M.STEP_STEP, gid, seat, M.STEP_ROLLOUT, t, logits)
        assert np.array_equal(M.step_uniforms(M.STEP_SEED, M.STEP_STEP, gid, seat, M.STEP_ROLLOUT, t, seats), u)
        M.check_allowed(got, index, amb, lo, hi, f"sn_puct_step (lane) N={seats} t={t}")
        before = after
    env.close()


# ---------------------------------------------------------------- rollout numbers stay below the reserved tags
def test_rollout_numbers_in_the_reserved_tags_are_refused():
    """a rollout number at or past 0xFFF00 would draw from the stream of a noise, select or sample tag:
    sn_puct_deal, sn_puct_deal_batch, sn_puct_step and sn_puct_rollouts return SN_EINVAL, say why, and write
    nothing; the last rollout number below the bound is still served"""
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.engine import ROLLOUT_TAG_END as END
    from test_gpu_puct_players import plain_engine

    env, eng = plain_engine(4, 8, MASK, 1)
    eng.memorize()
    D, L, h, st = eng.D, nat.lib(), env._h, env._stream()
    c, w2p, head, w1s = eng.sync_net().fused()
    eng.ro.fill_(-3)
    eng.stats.fill_(-3)
    buf = torch.full((3, D, 48), -3, dtype=torch.int32, device=env.device)
    lg = torch.zeros((D * 4 * 10,), device=env.device)
    refused = "reaches the reserved stream tags"
    for rollout in (END, END + 0xFE, 0xFFFFF, 2**32 - 1):
        q = eng._params(10, rollout=rollout)
        with pytest.raises(ValueError, match=f"sn_puct_deal: rollout number {rollout} {refused}"):
            nat.check(L.sn_puct_deal(h, ctypes.byref(q), st), "sn_puct_deal")
        with pytest.raises(ValueError, match=f"sn_puct_step: rollout number {rollout} {refused}"):
            nat.check(L.sn_puct_step(h, ctypes.byref(q), nat.ptr(lg), 0, 10, st), "sn_puct_step")
    q = eng._params(10)
    for r0, nr in ((END - 2, 3), (END, 1), (2**31 - 1, 1), (2**31 - 1, 2**31 - 1)):
        last = r0 + nr - 1
        with pytest.raises(ValueError, match=f"sn_puct_deal_batch: rollout number {last} {refused}"):
            nat.check(L.sn_puct_deal_batch(h, ctypes.byref(q), r0, nr, buf.data_ptr(), st), "sn_puct_deal_batch")
        with pytest.raises(ValueError, match=f"sn_puct_rollouts: rollout number {last} {refused}"):
            nat.check(L.sn_puct_rollouts(h, ctypes.byref(q), r0, nr, buf.data_ptr(), nat.ptr(w1s), nat.ptr(c),
                                         nat.ptr(w2p), nat.ptr(head), st), "sn_puct_rollouts")
    torch.cuda.synchronize()
    assert bool((eng.ro == -3).all()) and bool((buf == -3).all()) and bool((eng.stats == -3).all())  # nothing ran
    # the largest rollout numbers allowed
    nat.check(L.sn_puct_deal(h, ctypes.byref(eng._params(10, rollout=END - 1)), st), "sn_puct_deal")
    nat.check(L.sn_puct_deal_batch(h, ctypes.byref(q), END - 3, 3, buf.data_ptr(), st), "sn_puct_deal_batch")
    torch.cuda.synchronize()
    assert torch.equal(buf[2], eng.ro[:D]) and not bool((buf[:, :, : 8 + 3 * 4] == -3).any())  # board and hands dealt
    env.close()
