"""GPU checks of the batched DQN engine (rl_6_nimmt/dqn.py; sn_dqn_* and
sn_per_gather of include/sechs.h) and of its seat in the batched league.

The kernels are held to the torch models of dqn.py (pack_rows_host,
unpack_rows_host, bellman_target_host -- tied to the drop-ins on the CPU by
test_dqn_batched_cpu.py) and to the environment's own views (obs, hands,
sn_puct_root_rows), exactly.  Sizes: 130 games x 2 deciding seats = 260
decisions (past a 64-lane wave and a 256-thread block, a ragged tail).
Exploration is Philox, so it is checked in law: frequencies within 5
standard errors, the margin test_playout_sampling_follows_the_policy uses.
"""
import copy
import ctypes

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

B, N, MASK, SEATS = 130, 4, 0b0101, [0, 2]
D = B * len(SEATS)


def _q_net(seed=0, hidden=(64,)):
    from rl_6_nimmt.utils.nets import MultiHeadedMLP

    torch.manual_seed(seed)
    return MultiHeadedMLP(47, hidden_sizes=hidden, head_sizes=(104,), activation=nn.ReLU(), head_activations=(None,))


def _engine(seed=3, target=False, prioritised=False, dtype=torch.float32, **kw):
    from rl_6_nimmt.dqn import BatchedDQN
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(B, N, seed=seed)
    net = _q_net(seed).to(env.device)
    tgt = copy.deepcopy(net) if target else None
    kw.setdefault("capacity", 8192)
    return env, BatchedDQN(env, net, target_net=tgt, prioritised=prioritised, seats_mask=MASK, net_dtype=dtype,
                           seed=seed, **kw)


def _decider_obs(env):
    return env.obs()[:, SEATS].reshape(D, 47)


def _obs(env, q, num):
    """sn_dqn_obs in all three forms"""
    from rl_6_nimmt import _native as nat

    dev = env.device
    i8 = torch.full((num, 48), 77, dtype=torch.int8, device=dev)
    f32 = torch.full((num, 48), 77.0, dtype=torch.float32, device=dev)
    bf = torch.full((num, 48), 77.0, dtype=torch.bfloat16, device=dev)
    L, st = nat.lib(), env._stream()
    nat.check(L.sn_dqn_obs(env._h, ctypes.byref(q), nat.ptr(i8), nat.ptr(f32), 0, st), "sn_dqn_obs")
    nat.check(L.sn_dqn_obs(env._h, ctypes.byref(q), None, nat.ptr(bf), 1, st), "sn_dqn_obs")
    return i8, f32, bf


def test_obs_is_the_env_observation_in_all_three_forms():
    env, eng = _engine()
    env.reset()
    for t in range(11):
        if t in (0, 3, 9, 10):  # 10: after the last step, empty hands -- the terminal next_state
            want = _decider_obs(env)
            i8, f32, bf = _obs(env, eng._params(10 - t), D)
            assert torch.equal(i8[:, :47], want) and not bool(i8[:, 47].any()), t
            wf = torch.cat((want.float(), torch.zeros((D, 1), device=env.device)), dim=1)
            assert torch.equal(f32, wf) and torch.equal(bf.float(), wf), t
            if t == 10:
                assert bool((want[:, :10] == -1).all())
        if t < 10:
            env.step()


def _league(agent, train, seed=21, slots=256):
    """2-4 players need four agents on the roster (tournament.py:170): three DrunkHamsters and the DQN agent"""
    from rl_6_nimmt.agents import DrunkHamster
    from rl_6_nimmt.league import BatchedTournament

    t = BatchedTournament(slots, 2, 4, seed=seed, train=train, fused=False)
    t.add_player("R0", DrunkHamster())
    t.add_player("R1", DrunkHamster())
    t.add_player("Q", agent)
    t.add_player("R2", DrunkHamster())
    return t


def test_obs_on_a_tournament_handle_is_the_root_rows_observation():
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.agents import DQNVanilla
    from rl_6_nimmt.utils.preprocessing import SechsNimmtStateNormalization

    t = _league(DQNVanilla(history_length=1000), train=False)
    t.play_games(1)
    env, eng = t.env, t.engines["Q"]
    nat.check(nat.lib().sn_reset(env._h, None, env._stream()), "sn_reset")  # a fresh seat draw + deal
    t._use_decisions()
    n = eng.D
    assert n > 64
    q = eng._params(10)
    i8, f32, bf = _obs(env, q, n)
    rows = torch.empty((n * 10, 48), dtype=torch.float32, device=env.device)
    nat.check(nat.lib().sn_puct_root_rows(env._h, ctypes.byref(q), nat.ptr(rows), 0, env._stream()), "sn_puct_root_rows")
    want = rows.view(n, 10, 48)[:, 0, 1:].cpu()
    assert torch.equal(SechsNimmtStateNormalization()(f32.cpu()[:, :47]), want)  # host fp32: true divisions
    k, _ = t.seats()
    players = k.to(env.device).long()[eng.dec.long() // env.num_players]
    assert int(players.min()) == 2 and int(players.max()) == 4
    assert torch.equal(i8[:, 10].long(), players) and torch.equal(f32[:, 10].long(), players)
    assert torch.equal(bf.float(), f32) and torch.equal(i8.float(), f32)
    t.close()


def _select(env, q, qv, eps):
    from rl_6_nimmt import _native as nat

    dev = env.device
    actions = torch.full((B, N), -7, dtype=torch.int32, device=dev)
    index = torch.full((D,), -7, dtype=torch.int32, device=dev)
    value = torch.full((D,), -7.0, dtype=torch.float32, device=dev)
    nat.check(nat.lib().sn_dqn_select(env._h, ctypes.byref(q), nat.ptr(qv), qv.stride(0), float(eps), nat.ptr(actions),
                                      nat.ptr(index), nat.ptr(value), env._stream()), "sn_dqn_select")
    return actions, index, value


def test_select_is_epsilon_greedy_over_the_hand():
    env, eng = _engine()
    env.reset()
    dev = env.device
    hands = env.hands()[:, SEATS].reshape(D, 10).long()
    g = torch.Generator().manual_seed(9)
    wide = torch.full((D, 112), 1e9, device=dev)  # a padded head: q_stride 112, the pad never read
    qv = wide[:, :104]
    qv.copy_(torch.randn((D, 104), generator=g).to(dev))
    legal = torch.zeros((D, 104), dtype=torch.bool, device=dev)
    legal[torch.arange(D, device=dev)[:, None], hands] = True
    illegal_card = (~legal).float().argmax(dim=1)
    qv[torch.arange(D, device=dev), illegal_card] = 50.0  # the global maximum sits on an illegal card
    pos = torch.stack([torch.randperm(10, generator=g)[:2] for _ in range(D)]).to(dev)
    lo = pos.min(dim=1).values
    for j in range(2):  # two legal cards share the legal maximum: the lower card (first position) wins
        qv[torch.arange(D, device=dev), hands[torch.arange(D, device=dev), pos[:, j]]] = 7.0
    q = eng._params(10)
    actions, index, value = _select(env, q, qv, 0.0)
    assert torch.equal(index.long(), lo)
    assert torch.equal(actions[:, SEATS].reshape(D).long(), hands[torch.arange(D, device=dev), lo])
    assert bool((value == 7.0).all())
    assert bool((actions[:, [1, 3]] == -7).all())  # deciding seats only
    # eps = 1: always a uniform legal card, value -1; eps = 0.3: that share explores
    counts, explored, total = torch.zeros(10, dtype=torch.long), 0, 0
    for step in range(64):
        eng.step_id = step
        q = eng._params(10)
        a, i, v = _select(env, q, qv, 1.0)
        assert bool((v == -1.0).all())
        assert torch.equal(a[:, SEATS].reshape(D).long(), hands[torch.arange(D, device=dev), i.long()])
        counts += torch.bincount(i.long().cpu(), minlength=10)
        a, i, v = _select(env, q, qv, 0.3)
        assert torch.equal(a[:, SEATS].reshape(D).long(), hands[torch.arange(D, device=dev), i.long()])
        ex = v == -1.0
        assert torch.equal(i.long()[~ex], lo[~ex]) and bool((v[~ex] == 7.0).all())
        explored += int(ex.sum())
        total += D
    assert total == 16640
    freq = counts.double() / total
    se = (0.1 * 0.9 / total) ** 0.5
    assert bool(((freq - 0.1).abs() < 5 * se).all()), freq
    assert abs(explored / total - 0.3) < 5 * (0.3 * 0.7 / total) ** 0.5, explored / total
    # the draws are a function of (seed, step)
    eng.step_id = 5
    x = _select(env, eng._params(10), qv, 0.5)
    y = _select(env, eng._params(10), qv, 0.5)
    eng.step_id = 6
    z = _select(env, eng._params(10), qv, 0.5)
    assert all(torch.equal(a, b) for a, b in zip(x, y))
    assert not torch.equal(x[1], z[1]) and not torch.equal(x[2], z[2])


def _sequential_counters(stores, cap):
    """SumTree.add x stores: (data_pointer, num_items)"""
    pointer = items = 0
    for _ in range(stores):
        pointer += 1
        if pointer >= cap:
            pointer = 0
        else:
            items += 1
    return pointer, items


def test_episode_transitions_pack_unpack_and_fill_the_ring():
    from rl_6_nimmt.dqn import pack_rows_host, unpack_rows_host

    cap = 1024
    env, eng = _engine(capacity=cap, eps_func=lambda e: 0.5)
    dev = env.device
    keep = torch.tensor([(MASK >> p) & 1 for p in range(N)], dtype=torch.bool, device=dev)
    env.reset()
    snaps, acts = [], []
    per_step = torch.zeros((10, B, N), dtype=torch.int32, device=dev)
    for t in range(10):
        snaps.append(_decider_obs(env).clone())
        full = torch.where(keep[None, :], eng.decide(10 - t, record=True), eng._random_moves())
        acts.append(full[:, SEATS].reshape(D).clone())
        rew, done, inv = env.step(full)
        assert bool((inv < 0).all())
        per_step[t] = rew
    snaps.append(_decider_obs(env).clone())
    rows = eng.end_episode(per_step)
    seen = torch.zeros((10, D), dtype=torch.int32, device=dev)
    seen[1:] = per_step[:9][:, :, SEATS].reshape(9, D)  # GameSession's one-step lag; the last reward is never seen
    want = pack_rows_host(torch.stack(snaps), torch.stack(acts), seen)
    assert rows.shape == (10 * D, 112) and torch.equal(rows, want)
    assert int(rows[:, 97].sum()) == D and bool((rows[9 * D:, 97] == 1).all())
    assert torch.equal(rows[:, 98].long().cpu(), (10 - torch.arange(10)).repeat_interleave(D))
    for got, model in zip(eng.unpack(rows), unpack_rows_host(rows)):
        assert got.dtype == model.dtype and torch.equal(got, model)
    # 2600 rows through a 1024-slot ring, in calls of at most `capacity` rows = 2600 sequential stores
    assert (eng.replay.pointer, len(eng.replay)) == _sequential_counters(10 * D, cap) == (552, 2598)
    newest = torch.arange(cap) + ((10 * D - 1 - torch.arange(cap)) // cap) * cap
    assert torch.equal(eng.replay.gather(torch.arange(cap, dtype=torch.int32, device=dev)), rows[newest.to(dev)])
    assert eng.episode == 1 and eng.eps_history == [0.5]


def _q_with_ties(n, seed, stride, dev):
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((n, stride), 1e9)  # pad columns (stride 112) would win if they were read
    q = buf[:, :104]
    q.copy_(torch.randn((n, 104), generator=g))
    for i in range(0, n, 3):  # the row maximum twice: the lowest index counts
        a, b = (int(x) for x in torch.randperm(104, generator=g)[:2])
        q[i, a] = q[i, b] = q[i].max() + 1.0
    return buf.to(dev)[:, :104]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("stride", [104, 112])
def test_bellman_targets_are_bit_equal_to_the_torch_expression(n, stride):
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.dqn import bellman_target_host

    nat.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    ql, qt = _q_with_ties(n, 31, stride, dev), _q_with_ties(n, 32, stride, dev)
    g = torch.Generator().manual_seed(33)
    reward = (-torch.randint(0, 40, (n,), generator=g).float()).to(dev)
    not_done = (torch.rand((n,), generator=g) >= 0.3).float().to(dev)
    not_done[0] = 0.0
    gamma = 0.97
    for target_q in (None, qt):
        out = torch.full((n,), 77.0, device=dev)
        nat.check(nat.lib().sn_dqn_target(n, nat.ptr(ql), nat.ptr(target_q), stride, nat.ptr(reward), nat.ptr(not_done),
                                          gamma, nat.ptr(out), nat.stream_handle(dev)), "sn_dqn_target")
        assert torch.equal(out, bellman_target_host(ql, target_q, reward, not_done, gamma)), (n, stride)
    assert float(out[0]) == float(reward[0])  # a done row keeps the reward alone


def test_gather_returns_the_stored_rows_and_zeros_out_of_range():
    from rl_6_nimmt.replay import DevicePER

    cap = 300
    per = DevicePER(cap, 112)
    g = torch.Generator().manual_seed(4)
    rows = torch.randint(1, 256, (500, 112), generator=g).to(torch.uint8).cuda()
    per.store(rows[:200])
    slots = torch.tensor([0, 5, 199, 150, 64, 65], dtype=torch.int32).cuda()
    assert torch.equal(per.gather(slots), rows[slots.long()])
    per.store(rows[200:500])  # wraps: slot s holds row s + 300 for s < 200
    slots = torch.tensor([0, 5, 199, 200, 299, 150, -1, 300, 2**31 - 1, 7], dtype=torch.int32).cuda()
    got = per.gather(slots)
    src = torch.tensor([300, 305, 499, 200, 299, 450, 0, 0, 0, 307]).cuda()
    want = rows[src]
    want[6:9] = 0
    assert torch.equal(got, want)
    per.close()


VARIANTS = {"dqn": (False, False), "ddqn": (True, False), "dqn_prb": (False, True), "ddqn_prb": (True, True)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_loss_terms_and_learn_follow_the_dropin(variant):
    from rl_6_nimmt.dqn import bellman_target_host, unpack_rows_host

    double, prioritised = VARIANTS[variant]
    tau, gamma = 0.25, 0.97
    env, eng = _engine(seed=5, target=double, prioritised=prioritised, minibatch=64, updates=1, retrain_interval=2,
                       tau=tau, gamma=gamma, eps_func=lambda e: 0.3)
    dev = env.device
    net, tgt = eng.actor, eng.target_net
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    # the gate: a replay of exactly `minibatch` rows does not learn
    before = [p.detach().clone() for p in net.parameters()]
    eng.play_episode(record=True)
    rows0 = eng.replay.gather(torch.arange(64, dtype=torch.int32, device=dev))
    env2, gate = _engine(seed=5, target=double, prioritised=prioritised, minibatch=64)
    gate.replay.store(rows0)
    assert len(gate.replay) == 64 and gate.learn(torch.optim.Adam(gate.actor.parameters())) == []
    assert all(torch.equal(a, b) for a, b in zip(gate.actor.parameters(), before))
    eng.play_episode(record=True)
    assert len(eng.replay) == 2 * 10 * D and eng.episode == 2

    gen = torch.Generator().manual_seed(8)
    u = torch.rand(64, generator=gen, dtype=torch.float64)
    slots = torch.randperm(2 * 10 * D, generator=gen)[:64].to(torch.int32)

    sample = eng.sample_batch

    def fixed_batch():
        return sample(u=u) if prioritised else sample(slots=slots)

    batch = fixed_batch()
    q_eval, target, weights, loss = eng.loss_terms(batch)
    s, s2, a, r, nd = unpack_rows_host(batch["rows"])
    with torch.no_grad():
        qn = net(s2[:, :47])[0]
        qt = tgt(s2[:, :47])[0] if double else None
    want_target = bellman_target_host(qn, qt, r, nd, gamma)
    assert torch.equal(target, want_target)
    want_eval = torch.squeeze(net(s[:, :47])[0].gather(1, a.view(-1, 1)))  # DQNVanilla._learn
    assert torch.equal(q_eval, want_eval)
    if prioritised:  # DQN_PRBAgent._optimize_loss
        assert weights.dtype == torch.float32 and torch.equal(weights, batch["weights"].float())
        want_loss = (weights * (want_eval - want_target) ** 2).mean()
    else:
        assert weights is None
        want_loss = nn.functional.mse_loss(want_eval, want_target)
    assert torch.equal(loss, want_loss)
    err = torch.abs(q_eval.detach() - target).double().cpu()

    eng.sample_batch = fixed_batch  # learn() trains on the batch above
    local0 = [p.detach().clone() for p in net.parameters()]
    target0 = [p.detach().clone() for p in tgt.parameters()] if double else None
    losses = eng.learn(opt)  # update 1: no soft update at retrain_interval 2
    assert len(losses) == 1
    if not prioritised:  # (a second PER sample has moved beta, and with it the weights)
        assert torch.equal(losses[0], want_loss)
    assert any(not torch.equal(p, q) for p, q in zip(net.parameters(), local0))
    if double:
        assert all(torch.equal(p, q) for p, q in zip(tgt.parameters(), target0))
    if prioritised:
        tree = eng.replay.tree().cpu()
        cap = eng.capacity
        last = {}
        for i, e in zip(batch["idx"].cpu().tolist(), err.tolist()):
            last[i] = e  # batch_update is sequential: the last of a repeated index wins
        idx = torch.tensor(sorted(last))
        want_leaf = torch.tensor([min(last[i] + 0.01, 1.0) ** 0.6 for i in sorted(last)], dtype=torch.float64)
        assert bool(((tree[idx] - want_leaf).abs() <= 1e-12 * want_leaf).all())
        inner = torch.arange(cap - 1)
        assert torch.equal(tree[inner], tree[2 * inner + 1] + tree[2 * inner + 2])
    local1 = [p.detach().clone() for p in net.parameters()]
    assert len(eng.learn(opt)) == 1 and eng.update_count == 2  # update 2: the target net follows
    if double:
        for p, l, t0 in zip(tgt.parameters(), local1, target0):
            assert torch.equal(p, tau * l + (1 - tau) * t0) and not torch.equal(p, t0)


def _model_counters(round_rows, cap):
    pointer = items = 0
    for rows in round_rows:
        for _ in range(rows):
            pointer += 1
            if pointer >= cap:
                pointer = 0
            else:
                items += 1
    return pointer, items


@pytest.mark.parametrize("kind", ["dqn", "ddqn", "dqn_prb", "ddqn_prb"])
def test_league_seats_and_trains_a_dqn_agent(kind):
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.dqn import BatchedDQN
    from rl_6_nimmt.league import T_STEPS, decode_seats

    def eps_func(episode):
        return max(0.9 - 0.4 * episode, 0.1)

    torch.manual_seed(2)
    agent = A.DQN_AGENTS[kind](history_length=1000, eps_func=eps_func, minibatch=64)
    before = [p.detach().clone() for p in agent.dqn_net_local.parameters()]
    t = _league(agent, train=True)
    rec = t.play_games(1)
    rec = torch.cat((rec, t.play_games(1)), dim=0)  # an illegal move of the engine would raise in the round
    eng = t.engines["Q"]
    assert isinstance(eng, BatchedDQN) and eng.prioritised == ("prb" in kind) and (eng.target_net is not None) == \
        kind.startswith("ddqn")
    assert eng.minibatch == 256 and eng.updates == T_STEPS and eng.capacity == 4096
    k, ids = decode_seats(rec[..., 0], 4)
    seated = (ids == 2).sum(dim=(1, 2)).tolist()  # "Q" is the third active agent
    assert min(seated) > 0
    st = t.agent_stats()
    assert int(st[:, 0].sum()) == int(k.sum()) and int(st[2, 0]) == sum(seated)
    assert t.env.pipe_errors() == 0
    assert (eng.replay.pointer, len(eng.replay)) == _model_counters([10 * s for s in seated], eng.capacity)
    assert any(not torch.equal(a.detach().cpu(), b) for a, b in zip(agent.dqn_net_local.parameters(), before))
    assert t.optimizer_steps["Q"] == 2 * T_STEPS and eng.update_count == 2 * T_STEPS
    assert eng.eps_history == [eps_func(0), eps_func(1)]
    t.close()


@pytest.mark.parametrize("kind", ["dqn", "ddqn", "dqn_prb", "ddqn_prb"])
def test_league_with_a_greedy_dqn_agent_is_deterministic(kind):
    from rl_6_nimmt.agents import DQN_AGENTS

    torch.manual_seed(3)
    agent = DQN_AGENTS[kind](history_length=1000)
    assert agent.eps == 0
    recs = []
    for _ in range(2):
        t = _league(copy.deepcopy(agent), train=False, seed=22)
        recs.append(t.play_games(2).cpu())
        assert len(t.engines["Q"].replay) == 0 and t.engines["Q"].eps_history == [0.0, 0.0]
        t.close()
    assert torch.equal(recs[0], recs[1])
