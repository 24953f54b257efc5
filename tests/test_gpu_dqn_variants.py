"""GPU checks of the duelling and n-step DQN variants: the kernels
sn_dqn_pack_nstep, sn_dqn_unpack_nstep and sn_dqn_select_duel against their
torch models (rl_6_nimmt/dqn.py: pack_rows_nstep_host, unpack_rows_nstep_host,
duelling_q_host -- tied to the reference by test_dqn_variants_cpu.py), the
engine built on them, its seat in the batched league, and the drop-in agents
on the recorded sessions of golden F17.

The models run on the host, as the reference's agents do (the host's
A.mean is sum / 104, the division the kernel makes).
"""
import copy
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SPEC = json.load(open(os.path.join(GOLDEN, "dqn_variant_games.json")))


# ---------------------------------------------------------------- sn_dqn_pack_nstep / sn_dqn_unpack_nstep
def _episode(T, D, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randint(-1, 104, (T + 1, D, 48), generator=g).to(torch.int8)
    obs[..., 47] = 0
    for t in range(T + 1):  # hands of T - t cards, -1 padded
        obs[t, :, T - t:10] = -1
        obs[t, :, : T - t].clamp_(min=0)
    actions = torch.randint(0, 104, (T, D), generator=g).to(torch.int32)
    rewards = -torch.randint(0, 71, (T, D), generator=g).to(torch.int32)  # -70..0
    return obs, actions, rewards


def _pack_nstep(obs, actions, rewards, n, gamma, dev):
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.dqn import gamma_powers

    T, D = actions.shape
    o, a, r = obs.to(dev).contiguous(), actions.to(dev).contiguous(), rewards.to(dev).contiguous()
    rows = torch.full((T * D, 112), 0xAB, dtype=torch.uint8, device=dev)
    gpow = nat.SnDqnGpow()
    gpow.v[:] = gamma_powers(gamma)
    nat.check(nat.lib().sn_dqn_pack_nstep(T, D, n, gpow, nat.ptr(o), nat.ptr(a), nat.ptr(r), nat.ptr(rows),
                                          nat.stream_handle(dev)), "sn_dqn_pack_nstep")
    return rows


@pytest.mark.parametrize("D,T", [(1, 10), (37, 10), (300, 10), (37, 4)])
def test_pack_nstep_writes_the_models_rows(D, T):
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.dqn import pack_rows_nstep_host

    nat.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    obs, actions, rewards = _episode(T, D, 1000 * T + D)
    assert int(rewards.min()) >= -70 and int(rewards.max()) <= 0
    for gamma in (0.99, 0.5):
        for n in (1, 2, 3, 10, 11):
            got = _pack_nstep(obs, actions, rewards, n, gamma, dev).cpu()
            want = pack_rows_nstep_host(obs, actions, rewards, n, gamma)
            assert torch.equal(got, want), (n, gamma, (got != want).nonzero()[:4].tolist())


def test_pack_nstep_rejects_what_it_cannot_pack():
    from rl_6_nimmt import _native as nat

    nat.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    obs, actions, rewards = _episode(10, 2, 3)
    o, a, r = obs.to(dev), actions.to(dev), rewards.to(dev)
    rows = torch.zeros((11 * 2, 112), dtype=torch.uint8, device=dev)
    gpow = nat.SnDqnGpow()
    L, st = nat.lib(), nat.stream_handle(dev)
    for T, n in ((11, 3), (10, 0), (10, -1), (0, 3)):
        assert L.sn_dqn_pack_nstep(T, 2, n, gpow, nat.ptr(o), nat.ptr(a), nat.ptr(r), nat.ptr(rows), st) == nat.SN_EINVAL
    assert not bool(rows.any())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_unpack_nstep_reads_the_return_and_unpack_still_the_reward(n):
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.dqn import pack_rows_nstep_host, unpack_rows_host, unpack_rows_nstep_host

    nat.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    obs, actions, rewards = _episode(10, 100, 17)
    rows = pack_rows_nstep_host(obs, actions, rewards, 3, 0.99)
    rows = rows[torch.randperm(1000, generator=torch.Generator().manual_seed(n))[:n]].contiguous()
    drows = rows.to(dev)
    for name, model in (("sn_dqn_unpack_nstep", unpack_rows_nstep_host), ("sn_dqn_unpack", unpack_rows_host)):
        s = torch.full((n, 48), 77.0, device=dev)
        s2 = torch.full((n, 48), 77.0, device=dev)
        action = torch.full((n,), 77, dtype=torch.int64, device=dev)
        reward, not_done = torch.full((n,), 77.0, device=dev), torch.full((n,), 77.0, device=dev)
        nat.check(getattr(nat.lib(), name)(n, nat.ptr(drows), nat.ptr(s), nat.ptr(s2), nat.ptr(action), nat.ptr(reward),
                                           nat.ptr(not_done), nat.stream_handle(dev)), name)
        for got, want in zip((s, s2, action, reward, not_done), model(rows)):
            assert got.dtype == want.dtype and torch.equal(got.cpu(), want), name
    if n >= 63:
        a, b = unpack_rows_nstep_host(rows)[3], unpack_rows_host(rows)[3]
        assert not torch.equal(a, b) and bool((b == b.round()).all())


# ---------------------------------------------------------------- sn_dqn_select_duel
B, N = 8, 4
D = B * N
LAYOUTS = {"padded": (112, 104, 0), "packed": (105, 104, 0), "v_first": (105, 0, 1)}  # stride, v_col, a_off


def _env_engine(steps=0, seed=4):
    from rl_6_nimmt.dqn import BatchedDQN
    from rl_6_nimmt.utils.nets import MultiHeadedMLP
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(B, N, seed=seed)
    net = MultiHeadedMLP(47, (8,), (104,), nn.ReLU(), (None,)).to(env.device)
    eng = BatchedDQN(env, net, net_dtype=torch.float32, seed=seed, capacity=64)
    env.reset()
    for _ in range(steps):
        env.step()
    return env, eng


def _heads(V, A, layout, dev):
    """V [D], A [D, 104] (host) in a head buffer of the layout; whatever is not V or A would win if it were read"""
    stride, v_col, a_off = LAYOUTS[layout]
    buf = torch.full((D, stride), 1e9)
    buf[:, a_off: a_off + 104] = A
    buf[:, v_col] = V
    return buf.to(dev), stride, v_col, a_off


def _select_duel(env, q, heads, stride, v_col, a_off, eps):
    from rl_6_nimmt import _native as nat

    dev = env.device
    actions = torch.full((B, N), -7, dtype=torch.int32, device=dev)
    index = torch.full((D,), -7, dtype=torch.int32, device=dev)
    value = torch.full((D,), -7.0, dtype=torch.float32, device=dev)
    nat.check(nat.lib().sn_dqn_select_duel(env._h, ctypes.byref(q), nat.ptr(heads), stride, v_col, a_off, float(eps),
                                           nat.ptr(actions), nat.ptr(index), nat.ptr(value), env._stream()),
              "sn_dqn_select_duel")
    return actions.cpu(), index.cpu(), value.cpu()


def _select_plain(env, q, qv, eps):
    from rl_6_nimmt import _native as nat

    dev = env.device
    qv = qv.to(dev).contiguous()
    actions = torch.full((B, N), -7, dtype=torch.int32, device=dev)
    index = torch.full((D,), -7, dtype=torch.int32, device=dev)
    value = torch.full((D,), -7.0, dtype=torch.float32, device=dev)
    nat.check(nat.lib().sn_dqn_select(env._h, ctypes.byref(q), nat.ptr(qv), qv.stride(0), float(eps), nat.ptr(actions),
                                      nat.ptr(index), nat.ptr(value), env._stream()), "sn_dqn_select")
    return actions.cpu(), index.cpu(), value.cpu()


def _integer_heads(hands, held, seed):
    """integer V and A (every sum exact in any order); two legal cards share the best legal Q, an illegal card
    beats them.  Returns V, A, the hand position that must win."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-50, 51, (D, 104), generator=g).float()
    V = torch.randint(-30, 31, (D,), generator=g).float()
    rows = torch.arange(D)
    legal = torch.zeros((D, 104), dtype=torch.bool)
    legal[rows[:, None], hands[:, :held]] = True
    A[rows, (~legal).float().argmax(dim=1)] = 90.0
    pos = torch.stack([torch.randperm(held, generator=g)[:2] for _ in range(D)])
    for j in range(2):
        A[rows, hands[rows, pos[:, j]]] = 60.0
    return V, A, pos.min(dim=1).values


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_select_duel_is_select_on_the_duelling_q_bit_for_bit(layout):
    from rl_6_nimmt.dqn import duelling_q_host

    env, eng = _env_engine()
    hands = env.hands().reshape(D, 10).long().cpu()
    assert bool((hands[:, 1:] > hands[:, :-1]).all())  # ascending
    V, A, lo = _integer_heads(hands, 10, 9)
    Q = duelling_q_host(V[:, None], A)
    assert not bool((A.sum(dim=1) % 104 == 0).all())  # the mean is no integer: its rounding takes part
    heads, stride, v_col, a_off = _heads(V, A, layout, env.device)
    rows = torch.arange(D)
    q = eng._params(10)
    actions, index, value = _select_duel(env, q, heads, stride, v_col, a_off, 0.0)
    assert torch.equal(index.long(), lo)  # the first maximum over the ascending hand
    assert torch.equal(actions.reshape(D).long(), hands[rows, lo])
    assert torch.equal(value, Q[rows, hands[rows, lo]])
    for got, want in zip((actions, index, value), _select_plain(env, q, Q, 0.0)):
        assert torch.equal(got, want)
    # the same Philox keys and exploring branch: at every eps and step the plain kernel on Q decides alike
    explored = 0
    for step in range(6):
        eng.step_id = step
        q = eng._params(10)
        for eps in (1.0, 0.3):
            got = _select_duel(env, q, heads, stride, v_col, a_off, eps)
            want = _select_plain(env, q, Q, eps)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (step, eps)
            ex = got[2] == -1.0
            assert bool(ex.all()) if eps == 1.0 else True
            assert torch.equal(got[1].long()[~ex], lo[~ex])
            explored += int(ex.sum()) if eps == 0.3 else 0
    assert 0 < explored < 6 * D


def test_select_duel_with_a_hand_shorter_than_n():
    from rl_6_nimmt.dqn import duelling_q_host

    env, eng = _env_engine(steps=3)
    hands = env.hands().reshape(D, 10).long().cpu()
    assert bool((hands[:, :7] >= 0).all()) and bool((hands[:, 7:] < 0).all())
    V, A, lo = _integer_heads(hands, 7, 10)
    Q = duelling_q_host(V[:, None], A)
    rows = torch.arange(D)
    for layout in sorted(LAYOUTS):
        heads, stride, v_col, a_off = _heads(V, A, layout, env.device)
        q = eng._params(10)  # three more than the hands hold: the scan ends with the hand
        actions, index, value = _select_duel(env, q, heads, stride, v_col, a_off, 0.0)
        assert torch.equal(index.long(), lo) and torch.equal(value, Q[rows, hands[rows, lo]])
        assert torch.equal(actions.reshape(D).long(), hands[rows, lo])
        for got, want in zip((actions, index, value), _select_plain(env, q, Q, 0.0)):
            assert torch.equal(got, want)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_select_duel_on_random_heads_within_the_summation_bound(layout):
    """tol = 2^-17 * (|V| + 2 max|A|) per row: 128 roundings' worth (103 additions, the divide, the combine),
    from the summation bound, not from a measurement"""
    from rl_6_nimmt.dqn import duelling_q_host

    env, eng = _env_engine()
    hands = env.hands().reshape(D, 10).long().cpu()
    g = torch.Generator().manual_seed(12)
    A = torch.randn((D, 104), generator=g) * 3.0
    V = torch.randn((D,), generator=g) * 10.0
    rows = torch.arange(D)
    lift = hands[rows, torch.randint(0, 10, (D,), generator=g)]  # one legal card a clear best
    A[rows, lift] = A[rows[:, None], hands].max(dim=1).values + 1.0
    Q = duelling_q_host(V[:, None], A)
    tol = 2.0 ** -17 * (V.abs() + 2 * A.abs().max(dim=1).values)
    legal_q = Q[rows[:, None], hands]
    top = legal_q.sort(dim=1, descending=True).values
    clear = (top[:, 0] - top[:, 1]) >= 16 * tol
    assert int(clear.sum()) == D  # no row skipped
    heads, stride, v_col, a_off = _heads(V, A, layout, env.device)
    actions, index, value = _select_duel(env, eng._params(10), heads, stride, v_col, a_off, 0.0)
    want = legal_q.argmax(dim=1)
    assert torch.equal(index.long(), want) and torch.equal(actions.reshape(D).long(), hands[rows, want])
    err = (value - Q[rows, hands[rows, want]]).abs()
    print("select_duel |value - model| max", float(err.max()), "tol min", float(tol.min()))
    assert bool((err <= tol).all())


def test_select_duel_rejects_overlapping_columns():
    from rl_6_nimmt import _native as nat

    env, eng = _env_engine()
    heads = torch.zeros((D, 112), device=env.device)
    acts = torch.zeros((B, N), dtype=torch.int32, device=env.device)
    q = eng._params(10)
    for stride, v_col, a_off in ((112, 50, 0), (112, 104, 9), (104, 104, 0), (112, 112, 0), (112, -1, 0)):
        assert nat.lib().sn_dqn_select_duel(env._h, ctypes.byref(q), nat.ptr(heads), stride, v_col, a_off, 0.0,
                                            nat.ptr(acts), None, None, env._stream()) == nat.SN_EINVAL


# ---------------------------------------------------------------- the engine
EB, MASK, SEATS = 16, 0b0101, [0, 2]
ED = EB * len(SEATS)


def _duelling_net(seed, hidden=(64,)):
    from rl_6_nimmt.utils.nets import DuellingDQNNet

    torch.manual_seed(seed)
    return DuellingDQNNet(47, hidden_sizes=hidden, out_size=104, activation=nn.ReLU())


def _plain_net(seed, hidden=(64,)):
    from rl_6_nimmt.utils.nets import MultiHeadedMLP

    torch.manual_seed(seed)
    return MultiHeadedMLP(47, hidden_sizes=hidden, head_sizes=(104,), activation=nn.ReLU(), head_activations=(None,))


def _engine(seed=3, duelling=True, target=False, prioritised=False, **kw):
    from rl_6_nimmt.dqn import BatchedDQN
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(EB, N, seed=seed)
    net = (_duelling_net if duelling else _plain_net)(seed).to(env.device)
    tgt = copy.deepcopy(net) if target else None
    kw.setdefault("capacity", 1024)
    kw.setdefault("net_dtype", torch.float32)
    return env, BatchedDQN(env, net, target_net=tgt, prioritised=prioritised, seats_mask=MASK, seed=seed, **kw)


def _staged(eng, per_step):
    return eng._obs.cpu(), eng._acts.cpu(), eng.rewards_seen(per_step, 10).cpu()


def test_engine_decides_by_the_duelling_q_of_its_net():
    """the greedy engine's cards are the arg-max of the module's own Q over the hand (fp32 device copy)"""
    env, eng = _engine(eps_func=lambda e: 0.0)
    env.reset()
    hands = env.hands()[:, SEATS].reshape(ED, 10).long()
    obs = env.obs()[:, SEATS].reshape(ED, 47).float()
    with torch.no_grad():
        (Q,) = eng.actor(obs)
    legal_q = Q[torch.arange(ED, device=env.device)[:, None], hands]
    top = legal_q.sort(dim=1, descending=True).values
    clear = (top[:, 0] - top[:, 1]) > 1e-3  # GEMM and mean orders differ between the two forms
    assert int(clear.sum()) >= ED // 2
    acts = eng.decide(10)[:, SEATS].reshape(ED).long()
    want = hands[torch.arange(ED, device=env.device), legal_q.argmax(dim=1)]
    assert torch.equal(acts[clear], want[clear])
    assert bool(((eng.value[:ED] - top[:, 0]).abs() < 1e-3).all())
    assert eng.duelling and eng._net.head_sizes == [104, 1] and eng._net.head_w.shape[1] == 112


def test_engine_stores_the_nstep_rows_of_its_staged_episode():
    from rl_6_nimmt.dqn import pack_rows_nstep_host, unpack_rows_nstep_host

    env, eng = _engine(n_steps=3, gamma=0.97, eps_func=lambda e: 0.5)
    _, per_step = eng.play_episode(record=True)
    assert len(eng.replay) == 10 * ED
    rows = eng.replay.gather(torch.arange(10 * ED, dtype=torch.int32, device=env.device))
    want = pack_rows_nstep_host(*_staged(eng, per_step), 3, 0.97)
    assert torch.equal(rows.cpu(), want)
    assert int(rows[:, 97].sum()) == 2 * ED and bool((rows[:, 99].cpu().view(10, ED)[:, 0] ==
                                                      torch.tensor([3] * 8 + [2, 1])).all())
    for got, model in zip(eng.unpack(rows), unpack_rows_nstep_host(want)):
        assert got.dtype == model.dtype and torch.equal(got.cpu(), model)


def test_plain_one_step_engine_stores_todays_rows():
    from rl_6_nimmt.dqn import pack_rows_host, unpack_rows_host

    env, eng = _engine(duelling=False, eps_func=lambda e: 0.5)
    assert eng.n_steps == 1 and not eng.duelling
    _, per_step = eng.play_episode(record=True)
    rows = eng.replay.gather(torch.arange(10 * ED, dtype=torch.int32, device=env.device))
    want = pack_rows_host(*_staged(eng, per_step))
    assert torch.equal(rows.cpu(), want) and not bool(rows[:, 99].any()) and not bool(rows[:, 104:].any())
    for got, model in zip(eng.unpack(rows), unpack_rows_host(want)):
        assert got.dtype == model.dtype and torch.equal(got.cpu(), model)


def test_loss_terms_of_the_d3qn_prb_nstep_engine_follow_the_dropin():
    from rl_6_nimmt.dqn import bellman_target_host, unpack_rows_nstep_host

    gamma = 0.97
    env, eng = _engine(seed=5, target=True, prioritised=True, n_steps=3, minibatch=64, updates=1, gamma=gamma,
                       eps_func=lambda e: 0.3)
    net, tgt = eng.actor, eng.target_net
    with torch.no_grad():
        for p in tgt.parameters():  # a target net of its own: the double-DQN pick is visible
            p.add_(0.05 * torch.randn_like(p))
    eng.play_episode(record=True)
    assert len(eng.replay) == 10 * ED > 64
    u = torch.rand(64, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    batch = eng.sample_batch(u=u)
    q_eval, target, weights, loss = eng.loss_terms(batch)
    s, s2, a, r, nd = (x.to(env.device) for x in unpack_rows_nstep_host(batch["rows"].cpu()))
    assert not torch.equal(r, r.round())  # n-step returns, not the raw rewards
    with torch.no_grad():
        qn, qt = net(s2[:, :47])[0], tgt(s2[:, :47])[0]
    want_target = bellman_target_host(qn, qt, r, nd, gamma ** 3)
    assert target.dtype == torch.float32 and torch.equal(target, want_target)
    want_eval = torch.squeeze(net(s[:, :47])[0].gather(1, a.view(-1, 1)))
    assert torch.equal(q_eval, want_eval)
    assert weights.dtype == torch.float32 and torch.equal(weights, batch["weights"].float())
    want_loss = (weights * (want_eval - want_target) ** 2).mean()  # DQN_PRBAgent._optimize_loss
    assert loss.dtype == torch.float32 and torch.equal(loss, want_loss)
    before = [p.detach().clone() for p in net.parameters()]
    assert len(eng.learn(torch.optim.Adam(net.parameters(), lr=1e-2))) == 1
    assert any(not torch.equal(p, q) for p, q in zip(net.parameters(), before))


# ---------------------------------------------------------------- the league
KINDS = ["duelling_dqn", "duelling_ddqn", "duelling_ddqn_prb", "dqn_nstep", "d3qn_prb_nstep"]


def _league(agent, train, seed=21, slots=256):
    from rl_6_nimmt.agents import DrunkHamster
    from rl_6_nimmt.league import BatchedTournament

    t = BatchedTournament(slots, 2, 4, seed=seed, train=train, fused=False)
    t.add_player("R0", DrunkHamster())
    t.add_player("R1", DrunkHamster())
    t.add_player("Q", agent)
    t.add_player("R2", DrunkHamster())
    return t


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


def _variant(kind, **kw):
    from rl_6_nimmt.agents import DQN_VARIANT_AGENTS

    if "nstep" in kind:
        kw["n_steps"] = 3
    return DQN_VARIANT_AGENTS[kind](history_length=1000, **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_league_seats_and_trains_a_variant(kind):
    from rl_6_nimmt.dqn import BatchedDQN
    from rl_6_nimmt.league import T_STEPS, decode_seats
    from rl_6_nimmt.utils.nets import DuellingDQNNet

    def eps_func(episode):
        return max(0.9 - 0.4 * episode, 0.1)

    torch.manual_seed(2)
    agent = _variant(kind, eps_func=eps_func, minibatch=64)
    before = [p.detach().clone() for p in agent.dqn_net_local.parameters()]
    t = _league(agent, train=True)
    rec = t.play_games(1)
    rec = torch.cat((rec, t.play_games(1)), dim=0)  # an illegal move of the engine would raise in the round
    eng = t.engines["Q"]
    assert isinstance(eng, BatchedDQN) and eng.prioritised == ("prb" in kind)
    assert (eng.target_net is not None) == ("ddqn" in kind or "d3qn" in kind)
    assert eng.duelling == isinstance(agent.dqn_net_local, DuellingDQNNet) == (kind != "dqn_nstep")
    assert eng.n_steps == (3 if "nstep" in kind else 1)
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


@pytest.mark.parametrize("kind", KINDS)
def test_league_with_a_greedy_variant_is_deterministic(kind):
    torch.manual_seed(3)
    agent = _variant(kind)
    assert agent.eps == 0
    recs = []
    for _ in range(2):
        t = _league(copy.deepcopy(agent), train=False, seed=22)
        recs.append(t.play_games(2).cpu())
        assert len(t.engines["Q"].replay) == 0 and t.engines["Q"].eps_history == [0.0, 0.0]
        t.close()
    assert torch.equal(recs[0], recs[1])


# ---------------------------------------------------------------- the drop-ins on golden F17
@pytest.mark.parametrize("si", range(len(SPEC["sessions"])))
def test_dropin_variants_replay_reference_training_sessions(si):
    """tests/test_gpu_dqn.py's comparisons and tolerances on the duelling and n-step sessions"""
    from rl_6_nimmt import GameSession
    from rl_6_nimmt.agents import DQN_VARIANT_AGENTS, DrunkHamster

    sess = SPEC["sessions"][si]
    W = np.load(os.path.join(GOLDEN, "dqn_variant_weights.npz"))
    cls = {c.__name__: c for c in DQN_VARIANT_AGENTS.values()}[sess["agent"]]
    torch.manual_seed(sess["seed"])
    kw = dict(sess["kwargs"])
    if sess["eps_const"] is not None:
        kw["eps_func"] = lambda episode, _c=sess["eps_const"]: _c
    agent = cls(**kw)
    agents = [agent] + [DrunkHamster() for _ in range(3)]
    agent.train()
    for k, v in agent.state_dict().items():  # the target net starts as the local net's copy: stored once
        assert np.array_equal(v.numpy(), W[f"s{si}_init_{k.replace('dqn_net_target.', 'dqn_net_local.', 1)}"]), k
    steps, losses, per_idx = [], [], []
    fwd, lrn = agent.forward, agent.learn

    def fwd_rec(state, **k):
        act, info = fwd(state, **k)
        steps.append([int(act), float(info["value"]), float(info["eps"])])
        return act, info

    def lrn_rec(*a, **k):
        loss = lrn(*a, **k)
        assert isinstance(loss, np.ndarray) and loss.shape == (1,)
        losses.append(float(loss[0]))
        return loss

    agent.forward, agent.learn = fwd_rec, lrn_rec
    prb = "beta" in sess
    if prb:
        smp = agent.history.sample

        def smp_rec(n):
            res = smp(n)
            per_idx.append([int(x) for x in res[0]])
            return res

        agent.history.sample = smp_rec
    np.random.seed(sess["seed"])
    random.seed(sess["seed"])
    s = GameSession(*agents)
    for _ in range(sess["games"]):
        s.play_game()
    assert [[int(x) for x in r] for r in s.results] == sess["results"]
    got = np.array(steps)
    want = np.stack([W[f"s{si}_actions"].astype(np.float64), W[f"s{si}_values"], W[f"s{si}_eps"]], axis=1)
    assert np.array_equal(got[:, 0], want[:, 0])  # every move
    assert np.array_equal(got[:, 1] == -1, want[:, 1] == -1)  # the same exploring / greedy decisions
    assert int((want[:, 1] != -1).sum()) == sess["greedy_steps"]
    assert np.allclose(got[:, 2], want[:, 2], rtol=1e-12, atol=0)
    assert np.allclose(got[:, 1], want[:, 1], rtol=0, atol=1e-3)
    assert len(losses) == len(W[f"s{si}_losses"])
    assert np.allclose(losses, W[f"s{si}_losses"], rtol=1e-3, atol=1e-4)
    if prb:
        assert per_idx == W[f"s{si}_per_idx"].tolist()
        assert agent.history.beta == sess["beta"] and len(agent.history) == sess["len"]
        assert agent.history.total_priority == pytest.approx(sess["total_priority"], rel=1e-3)
    for k, v in agent.state_dict().items():
        d = np.abs(v.detach().numpy() - W[f"s{si}_final_{k}"])
        assert np.mean(d <= 1e-4) >= 0.5 and d.max() <= 3e-3 * sess["games"], (k, d.max())
