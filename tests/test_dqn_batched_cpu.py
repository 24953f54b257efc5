"""CPU checks of the batched DQN engine's host side (rl_6_nimmt/dqn.py,
league.engine_kind): no GPU, no kernel call.

* engine_kind seats the four DQN drop-ins as "dqn" and is agent_kind for
  every other agent; agent_kind itself still has no answer for a DQN agent;
* the 112-byte transition row: documented offsets, pack -> unpack round trip
  on random transitions;
* bellman_target_host, the torch model the kernel sn_dqn_target is held to
  on the GPU, equals the drop-ins' _calc_reward bit for bit (DQNVanilla and
  DDQNAgent on the CPU, code that golden F16 pins), with ties and done rows.
"""
import numpy as np
import pytest
import torch


def test_engine_kind_seats_the_dqn_family_and_defers_otherwise():
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.league import KIND_DQN, NET_KINDS, agent_kind, engine_kind

    assert KIND_DQN == "dqn" and KIND_DQN in NET_KINDS
    for cls in (A.DQNVanilla, A.DDQNAgent, A.DQN_PRBAgent, A.DDQN_PRBAgent):
        agent = cls(history_length=8)
        assert engine_kind(agent) == "dqn", cls.__name__
        with pytest.raises(NotImplementedError):
            agent_kind(agent)
    others = [A.DrunkHamster(), A.MCSAgent(), A.PUCTAgent(), A.PolicyMCSAgent(), A.PUCTCustomedAgent(),
              A.BatchedACERAgent(), A.BatchedReinforceAgent()]
    assert sorted({agent_kind(a) for a in others}) == ["acer", "customed", "mcs", "puct", "random", "reinforce"]
    for a in others:
        assert engine_kind(a) == agent_kind(a), type(a).__name__


def _random_transitions(T, D, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randint(-1, 104, (T + 1, D, 48), generator=g).to(torch.int8)
    obs[..., 47] = 0
    for t in range(T + 1):  # hands of 10 - t cards (capped), -1 padded
        obs[t, :, max(0, min(10, T - t)):10] = -1
        obs[t, :, : max(0, min(10, T - t))].clamp_(min=0)
    actions = torch.randint(0, 104, (T, D), generator=g).to(torch.int32)
    rewards = -torch.randint(0, 70, (T, D), generator=g).to(torch.int32)
    rewards[0] = 0
    return obs, actions, rewards


def test_transition_row_layout_and_round_trip():
    from rl_6_nimmt import dqn

    assert dqn.ROW_BYTES == 112
    assert (dqn.OFF_STATE, dqn.OFF_NEXT_STATE, dqn.OFF_ACTION, dqn.OFF_DONE, dqn.OFF_HAND, dqn.OFF_REWARD) == \
        (0, 48, 96, 97, 98, 100)
    T, D = 10, 37
    obs, actions, rewards = _random_transitions(T, D, 5)
    rows = dqn.pack_rows_host(obs, actions, rewards)
    assert rows.dtype == torch.uint8 and rows.shape == (T * D, 112)
    raw = rows.numpy().reshape(T, D, 112)
    assert np.array_equal(raw[..., 0:48].view(np.int8), obs[:-1].numpy())
    assert np.array_equal(raw[..., 48:96].view(np.int8), obs[1:].numpy())
    assert np.array_equal(raw[..., 96], actions.numpy())
    assert np.array_equal(raw[..., 97], np.arange(T)[:, None].repeat(D, 1) == T - 1)
    assert np.array_equal(raw[..., 98], (10 - np.arange(T))[:, None].repeat(D, 1))
    assert np.array_equal(np.ascontiguousarray(raw[..., 100:104]).view("<i4")[..., 0], rewards.numpy())
    assert not raw[..., 99].any() and not raw[..., 104:].any()
    # a 47-wide observation gets the zero pad byte
    assert torch.equal(dqn.pack_rows_host(obs[..., :47], actions, rewards), rows)
    s, s2, a, r, nd = dqn.unpack_rows_host(rows)
    assert s.dtype == s2.dtype == r.dtype == nd.dtype == torch.float32 and a.dtype == torch.int64
    assert torch.equal(s, obs[:-1].reshape(-1, 48).float()) and torch.equal(s2, obs[1:].reshape(-1, 48).float())
    assert torch.equal(a, actions.reshape(-1).long()) and torch.equal(r, rewards.reshape(-1).float())
    assert torch.equal(nd, (torch.arange(T * D) < (T - 1) * D).float())


def _q_with_ties(n, seed, width=104):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((n, width), generator=g)
    for i in range(0, n, 3):  # the row maximum twice: the lowest index counts
        a, b = sorted(int(x) for x in torch.randperm(104, generator=g)[:2])
        q[i, a] = q[i, b] = q[i, :104].max() + 1.0
    return q


@pytest.mark.parametrize("double", [False, True])
def test_bellman_target_host_is_the_dropins_calc_reward(double, monkeypatch):
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.dqn import bellman_target_host

    n = 97
    agent = (A.DDQNAgent if double else A.DQNVanilla)(history_length=8, gamma=0.97)
    q_local, q_target = _q_with_ties(n, 11), _q_with_ties(n, 12)
    monkeypatch.setattr(agent.dqn_net_local, "forward", lambda x: [q_local])
    if double:
        monkeypatch.setattr(agent.dqn_net_target, "forward", lambda x: [q_target])
        agent.step = 1  # no soft update inside _calc_reward (retrain_interval 4)
    g = torch.Generator().manual_seed(13)
    reward = -torch.randint(0, 40, (n,), generator=g).float()
    done = (torch.rand((n,), generator=g) < 0.3).to(torch.int64)
    assert 0 < int(done.sum()) < n
    want = agent._calc_reward(torch.zeros((n, 47)), reward, done)
    got = bellman_target_host(q_local, q_target if double else None, reward, 1.0 - done.float(), agent.gamma)
    assert got.dtype == torch.float32 and torch.equal(got, want.reshape(-1))
    # a padded head (stride 112): the pad columns never win
    wide = torch.full((n, 112), 1e9)
    wide[:, :104] = q_local
    wide_t = torch.zeros((n, 112))
    wide_t[:, :104] = q_target
    assert torch.equal(bellman_target_host(wide, wide_t if double else None, reward, 1.0 - done.float(), agent.gamma), got)
