"""CPU checks of the duelling and n-step DQN variants (utils/nets.py,
agents/dqn.py, the torch models of rl_6_nimmt/dqn.py): no GPU, no kernel call.

* DuellingDQNNet loads the reference's state_dict (golden F17) and returns
  V + (A - mean A) of its own heads;
* the five classes: registry names, bases in the reference's order,
  engine_kind "dqn"; DQN_AGENTS keeps its four names; construction leaves the
  GPU alone;
* pack_rows_nstep_host -- the model sn_dqn_pack_nstep is held to on the GPU --
  reproduces the transitions the reference's D3QN_PRB_NStep stored for the
  recorded learn calls (F17), the float64 return exactly, and agrees with a
  direct transcription of DQN_NStep_Agent._store / _finish_episode on
  synthetic episodes; n = 1 is pack_rows_host but for the n-step bytes;
* unpack_rows_nstep_host inverts the pack.
"""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLDEN

SPEC = json.load(open(os.path.join(GOLDEN, "dqn_variant_games.json")))
VARIANT_NAMES = {"duelling_dqn": "DuellingDQNAgent", "duelling_ddqn": "DuellingDDQNAgent",
                 "duelling_ddqn_prb": "DuellingDDQN_PRBAgent", "dqn_nstep": "DQN_NStep_Agent",
                 "d3qn_prb_nstep": "D3QN_PRB_NStep"}


def test_fixture_holds_the_eight_sessions():
    got = [(s["agent"], s["eps_const"], s["kwargs"].get("n_steps", 1)) for s in SPEC["sessions"]]
    want = []
    for name, n in (("DuellingDQNAgent", 1), ("DuellingDDQNAgent", 1), ("DuellingDDQN_PRBAgent", 1),
                    ("D3QN_PRB_NStep", 3)):
        want += [(name, None, n), (name, 0.3, n)]
    assert got == want


def test_duelling_net_loads_the_reference_state_dict_and_combines_its_heads():
    from rl_6_nimmt.utils.nets import DuellingDQNNet, MultiHeadedMLP

    W = np.load(os.path.join(GOLDEN, "dqn_variant_weights.npz"))
    net = DuellingDQNNet(47, hidden_sizes=(64,), out_size=104, activation=nn.ReLU())
    assert isinstance(net.mlp, MultiHeadedMLP)
    assert sorted(net.state_dict()) == sorted(
        ["mlp.latent_net.0.weight", "mlp.latent_net.0.bias", "mlp.head_nets.0.0.weight", "mlp.head_nets.0.0.bias",
         "mlp.head_nets.1.0.weight", "mlp.head_nets.1.0.bias"])
    pre = "s0_init_dqn_net_local."
    sd = {k[len(pre):]: torch.from_numpy(W[k]) for k in W.files if k.startswith(pre)}
    net.load_state_dict(sd, strict=True)
    assert net.mlp.head_nets[0][0].out_features == 1 and net.mlp.head_nets[1][0].out_features == 104
    x = torch.randint(-1, 104, (9, 47), generator=torch.Generator().manual_seed(1)).float()
    with torch.no_grad():
        (q,) = net(x)
        V, A = net.mlp(x)
    assert q.shape == (9, 104) and V.shape == (9, 1)
    assert torch.equal(q, V + (A - A.mean(dim=-1, keepdim=True)))
    from rl_6_nimmt.dqn import duelling_q_host

    assert torch.equal(duelling_q_host(V, A), q)
    with pytest.raises(NotImplementedError):  # the noisy layers stay out
        DuellingDQNNet(47, (64,), 104, nn.ReLU(), linear=nn.Bilinear)


def test_class_layout_registry_and_engine_kind():
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.agents import dqn as M
    from rl_6_nimmt.league import engine_kind
    from rl_6_nimmt.utils.nets import DuellingDQNNet, MultiHeadedMLP
    from rl_6_nimmt.utils.replay_buffer import History, PriorityReplayBuffer

    assert {k: v.__name__ for k, v in A.DQN_VARIANT_AGENTS.items()} == VARIANT_NAMES
    assert (A.DUELLING_DQN, A.DUELLING_DDQN, A.DUELLING_DDQN_PRB, A.DQN_NSTEP, A.D3QN_PRB_NSTEP) == \
        ("duelling_dqn", "duelling_ddqn", "duelling_ddqn_prb", "dqn_nstep", "d3qn_prb_nstep")
    assert sorted(A.DQN_AGENTS) == ["ddqn", "ddqn_prb", "dqn", "dqn_prb"]
    assert not set(A.DQN_VARIANT_AGENTS) & (set(A.DQN_AGENTS) | set(A.AGENTS))
    assert M.DuellingDQNAgent.__bases__ == (M.DQNVanilla,)
    assert M.DuellingDDQNAgent.__bases__ == (M.DDQNAgent,)
    assert M.DQN_NStep_Agent.__bases__ == (M.DQNVanilla,)
    assert M.DuellingDDQN_PRBAgent.__bases__ == (M.DQN_PRBAgent, M.DuellingDDQNAgent)
    assert M.D3QN_PRB_NStep.__bases__ == (M.DQN_NStep_Agent, M.DuellingDDQN_PRBAgent)
    assert M.D3QN_PRB_NStep.__mro__[:7] == (M.D3QN_PRB_NStep, M.DQN_NStep_Agent, M.DuellingDDQN_PRBAgent,
                                            M.DQN_PRBAgent, M.DuellingDDQNAgent, M.DDQNAgent, M.DQNVanilla)
    was = torch.cuda.is_initialized()
    for name, cls in A.DQN_VARIANT_AGENTS.items():
        a = cls(history_length=32, minibatch=4, n_steps=3 if "nstep" in name else 1)
        a.train()
        assert engine_kind(a) == "dqn", name
        duel = name != "dqn_nstep"
        assert type(a.dqn_net_local) is (DuellingDQNNet if duel else MultiHeadedMLP)
        assert hasattr(a, "dqn_net_target") == ("ddqn" in name or "d3qn" in name)
        if hasattr(a, "dqn_net_target"):
            assert type(a.dqn_net_target) is DuellingDQNNet
            assert all(torch.equal(p, q) for p, q in zip(a.dqn_net_local.parameters(), a.dqn_net_target.parameters()))
        assert type(a.history) is (PriorityReplayBuffer if "prb" in name else History)
        assert a.n_steps == (3 if "nstep" in name else 1) and hasattr(a, "n_step_buffer") == ("nstep" in name)
        if "prb" in name:
            assert a.history.per._h is None
    assert torch.cuda.is_initialized() == was


# ---------------------------------------------------------------- the n-step row model
def _reference_rows(calls, n, gamma):
    """DQN_NStep_Agent._store / _finish_episode (reference agents/dqn.py:270-301), transcribed: the stored
    experiences of one episode's learn calls, in store order"""
    buf, stored = [], []
    for call in calls:
        kwargs = dict(call)
        buf.append(kwargs)
        if len(buf) >= n:
            R = sum([buf[i]["reward"] * (gamma ** i) for i in range(n)])
            exp = buf.pop(0)
            exp["reward"] = R
            exp["next_state"] = kwargs["next_state"]
            stored.append(exp)
        if call["done"]:
            if len(buf) == 0:
                continue
            last = buf[-1]
            while len(buf) > 0:
                R = sum([buf[i]["reward"] * (gamma ** i) for i in range(len(buf))])
                exp = buf.pop(0)
                exp["reward"] = R
                exp["next_state"] = last["next_state"]
                exp["done"] = True
                stored.append(exp)
    return stored


def _calls_to_arrays(calls):
    """learn calls of one episode, one decider -> obs [T+1, 1, 47], actions [T, 1], rewards_seen [T, 1]"""
    T = len(calls)
    for t in range(T - 1):
        assert calls[t]["next_state"] == calls[t + 1]["state"]
    assert [c["done"] for c in calls] == [False] * (T - 1) + [True]
    obs = torch.tensor([c["state"] for c in calls] + [calls[-1]["next_state"]], dtype=torch.int8)[:, None, :]
    actions = torch.tensor([c["action"] for c in calls], dtype=torch.int32)[:, None]
    rewards = [c["reward"] for c in calls]
    assert all(float(r).is_integer() for r in rewards)
    return obs, actions, torch.tensor([int(r) for r in rewards], dtype=torch.int32)[:, None]


def _assert_rows_are(rows, returns, stored, T):
    """rows [T, 112] uint8 and float64 returns [T] of one decider against stored experience dicts"""
    from rl_6_nimmt import dqn

    assert len(stored) == T and rows.shape == (T, 112)
    raw = rows.numpy()
    for s, exp in enumerate(stored):
        assert raw[s, 0:47].view(np.int8).tolist() == [int(v) for v in exp["state"]], s
        assert raw[s, 48:95].view(np.int8).tolist() == [int(v) for v in exp["next_state"]], s
        assert raw[s, 47] == 0 and raw[s, 95] == 0
        assert raw[s, dqn.OFF_ACTION] == exp["action"] and bool(raw[s, dqn.OFF_DONE]) == bool(exp["done"]), s
        assert isinstance(exp["reward"], float) and float(returns[s]) == exp["reward"], s  # float64, bit for bit
        f32 = np.ascontiguousarray(raw[s, 104:108]).view("<f4")[0]
        assert f32 == np.float32(exp["reward"]), s
        assert not raw[s, 108:].any()


@pytest.mark.parametrize("si", [i for i, s in enumerate(SPEC["sessions"]) if "learn_calls" in s])
def test_nstep_row_model_reproduces_the_references_stored_transitions(si):
    from rl_6_nimmt import dqn

    sess = SPEC["sessions"][si]
    n, gamma = sess["kwargs"]["n_steps"], 0.99  # the agents' default gamma
    assert n == 3 and len(sess["learn_calls"]) == len(sess["stored"]) == 2
    assert any(c["reward"] != 0 for calls in sess["learn_calls"] for c in calls)
    for calls, stored in zip(sess["learn_calls"], sess["stored"]):
        T = len(calls)
        assert T == 10
        obs, actions, rewards = _calls_to_arrays(calls)
        rows = dqn.pack_rows_nstep_host(obs, actions, rewards, n, gamma)
        returns = dqn.nstep_returns_host(rewards, n, gamma)[:, 0]
        _assert_rows_are(rows, returns, stored, T)
        # and the transcription used below is the reference's, on its own recordings
        mine = _reference_rows(calls, n, gamma)
        assert [(e["reward"], e["done"], e["action"], e["state"], e["next_state"]) for e in mine] == \
            [(e["reward"], e["done"], e["action"], e["state"], e["next_state"]) for e in stored]
        # quirk kept: the row n steps before the end points at the terminal observation, done False
        assert stored[T - n]["next_state"] == calls[-1]["next_state"] and stored[T - n]["done"] is False


def _synthetic(T, D, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randint(-1, 104, (T + 1, D, 48), generator=g).to(torch.int8)
    obs[..., 47] = 0
    for t in range(T + 1):  # hands of T - t cards, -1 padded
        obs[t, :, T - t:10] = -1
        obs[t, :, : T - t].clamp_(min=0)
    actions = torch.randint(0, 104, (T, D), generator=g).to(torch.int32)
    rewards = -torch.randint(0, 71, (T, D), generator=g).to(torch.int32)
    rewards[0] = 0
    return obs, actions, rewards


@pytest.mark.parametrize("T", [10, 4])
@pytest.mark.parametrize("n", [1, 2, 3, 9, 10, 11, 15])
@pytest.mark.parametrize("gamma", [0.99, 0.5])
def test_nstep_row_model_is_the_references_two_loops(T, n, gamma):
    from rl_6_nimmt import dqn

    D = 3
    obs, actions, rewards = _synthetic(T, D, 100 * T + n)
    rows = dqn.pack_rows_nstep_host(obs, actions, rewards, n, gamma).reshape(T, D, 112)
    returns = dqn.nstep_returns_host(rewards, n, gamma)
    assert returns.dtype == torch.float64
    for d in range(D):
        calls = [{"state": obs[t, d, :47].tolist(), "reward": int(rewards[t, d]), "action": int(actions[t, d]),
                  "next_state": obs[t + 1, d, :47].tolist(), "done": t == T - 1} for t in range(T)]
        stored = _reference_rows(calls, n, gamma)
        for e in stored:
            e["reward"] = float(e["reward"])  # n = 1: int * 1.0 is a float already; kept for clarity
        _assert_rows_are(rows[:, d], returns[:, d], stored, T)
    raw = rows.numpy()
    assert np.array_equal(raw[..., dqn.OFF_TERMS], np.minimum(n, T - np.arange(T))[:, None].repeat(D, 1))
    assert np.array_equal(raw[..., dqn.OFF_HAND], (T - np.arange(T))[:, None].repeat(D, 1))
    assert np.array_equal(np.ascontiguousarray(raw[..., 100:104]).view("<i4")[..., 0], rewards.numpy())
    if n == 1:  # today's rows, but for the n-step bytes
        plain = dqn.pack_rows_host(obs, actions, rewards).reshape(T, D, 112).numpy()
        keep = np.ones(112, dtype=bool)
        keep[[99, 104, 105, 106, 107]] = False
        assert np.array_equal(raw[..., keep], plain[..., keep])
        assert (raw[..., 99] == 1).all() and not plain[..., 99].any() and not plain[..., 104:108].any()
        assert np.array_equal(np.ascontiguousarray(raw[..., 104:108]).view("<f4")[..., 0], rewards.numpy().astype("f4"))


def test_nstep_unpack_inverts_the_pack():
    from rl_6_nimmt import dqn

    T, D, n, gamma = 10, 37, 3, 0.99
    obs, actions, rewards = _synthetic(T, D, 7)
    rows = dqn.pack_rows_nstep_host(obs, actions, rewards, n, gamma)
    assert torch.equal(dqn.pack_rows_nstep_host(obs[..., :47], actions, rewards, n, gamma), rows)  # 47-wide: padded
    s, s2, a, r, nd = dqn.unpack_rows_nstep_host(rows)
    assert s.dtype == s2.dtype == r.dtype == nd.dtype == torch.float32 and a.dtype == torch.int64
    nxt = torch.clamp(torch.arange(T) + n, max=T)
    assert torch.equal(s, obs[:-1].reshape(-1, 48).float()) and torch.equal(s2, obs[nxt].reshape(-1, 48).float())
    assert torch.equal(a, actions.reshape(-1).long())
    assert torch.equal(r, dqn.nstep_returns_host(rewards, n, gamma).float().reshape(-1))
    assert torch.equal(nd, (torch.arange(T * D) < (T - n + 1) * D).float())
    # the one-step reader still sees r_s in the same rows
    assert torch.equal(dqn.unpack_rows_host(rows)[3], rewards.reshape(-1).float())
    assert dqn.gamma_powers(gamma) == [gamma ** i for i in range(10)] and (dqn.OFF_TERMS, dqn.OFF_RETURN) == (99, 104)
