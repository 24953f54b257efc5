"""GPU checks of the drop-in DQN agents (agents/dqn.py), golden F16.

DQNVanilla, DDQNAgent, DQN_PRBAgent and DDQN_PRBAgent in seeded training
GameSessions against three DrunkHamster (GPU env, host nets like the
reference's, the prioritised replay's tree on the device): with the default
epsilon schedule and with a constant epsilon of 0.3 (the greedy branch), every
move, epsilon, the results and the sampled PER tree indices equal the
reference's recordings; values, losses and final weights by the rule of
test_dropin_acer_agent_replays_reference_training_sessions.
"""
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SPEC = json.load(open(os.path.join(GOLDEN, "dqn_games.json")))


@pytest.mark.parametrize("si", range(len(SPEC["sessions"])))
def test_dropin_dqn_agents_replay_reference_training_sessions(si):
    from rl_6_nimmt import GameSession
    from rl_6_nimmt.agents import DQN_AGENTS, DrunkHamster

    sess = SPEC["sessions"][si]
    W = np.load(os.path.join(GOLDEN, "dqn_weights.npz"))
    cls = {c.__name__: c for c in DQN_AGENTS.values()}[sess["agent"]]
    torch.manual_seed(sess["seed"])
    kw = dict(sess["kwargs"])
    if sess["eps_const"] is not None:
        kw["eps_func"] = lambda episode, _c=sess["eps_const"]: _c
    agent = cls(**kw)
    agents = [agent] + [DrunkHamster() for _ in range(3)]
    agent.train()
    for k, v in agent.state_dict().items():
        assert np.array_equal(v.numpy(), W[f"s{si}_init_{k}"]), k
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
    # host fp32 math on another CPU: floats to 1e-3 (Adam amplifies rounding), moves identical
    assert np.allclose(got[:, 1], want[:, 1], rtol=0, atol=1e-3)
    assert len(losses) == len(W[f"s{si}_losses"])
    assert np.allclose(losses, W[f"s{si}_losses"], rtol=1e-3, atol=1e-4)
    if prb:
        assert per_idx == W[f"s{si}_per_idx"].tolist()
        assert agent.history.beta == sess["beta"] and len(agent.history) == sess["len"]
        # a sum of leaves (|q - target| + 0.01) ** 0.6 of the fp32 values the losses are made of: their tolerance
        assert agent.history.total_priority == pytest.approx(sess["total_priority"], rel=1e-3)
    for k, v in agent.state_dict().items():
        d = np.abs(v.detach().numpy() - W[f"s{si}_final_{k}"])
        assert np.mean(d <= 1e-4) >= 0.5 and d.max() <= 3e-3 * sess["games"], (k, d.max())
