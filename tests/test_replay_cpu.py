"""CPU checks of the prioritised replay's contract and the DQN drop-ins' host side.

`PerModel` is a numpy model of what include/sechs.h promises for sn_per_*:
the reference's heap layout for any capacity, every internal node recomputed
pairwise from the leaves after store / update, the reference's descent in its
operation order, and its two quirks (len = stores - wraps; the weights'
minimum over the first min(len, capacity) leaves).  It must reproduce the
reference's recorded traces (golden F15, tools/gen_fixtures.py): sampled
indices exactly -- the reference's incremental tree drifts ~1e-14 from the
pairwise one and the recorded descents stay >= 1e-10 x total clear of every
threshold -- and weights, priorities and tree snapshots to 1e-12.  The GPU
tests (test_gpu_replay.py) hold the kernels to the same model.
"""
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN


class PerModel:
    def __init__(self, capacity):
        self.cap = capacity
        self.tree = np.zeros(2 * capacity - 1)
        self.pointer = self.num_items = 0
        self.absolute_error_upper, self.epsilon, self.alpha, self.beta, self.beta_increment = 1.0, 0.01, 0.6, 0.4, 0.001

    def rebuild(self):
        t = self.tree
        for i in range(self.cap - 2, -1, -1):
            t[i] = t[2 * i + 1] + t[2 * i + 2]

    def store(self, m=1):
        assert 1 <= m <= self.cap
        top = self.tree[self.cap - 1:].max()
        top = 1.0 if top == 0 else top
        slots = (self.pointer + np.arange(m)) % self.cap
        self.tree[self.cap - 1 + slots] = top
        self.rebuild()
        wraps = (self.pointer + m) // self.cap
        self.pointer = (self.pointer + m) % self.cap
        self.num_items += m - wraps
        return slots

    def descend(self, v):
        node = 0
        while 2 * node + 1 < len(self.tree):
            left = self.tree[2 * node + 1]
            if v <= left:
                node = 2 * node + 1
            else:
                v -= left
                node = 2 * node + 2
        return node

    def sample(self, n, u):
        total = self.tree[0]
        seg = total / n
        self.beta = min(1.0, self.beta + self.beta_increment)
        lo = self.cap - 1
        min_prob = self.tree[lo: lo + min(self.num_items, self.cap)].min() / total
        idx = np.array([self.descend(seg * i + u[i] * seg) for i in range(n)], dtype=np.int64)
        prio = self.tree[idx]
        return idx, prio, np.power((prio / total) / min_prob, -self.beta)

    def update(self, idx, err, epsilon=None, upper=None, alpha=None):
        epsilon = self.epsilon if epsilon is None else epsilon
        upper = self.absolute_error_upper if upper is None else upper
        alpha = self.alpha if alpha is None else alpha
        ps = np.minimum(np.asarray(err, dtype=np.float64) + epsilon, upper) ** alpha
        for i, p in zip(idx, ps):  # sequential: of a repeated index the last one stays
            if self.cap - 1 <= i <= 2 * self.cap - 2:
                self.tree[i] = p
        self.rebuild()


def per_traces():
    """golden F15 as [{capacity, nstore, n, rounds: [{u, errors, idx, weights, priorities, beta, len}], tree: {round:
    nodes}, ...}]: the shapes from per_traces.json, the arrays from per_traces.npz"""
    traces = json.load(open(os.path.join(GOLDEN, "per_traces.json")))["traces"]
    arrays = np.load(os.path.join(GOLDEN, "per_traces.npz"))
    for ti, tr in enumerate(traces):
        f = {k: arrays[f"t{ti}_{k}"] for k in ("u", "errors", "weights", "priorities", "beta", "tree", "idx", "len")}
        tr["rounds"] = [{"len": int(f["len"][r]), "beta": float(f["beta"][r]),
                         **{k: f[k][r].tolist() for k in ("idx", "u", "errors", "weights", "priorities")}}
                        for r in range(tr["rounds"])]
        tr["tree"] = {str(r): f["tree"][i] for i, r in enumerate(tr["snapshots"])}
    return traces


@pytest.mark.parametrize("ti", range(4))
def test_model_reproduces_the_reference_traces(ti):
    tr = per_traces()[ti]
    m = PerModel(tr["capacity"])
    for _ in range(tr["nstore"]):
        m.store()
    repeats = 0
    for r, rd in enumerate(tr["rounds"]):
        m.store()
        idx, prio, w = m.sample(tr["n"], rd["u"])
        assert idx.tolist() == rd["idx"], (ti, r)
        assert np.allclose(prio, rd["priorities"], rtol=1e-12, atol=0), (ti, r)
        assert np.allclose(w, rd["weights"], rtol=1e-12, atol=0), (ti, r)
        assert m.beta == rd["beta"] and m.num_items == rd["len"], (ti, r)
        repeats += len(set(rd["idx"])) < tr["n"]
        m.update(idx, rd["errors"])
        if str(r) in tr["tree"]:
            assert np.allclose(m.tree, tr["tree"][str(r)], rtol=1e-12, atol=0), (ti, r)
    assert repeats == tr["rounds_with_repeats"] >= 1
    assert tr["min_margin"] >= 1e-10
    assert str(len(tr["rounds"]) - 1) in tr["tree"]


def test_model_keeps_the_reference_quirks():
    m = PerModel(5)
    for _ in range(43):
        m.store()
    assert m.num_items == 35 and m.pointer == 3  # stores - wraps, past the capacity
    m = PerModel(5)
    for _ in range(5):
        m.store()
    assert m.num_items == 4  # the wrapping store did not count ...
    m.update([8], [0.0])  # ... so the last leaf (tiny now) is outside the weights' minimum
    idx, prio, w = m.sample(4, [0.5] * 4)
    assert np.allclose(w, 1.0)


def test_dqn_history_ring_indexing():
    from rl_6_nimmt.utils.replay_buffer import History

    h = History(max_length=4)
    lens = []
    for k in range(10):
        h.store(k=k)
        lens.append(len(h))
    # the pointer while filling, max_length at the store that wraps, the pointer again afterwards
    assert lens == [1, 2, 3, 4, 1, 2, 3, 4, 1, 2]
    assert [m["k"] for m in h.memories] == [8, 9, 6, 7]
    random.seed(3)
    want = random.sample(range(2), k=2)
    random.seed(3)
    idx, weights, batch = h.sample(2)
    assert idx == want and weights is None and batch == {"k": [h.memories[i]["k"] for i in want]}
    assert h.rollout() == {"k": [8, 9]} and h.rollout(1) == {"k": [9]}
    h.store(k=10)
    h.store(k=11)
    assert len(h) == 4 and h.rollout(2) == {"k": [10, 11]}  # full again: slots 2, 3
    u = History()
    for k in range(200):
        u.store(k=k)
    assert len(u) == 200 and u.rollout(1) == {"k": [199]}


def test_priority_replay_needs_a_length():
    from rl_6_nimmt.utils.replay_buffer import PriorityReplayBuffer

    with pytest.raises(ValueError):
        PriorityReplayBuffer()


def test_construction_touches_no_gpu():
    from rl_6_nimmt.agents import DDQN_PRBAgent, DDQNAgent, DQN_PRBAgent, DQNVanilla
    from rl_6_nimmt.replay import DevicePER
    from rl_6_nimmt.utils.replay_buffer import History, PriorityReplayBuffer

    was = torch.cuda.is_initialized()
    per = DevicePER(100, row_bytes=112)
    assert per._h is None and len(per) == 0 and per.pointer == 0
    assert (per.alpha, per.beta, per.beta_increment, per.epsilon, per.absolute_error_upper) == (0.6, 0.4, 0.001, 0.01, 1.0)
    for bad in ((1, 0), (8, 8), (8, -16)):
        with pytest.raises(ValueError):
            DevicePER(*bad)
    for cls in (DQNVanilla, DDQNAgent, DQN_PRBAgent, DDQN_PRBAgent):
        a = cls(history_length=32, minibatch=4)
        a.train()
        want = PriorityReplayBuffer if "PRB" in cls.__name__ else History
        assert type(a.history) is want and len(a.history) == 0 and a.history.max_length == 32
        assert a.eps == 1.0 and a.minibatch == 4
        assert hasattr(a, "dqn_net_target") == ("DDQN" in cls.__name__)
        if "PRB" in cls.__name__:
            assert a.history.per._h is None
    assert torch.cuda.is_initialized() == was


def test_dqn_agents_are_registered_beside_the_league_registry():
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.league import agent_kind

    assert A.DQN_AGENTS == {"dqn": A.DQNVanilla, "ddqn": A.DDQNAgent, "dqn_prb": A.DQN_PRBAgent,
                            "ddqn_prb": A.DDQN_PRBAgent}
    assert (A.DQN, A.DDQN, A.DQN_PRB, A.DDQN_PRB) == ("dqn", "ddqn", "dqn_prb", "ddqn_prb")
    assert sorted(A.AGENTS) == ["acer", "mcts", "pmcs", "puct", "random", "reinforce"]
    with pytest.raises(NotImplementedError):
        agent_kind(A.DQNVanilla(history_length=8))


def test_epsilon_schedule_and_exploring_draws():
    from rl_6_nimmt.agents import DQNVanilla
    from rl_6_nimmt.agents.dqn import eps_func_decay

    assert eps_func_decay(0) == 1.0 and eps_func_decay(100) == pytest.approx(np.exp(-0.25)) and eps_func_decay(5000) == 0.05
    torch.manual_seed(0)
    a = DQNVanilla(history_length=8)
    a.train()  # eps 1: always exploring
    legal = [3, 17, 50]
    random.seed(1)
    random.random()
    random.choice(range(104))  # one draw over all actions first, then one over the legal ones
    want = random.choice(legal)
    random.seed(1)
    act, info = a(torch.zeros(47), legal_actions=legal)
    assert act == want and info == {"value": -1, "eps": 1.0}
    a.eps = 0.0  # greedy: the best legal card, whatever the illegal ones score
    with torch.no_grad():
        q = a.dqn_net_local(torch.zeros(47))[0].numpy()
    act, info = a(torch.zeros(47), legal_actions=legal)
    assert act == legal[int(np.argmax(q[legal]))] and info["value"] == pytest.approx(q[legal].max())


def test_host_tree_indices_are_checked():
    from rl_6_nimmt.utils.replay_buffer import PriorityReplayBuffer

    buf = PriorityReplayBuffer(8)  # leaves 7 .. 14
    for bad in ([6], [15], [7, -1]):
        with pytest.raises(ValueError):
            buf.batch_update(np.array(bad), np.full(len(bad), 0.5))
        with pytest.raises(ValueError):
            buf.batch_update(bad, torch.full((len(bad),), 0.5))
    assert buf.per._h is None
