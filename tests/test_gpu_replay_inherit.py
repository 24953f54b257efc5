"""GPU checks of cloning the device prioritised replay (k_per_inherit behind
sn_per_inherit / sn_per_import, csrc/sechs_replay.hip) and of what
is built on it: DevicePER.inherit / clone / pickling, deep copies and
torch.save of the drop-in *_PRB agents, BatchedDQN.inherit in the league.

The kernel is held to replay.inherit_host: a DevicePER and the numpy model
(test_replay_inherit_cpu.build_parent) go through the same history, the
priorities written as given doubles (alpha 1, epsilon 0, no clip: no device pow
in the way), so every comparison of trees here is bit for bit -- the internal
nodes are the same pairwise sums on both sides.
"""
import copy
import ctypes
import io
import pickle
import random

import numpy as np
import pytest
import torch

from test_replay_cpu import PerModel
from test_replay_inherit_cpu import STATES, build_parent

pytestmark = pytest.mark.gpu

INF = float("inf")


def _tag_rows(first, m, row_bytes, device="cuda"):
    """m rows whose every int32 word is the row's store number first, first + 1, ..."""
    return torch.arange(first, first + m, dtype=torch.int32, device=device)[:, None].repeat(1, row_bytes // 4)


class _Mirror:
    """build_parent's stores and update, repeated on a DevicePER"""

    def __init__(self, per):
        self.per = per

    def store(self, m, first_tag):
        if self.per.row_bytes:
            self.per.store(_tag_rows(first_tag, m, self.per.row_bytes))
        else:
            self.per.store(count=m)

    def update(self, idx, prio):
        self.per.update(idx, prio, epsilon=0.0, upper=INF, alpha=1.0)


def _export(per):
    """(tree, rows or None, pointer, len) on the host"""
    rows = None
    if per.row_bytes:
        rows = per.gather(torch.arange(per.capacity, dtype=torch.int32, device="cuda")).cpu()
    return per.tree().cpu(), rows, per.pointer, len(per)


def _inherited(state, cap):
    """what a replay of `cap` slots holds after inheriting the exported `state`, by the host model"""
    from rl_6_nimmt.replay import inherit_host

    tree, rows, pointer, num_items = state
    cap_p = (tree.numel() + 1) // 2
    leaves, rows, pointer, num_items = inherit_host(tree[cap_p - 1:], rows, pointer, num_items, cap)
    m = PerModel(cap)
    m.tree[cap - 1:] = leaves.numpy()
    m.rebuild()
    return torch.from_numpy(m.tree), rows, pointer, num_items


def _same(a, b):
    assert torch.equal(a[0], b[0])
    assert (a[1] is None and b[1] is None) or torch.equal(a[1], b[1])
    assert a[2:] == b[2:], (a[2:], b[2:])


def _parent(cap, state, row_bytes):
    from rl_6_nimmt.replay import DevicePER

    per = DevicePER(cap, row_bytes=row_bytes)
    model = build_parent(cap, state, also=_Mirror(per))
    return per, model


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("row_bytes", [0, 16, 112])
@pytest.mark.parametrize("cap_c", [2, 5, 8, 4099])
@pytest.mark.parametrize("cap_p", [2, 5, 8, 4099])
def test_inherit_equals_the_host_model(cap_p, cap_c, row_bytes, state):
    from rl_6_nimmt.replay import DevicePER

    parent, model = _parent(cap_p, state, row_bytes)
    before = _export(parent)
    assert torch.equal(before[0], torch.from_numpy(model.tree)) and before[2:] == (model.pointer, model.num_items)
    if row_bytes:
        want = np.repeat(model.tags[:, None], row_bytes // 4, axis=1).astype(np.int32)
        assert np.array_equal(before[1].view(torch.int32).numpy(), want)
    child = DevicePER(cap_c, row_bytes=row_bytes)  # dirtied: stores of its own, one leaf moved
    m = min(cap_c, 3)
    child.store(torch.full((m, row_bytes), 0xEE, dtype=torch.uint8, device="cuda") if row_bytes else None, count=m)
    child.update([cap_c - 1], [7.5], epsilon=0.0, upper=INF, alpha=1.0)
    child.beta = 0.9
    parent.beta = 0.61
    child.inherit(parent)
    _same(_export(child), _inherited(before, cap_c))
    _same(_export(parent), before)
    assert child.beta == 0.61 and child.capacity == cap_c
    if cap_p != cap_c and state != "empty":  # re-homed: the newest store is the last kept slot
        h = min(model.stores, cap_p, cap_c)
        assert child.pointer == h % cap_c
        if row_bytes:
            got = child.gather(torch.tensor([h - 1], dtype=torch.int32)).view(torch.int32).cpu()
            assert bool((got == model.stores).all())


def _twins_answer_alike(a, b, seed):
    """same uniforms -> same samples; a following store lands alike; then an update on one leaves the other alone"""
    rng = np.random.RandomState(seed)
    n, cap = 7, a.capacity
    assert a is not b and a._h is not b._h and (a.pointer, len(a), a.beta) == (b.pointer, len(b), b.beta)
    u = rng.random_sample(n)
    sa, sb = a.sample(n, u), b.sample(n, u)
    for x, y in zip(sa, sb):
        assert (x is None and y is None) or torch.equal(x, y)
    assert a.beta == b.beta
    slot = a.pointer
    for p in (a, b):
        p.store(_tag_rows(1000, 1, p.row_bytes) if p.row_bytes else None, count=1)
    _same(_export(a), _export(b))
    assert a.pointer == (slot + 1) % cap
    assert float(a.tree()[cap - 1 + slot]) == float(a.tree()[cap - 1:].max())  # entered at the maximum leaf
    ta, tb = _export(a), _export(b)
    b.update([cap - 1], [0.25 / seed], epsilon=0.0, upper=INF, alpha=1.0)  # a value no leaf holds yet
    _same(_export(a), ta)
    assert not torch.equal(b.tree().cpu(), tb[0])
    tb = _export(b)
    a.update([2 * cap - 2], [0.125 / seed], epsilon=0.0, upper=INF, alpha=1.0)
    _same(_export(b), tb)
    assert not torch.equal(a.tree().cpu(), ta[0])


@pytest.mark.parametrize("cap,row_bytes", [(5, 112), (4099, 16), (8, 0)])
def test_verbatim_clones_answer_alike_and_part_ways(cap, row_bytes):
    parent, model = _parent(cap, "wrapped", row_bytes)
    parent.sample(3)  # beta has moved
    clone = copy.deepcopy(parent)
    assert (clone.capacity, clone.row_bytes, clone.device) == (parent.capacity, parent.row_bytes, parent.device)
    assert len(clone) == model.num_items > cap - 1  # the reference's count past the capacity is copied as it is
    _twins_answer_alike(parent, clone, cap)
    _twins_answer_alike(clone.clone(), clone, cap + 1)


@pytest.mark.parametrize("how", ["pickle", "torch.save"])
def test_pickle_round_trip_of_a_stored_into_replay(how):
    parent, model = _parent(5, "wrapped", 112)
    for _ in range(4):
        parent.sample(3)
    assert parent.beta == pytest.approx(0.404)
    if how == "pickle":
        loaded = pickle.loads(pickle.dumps(parent))
    else:
        buf = io.BytesIO()
        torch.save(parent, buf)
        buf.seek(0)
        loaded = torch.load(buf, weights_only=False)
    assert loaded._h is None and loaded.beta == parent.beta  # nothing touched yet: the kept counters answer
    assert (loaded.pointer, len(loaded)) == (model.pointer, model.num_items)
    again = pickle.loads(pickle.dumps(loaded))  # a state still on the host is carried on as it is
    _same(_export(loaded), _export(parent))
    assert loaded._h is not None and loaded._saved is None
    _twins_answer_alike(parent, loaded, 5)
    tree, _, pointer, num_items = _export(again)
    assert torch.equal(tree, torch.from_numpy(model.tree)) and (pointer, num_items) == (model.pointer, model.num_items)


def test_error_paths_launch_nothing():
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.replay import DevicePER

    parent, _ = _parent(5, "partly", 16)
    before = _export(parent)
    with pytest.raises(ValueError):
        DevicePER(5, row_bytes=112).inherit(parent)
    with pytest.raises(ValueError):
        parent.inherit(parent)
    L, st = nat.lib(), parent._stream()
    assert L.sn_per_inherit(parent._h, parent._h, st) == nat.SN_EINVAL
    assert L.sn_per_inherit(parent._h, None, st) == nat.SN_EINVAL and L.sn_per_inherit(None, parent._h, st) == nat.SN_EINVAL
    other = DevicePER(8, row_bytes=0)
    other.store()
    assert L.sn_per_inherit(other._h, parent._h, st) == nat.SN_EINVAL  # row_bytes differ
    leaves = torch.ones(5, dtype=torch.float64, device="cuda")
    rows = torch.zeros((5, 16), dtype=torch.uint8, device="cuda")
    P = nat.ptr
    assert L.sn_per_import(parent._h, P(leaves), P(rows), 5, 3, st) == nat.SN_EINVAL   # pointer == capacity
    assert L.sn_per_import(parent._h, P(leaves), P(rows), -1, 3, st) == nat.SN_EINVAL
    assert L.sn_per_import(parent._h, P(leaves), P(rows), 0, -1, st) == nat.SN_EINVAL
    assert L.sn_per_import(parent._h, P(leaves), None, 0, 3, st) == nat.SN_EINVAL      # rows missing
    assert L.sn_per_import(other._h, P(leaves), P(rows), 0, 3, st) == nat.SN_EINVAL    # rows for a replay without
    assert L.sn_per_import(parent._h, P(leaves), ctypes.c_void_p(rows.data_ptr() + 8), 0, 3, st) == nat.SN_EINVAL  # misaligned
    assert L.sn_per_import(parent._h, None, P(rows), 0, 3, st) == nat.SN_EINVAL
    _same(_export(parent), before)
    # the accepted call: the given leaves and rows, slot for slot, under the given counters
    assert L.sn_per_import(parent._h, P(leaves), P(rows), 4, 9, st) == nat.SN_OK
    tree, got, pointer, num_items = _export(parent)
    want = PerModel(5)
    want.tree[4:] = 1.0
    want.rebuild()
    assert torch.equal(tree, torch.from_numpy(want.tree)) and not got.any() and (pointer, num_items) == (4, 9)
    # a parent nothing was stored into empties a child that held something
    other.inherit(DevicePER(8, row_bytes=0))
    assert (other.pointer, len(other)) == (0, 0) and not other.tree().any()


# ---------------------------------------------------------------- the drop-in agents
def _trained_prb_agent():
    from rl_6_nimmt.agents import DQN_PRBAgent

    torch.manual_seed(5)
    agent = DQN_PRBAgent(history_length=8, minibatch=2)
    agent.train()
    for k in range(11):  # wraps: slots 0..2 hold stores 8..10
        agent.history.store(state=torch.full((47,), float(k)), reward=k, action=k % 104,
                            next_state=torch.full((47,), k + 1.0), done=(k == 10))
    random.seed(11)
    idx, _, _ = agent.history.sample(2)
    agent.history.batch_update(idx, torch.tensor([0.3, 0.7]))
    return agent


def _histories_answer_alike(a, b):
    assert a is not b and a.per is not b.per and a.data is not b.data
    assert (len(a), a.per.pointer, a.beta) == (len(b), b.per.pointer, b.beta) and a.total_priority == b.total_priority
    random.seed(3)
    ia, wa, ma = a.sample(4)
    random.seed(3)
    ib, wb, mb = b.sample(4)
    assert np.array_equal(ia, ib) and np.array_equal(wa, wb) and ma.keys() == mb.keys()
    for k in ma:
        assert all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(ma[k], mb[k])), k


def test_a_trained_prb_agent_deep_copies_with_its_replay():
    from rl_6_nimmt.tournament import Tournament

    agent = _trained_prb_agent()
    assert len(agent.history) == 10 and agent.history.per.pointer == 3
    clone = copy.deepcopy(agent)
    _histories_answer_alike(agent.history, clone.history)
    for p, q in zip(agent.dqn_net_local.parameters(), clone.dqn_net_local.parameters()):
        assert torch.equal(p, q) and p is not q
    t = Tournament()
    t.add_player("q", agent)
    t.copy_player("q", "q_c")
    assert t.agents["q_c"] is not agent and t.agents["q_c"].__name__ == "q_c"
    _histories_answer_alike(agent.history, t.agents["q_c"].history)
    clone.history.store(state=torch.zeros(47), reward=0, action=0, next_state=torch.zeros(47), done=False)
    assert len(clone.history) == 11 and len(agent.history) == 10  # from here on each its own


def test_a_trained_prb_agent_is_saved_and_loaded_with_its_replay():
    agent = _trained_prb_agent()
    buf = io.BytesIO()
    torch.save(agent, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    assert loaded.history.per._h is None and len(loaded.history) == 10 and loaded.step == agent.step
    _histories_answer_alike(agent.history, loaded.history)


# ---------------------------------------------------------------- the league
def test_league_dqn_clone_goes_on_where_its_parent_stands():
    from rl_6_nimmt.agents import DDQN_PRBAgent
    from rl_6_nimmt.league import BatchedTournament, decode_seats

    torch.manual_seed(1)
    t = BatchedTournament(48, 2, 4, seed=5, rng="numpy", train=True, fused=False)
    agent = DDQN_PRBAgent(history_length=64, minibatch=16)
    agent.train()
    t.add_player("q", agent)
    for i in range(5):
        t.add_player(f"x{i}")
    t.play_games(2)
    src = t.engines["q"]
    assert src.episode == 2 and src.update_count > 0 and len(src.replay) > 0
    t.copy_player("q", "q_c")
    t.remove_player("x0")
    t.remove_player("x1")
    t._configure()  # what the next game does first
    dst = t.engines["q_c"]
    assert dst is not src and dst.replay is not src.replay and dst.actor is not src.actor
    assert dst.episode == 2 and dst.update_count == src.update_count and dst.replay.beta == src.replay.beta > 0.4
    assert dst.eps_history == src.eps_history and dst.current_eps() == src.current_eps() < 1.0
    assert len(dst.replay) > dst.minibatch
    _same(_export(dst.replay), _inherited(_export(src.replay), dst.capacity))
    steps = t.optimizer_steps.get("q_c", 0)
    rec = t.play_games(1)
    kk, ids = decode_seats(rec[0, :, 0], 4)
    seated = (ids == t.active_agents().index("q_c")) & (torch.arange(4, device=ids.device)[None, :] < kk[:, None])
    assert bool(seated.any()) and t.optimizer_steps["q_c"] > steps and dst.episode == 3
    assert t.env.pipe_errors() == 0
    t.close()


def _hand_engine(capacity, seed=3, games=7, **kw):
    from torch import nn

    from rl_6_nimmt.dqn import BatchedDQN
    from rl_6_nimmt.utils.nets import MultiHeadedMLP
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(games, 4, seed=seed)
    torch.manual_seed(seed)
    net = MultiHeadedMLP(47, hidden_sizes=(64,), head_sizes=(104,), activation=nn.ReLU(), head_activations=(None,))
    return BatchedDQN(env, net.to(env.device), prioritised=True, seats_mask=0b0101, net_dtype=torch.float32, seed=seed,
                      capacity=capacity, minibatch=16, **kw)


def test_engine_clone_of_a_smaller_capacity_takes_the_newest_rows():
    parent, child = _hand_engine(64), _hand_engine(32, seed=4)
    for _ in range(2):  # 2 x 140 rows through 64 slots: wrapped, the pointer at 24
        parent.play_episode(record=True)
    assert (parent.replay.pointer, len(parent.replay)) == (24, 276)
    parent.replay.update(torch.arange(63, 127), torch.linspace(0.1, 0.9, 64, dtype=torch.float64))
    child.play_episode(record=True)  # rows of its own, to be overwritten
    before = _export(parent.replay)
    child.inherit(parent)
    _same(_export(child.replay), _inherited(before, 32))
    _same(_export(parent.replay), before)
    assert (child.replay.pointer, len(child.replay)) == (0, 31) and (child.episode, child.capacity) == (2, 32)
    newest = [(parent.replay.pointer - 32 + k) % 64 for k in range(32)]
    assert torch.equal(_export(child.replay)[1], before[1][newest])
    assert torch.equal(_export(child.replay)[0][31:], before[0][63:][newest])  # the parent's priorities


def test_engines_of_another_row_layout_do_not_inherit():
    one, nstep = _hand_engine(64), _hand_engine(64, seed=4, n_steps=3)
    one.play_episode(record=True)
    nstep.inherit(one)
    assert nstep.replay._h is None and len(nstep.replay) == 0 and nstep.episode == 0
    nstep.play_episode(record=True)
    heir = _hand_engine(32, seed=5, n_steps=3)
    heir.inherit(nstep)
    assert heir.episode == 1 and len(heir.replay) == 31
    one.inherit(heir)
    assert one.episode == 1 and len(one.replay) != 31
