"""CPU checks of the replay's clone rule (replay.inherit_host, the model of
sn_per_inherit) and of cloning a DevicePER that holds no device
memory yet.

`TaggedModel` is test_replay_cpu.PerModel with every slot tagged by the number
of the store that wrote it (1, 2, ...; 0 = never written), so that "the newest
h rows, oldest first" can be read off the tags.  `build_parent` drives it into
one of four states -- empty, partly filled, exactly full (the store that wraps:
pointer 0, num_items = cap - 1), wrapped with the pointer mid-ring -- and then
gives the written leaves distinct priorities (sqrt(1), sqrt(2), ...: sums that
round, written as they are with alpha = 1, epsilon = 0, no clip, so the device
holds the same doubles).  The GPU tests (test_gpu_replay_inherit.py) drive a
DevicePER through the same history.
"""
import copy
import io
import pickle

import numpy as np
import pytest
import torch

from test_replay_cpu import PerModel

STATES = ("empty", "partly", "full", "wrapped")
PAIRS = [(5, 5), (5, 3), (5, 8), (8, 2), (2, 5), (6, 6)]


class TaggedModel(PerModel):
    def __init__(self, capacity):
        super().__init__(capacity)
        self.tags = np.zeros(capacity, dtype=np.int64)
        self.stores = 0

    def store(self, m=1):
        slots = super().store(m)
        self.tags[slots] = self.stores + 1 + np.arange(m)
        self.stores += m
        return slots

    @property
    def leaves(self):
        return self.tree[self.cap - 1:]


def store_chunks(cap, state):
    """the batched stores (each <= cap) that bring an empty ring into `state`"""
    some = max(1, cap // 2)
    return {"empty": [], "partly": [some], "full": [cap], "wrapped": [cap, cap, some]}[state]


def distinct_update(cap, filled):
    """(tree indices, priorities) that make the first `filled` leaves distinct"""
    return cap - 1 + np.arange(filled), np.sqrt(1.0 + np.arange(filled))


def build_parent(cap, state, also=None):
    """a TaggedModel in `state`; `also(m, first_tag)` / `also(idx, prio)` mirror every store / the update"""
    model = TaggedModel(cap)
    for m in store_chunks(cap, state):
        if also is not None:
            also.store(m, model.stores + 1)
        model.store(m)
    filled = min(model.stores, cap)
    if filled:
        idx, prio = distinct_update(cap, filled)
        model.update(idx, prio, epsilon=0.0, upper=float("inf"), alpha=1.0)
        if also is not None:
            also.update(idx, prio)
    return model


def expected_state(state, cap):
    stores = sum(store_chunks(cap, state))
    return stores % cap, stores - stores // cap


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("cap", [2, 5, 6, 8])
def test_parent_states_are_what_they_are_called(cap, state):
    m = build_parent(cap, state)
    assert (m.pointer, m.num_items) == expected_state(state, cap)
    if state == "full":
        assert m.pointer == 0 and m.num_items == cap - 1
    if state == "wrapped":
        assert 0 < m.pointer < cap and (m.tags > 0).all()
    filled = min(m.stores, cap)
    assert len(set(m.leaves[:filled])) == filled and (m.leaves[filled:] == 0).all()


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("cap_p,cap_c", PAIRS)
def test_inherit_host_keeps_the_newest_rows_in_age_order(cap_p, cap_c, state):
    from rl_6_nimmt.replay import inherit_host

    p = build_parent(cap_p, state)
    rows = np.stack((p.tags, -p.tags), axis=1)  # two columns: a row moves as a whole
    before = (p.leaves.copy(), rows.copy())
    leaves, new_rows, pointer, num_items = inherit_host(p.leaves, rows, p.pointer, p.num_items, cap_c)
    leaves, new_rows = leaves.numpy(), new_rows.numpy()
    assert np.array_equal(p.leaves, before[0]) and np.array_equal(rows, before[1])  # the parent's arrays are left alone
    assert leaves.shape == (cap_c,) and leaves.dtype == np.float64 and new_rows.shape == (cap_c, 2)
    if cap_p == cap_c:  # verbatim: slot for slot, the counters as they are (num_items past the capacity too)
        assert np.array_equal(leaves, p.leaves) and np.array_equal(new_rows, rows)
        assert (pointer, num_items) == (p.pointer, p.num_items)
        return
    h = min(p.stores, cap_p, cap_c)
    newest = np.arange(p.stores - h + 1, p.stores + 1)  # store numbers, oldest first
    assert new_rows[:h, 0].tolist() == newest.tolist() and np.array_equal(new_rows[:, 1], -new_rows[:, 0])
    where = {int(t): s for s, t in enumerate(p.tags) if t}
    assert leaves[:h].tolist() == [p.leaves[where[int(t)]] for t in newest]  # the parent's priorities, not the maximum
    assert (leaves[h:] == 0).all() and (new_rows[h:] == 0).all()
    fresh = PerModel(cap_c)
    for _ in range(h):
        fresh.store()
    assert (pointer, num_items) == (fresh.pointer, fresh.num_items)
    if state == "wrapped" and cap_c > cap_p:  # the whole parent fits: nothing is lost, only re-homed
        assert sorted(leaves[:h]) == sorted(p.leaves)


def test_inherit_host_runs_without_rows_and_on_torch_tensors():
    from rl_6_nimmt.replay import inherit_host

    p = build_parent(5, "wrapped")
    leaves, rows, pointer, num_items = inherit_host(torch.from_numpy(p.leaves.copy()), None, p.pointer, p.num_items, 3)
    want, _, wp, wn = inherit_host(p.leaves, p.tags[:, None], p.pointer, p.num_items, 3)
    assert rows is None and torch.equal(leaves, want) and (pointer, num_items) == (wp, wn) == (0, 2)
    ring = torch.arange(5 * 16, dtype=torch.uint8).reshape(5, 16)  # the device ring's form
    _, got, _, _ = inherit_host(p.leaves, ring, p.pointer, p.num_items, 8)
    order = [(p.pointer + k) % 5 for k in range(5)]
    assert got.dtype == torch.uint8 and torch.equal(got[:5], ring[order]) and not got[5:].any()


@pytest.mark.parametrize("cap", [2, 3, 5])
def test_the_ring_has_wrapped_exactly_when_num_items_differs_from_the_pointer(cap):
    m = PerModel(cap)
    for stores in range(4 * cap + 1):
        assert (m.num_items != m.pointer) == (stores >= cap), (cap, stores)
        m.store()


def _hyper(per):
    return per.alpha, per.beta, per.beta_increment, per.epsilon, per.absolute_error_upper


def test_a_handle_less_replay_copies_and_pickles_without_a_gpu():
    from rl_6_nimmt.agents import DQN_PRBAgent
    from rl_6_nimmt.replay import DevicePER

    was = torch.cuda.is_initialized()
    per = DevicePER(100, row_bytes=112)
    per.alpha, per.beta, per.beta_increment, per.epsilon, per.absolute_error_upper = 0.5, 0.7, 0.002, 0.02, 2.0
    buf = io.BytesIO()
    torch.save(per, buf)
    buf.seek(0)
    for other in (copy.deepcopy(per), per.clone(), pickle.loads(pickle.dumps(per)), torch.load(buf, weights_only=False)):
        assert other is not per and other._h is None and (other.capacity, other.row_bytes) == (100, 112)
        assert len(other) == 0 and other.pointer == 0 and _hyper(other) == (0.5, 0.7, 0.002, 0.02, 2.0)
    child = DevicePER(50, row_bytes=112)
    child.inherit(per)
    assert child._h is None and len(child) == 0 and _hyper(child) == _hyper(per)
    with pytest.raises(ValueError):
        DevicePER(50, row_bytes=16).inherit(per)
    agent = DQN_PRBAgent(history_length=8, minibatch=2)
    agent.history.beta = 0.9
    clone = copy.deepcopy(agent)
    assert clone.history is not agent.history and clone.history.per is not agent.history.per
    assert clone.history.per._h is None and clone.history.beta == 0.9 and len(clone.history) == 0
    assert torch.cuda.is_initialized() == was


def test_a_loaded_state_waits_on_the_host_and_answers_from_its_counters():
    """what __setstate__ keeps until the handle is next created: the counters answer, a copy or a pickle
    carries the arrays on, and a clone of another capacity re-homes them by inherit_host -- all without a GPU"""
    from rl_6_nimmt.replay import DevicePER, inherit_host

    was = torch.cuda.is_initialized()
    p = build_parent(5, "wrapped")
    ring = torch.arange(5 * 16, dtype=torch.uint8).reshape(5, 16)
    state = DevicePER(5, row_bytes=16).__getstate__()
    assert "saved" not in state
    state["saved"] = (torch.from_numpy(p.leaves.copy()), ring, p.pointer, p.num_items)
    state["beta"] = 0.55
    per = DevicePER.__new__(DevicePER)
    per.__setstate__(state)
    assert per._h is None and (per.pointer, len(per)) == (p.pointer, p.num_items) and per.beta == 0.55
    for other in (copy.deepcopy(per), pickle.loads(pickle.dumps(per))):
        assert other._h is None and (other.pointer, len(other)) == (p.pointer, p.num_items) and other.beta == 0.55
        assert torch.equal(other._saved[0], per._saved[0]) and torch.equal(other._saved[1], ring)
    assert copy.deepcopy(per)._saved[0] is not per._saved[0]
    small = DevicePER(3, row_bytes=16)
    small.inherit(per)
    want = inherit_host(p.leaves, ring, p.pointer, p.num_items, 3)
    assert small._h is None and (small.pointer, len(small)) == want[2:] == (0, 2)
    assert torch.equal(small._saved[0], want[0]) and torch.equal(small._saved[1], want[1])
    assert torch.cuda.is_initialized() == was


def test_a_dqn_engine_inherits_its_counters_only_from_its_own_kind():
    from torch import nn

    from rl_6_nimmt.acer import BatchedACER
    from rl_6_nimmt.dqn import BatchedDQN
    from rl_6_nimmt.utils.nets import MultiHeadedMLP
    from test_engine_protocol_cpu import _HostEnv

    def engine(**kw):
        q_net = MultiHeadedMLP(47, (64,), (104,), nn.ReLU(), (None,))
        kw.setdefault("capacity", 64)
        return BatchedDQN(_HostEnv(3, 4), q_net, net_dtype=torch.float32, max_decisions=12, **kw)

    parent = engine(prioritised=True)
    parent.episode, parent.update_count, parent.eps_history, parent.replay.beta = 3, 30, [1.0, 0.9, 0.8], 0.43
    child = engine(prioritised=True, capacity=32)
    child.inherit(parent)
    assert (child.episode, child.update_count, child.eps_history, child.replay.beta) == (3, 30, [1.0, 0.9, 0.8], 0.43)
    assert child.eps_history is not parent.eps_history and child.replay._h is None and child.capacity == 32
    assert child.current_eps() == parent.current_eps() < 1.0  # the schedule goes on
    for other in (engine(n_steps=3), BatchedACER(_HostEnv(3, 4), net_dtype=torch.float32, max_decisions=12)):
        fresh = engine()
        fresh.inherit(other)
        other.inherit(parent)
        assert (fresh.episode, fresh.update_count, fresh.eps_history, fresh.replay.beta) == (0, 0, [], 0.4)
    nstep = engine(n_steps=3)
    nstep.episode = 5
    heir = engine(n_steps=3)
    heir.inherit(nstep)
    assert heir.episode == 5
