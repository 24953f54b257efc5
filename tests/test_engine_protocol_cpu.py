"""The engine protocol the batched tournament drives (engine.BatchedEngine and
its subclasses; league.py's module docstring), on the host: the decider
index both modes share, the replay sizing of the league's engines,
`from_agent`, `inherit`, that league.py names no engine class in an
isinstance, and that only puct.BatchedPUCT carries the search: its buffers,
its settings and the rollout preparation of `sync_net`."""
import inspect
import re

import pytest
import torch

B, N, MASK, SEATS = 3, 4, 0b0101, [0, 2]
DEC = [9, 1, 6]


class _HostEnv:
    """shape-only stand-in for VecSechsNimmtEnv (tests/test_acer_cpu.py): the
    engines' constructors, replays and losses need no device kernels"""

    def __init__(self, B, N):
        self.num_games, self.num_players, self.device = B, N, torch.device("cpu")


def _per_step():
    return torch.arange(10 * B * N, dtype=torch.int32).reshape(10, B, N)


def _modes(cls, **kw):
    """(engine, the parent commit's selection of its deciders' rewards) in seats-mask and in tournament mode"""
    ps = _per_step()
    masked = cls(_HostEnv(B, N), seats_mask=MASK, net_dtype=torch.float32, **kw)
    listed = cls(_HostEnv(B, N), max_decisions=12, net_dtype=torch.float32, **kw)
    listed.use_decisions(DEC)
    return [(masked, ps[:, :, SEATS].reshape(10, -1)), (listed, ps.reshape(10, -1)[:, DEC])]


def test_decider_index_and_rewards_in_both_modes():
    from rl_6_nimmt.puct import BatchedPUCT, make_actor

    (masked, want_m), (listed, want_l) = _modes(BatchedPUCT, actor=make_actor())
    assert masked.decider_index().tolist() == [0, 2, 4, 6, 8, 10]
    assert masked.decider_index() is masked.decider_index()  # built once
    assert listed.decider_index().tolist() == DEC
    for eng, want in ((masked, want_m), (listed, want_l)):
        got = eng.decider_rewards(_per_step())
        assert got.dtype == want.dtype and torch.equal(got, want)


def test_reinforce_returns_use_the_decider_rewards():
    from rl_6_nimmt.reinforce import BatchedReinforce

    for eng, sel in _modes(BatchedReinforce, gamma=0.9, r_factor=0.5):
        r = sel.T.double() * 0.5  # the parent's expression: [D, T]
        seen = torch.zeros_like(r)
        seen[:, 1:] = r[:, :-1]
        G, acc = torch.zeros_like(seen), torch.zeros_like(seen[:, 0])
        for t in range(9, -1, -1):
            acc = seen[:, t] + 0.9 * acc
            G[:, t] = acc
        assert torch.equal(eng.returns(_per_step()), G.float())


def test_customed_loss_targets_the_decider_rewards():
    """loss = MSE(value of the chosen move, the deciders' first nine rewards
    summed) - log pi(chosen), summed over deciders (mcts.py:431-451): the
    targets are hundreds apart between deciders, so another selection of
    seats moves the loss by orders of magnitude more than fp32 rounding"""
    from rl_6_nimmt.puct import BatchedPUCTCustomed, make_actor_value

    torch.manual_seed(0)
    actor = make_actor_value()
    for eng, sel in _modes(BatchedPUCTCustomed, actor=actor):
        D = sel.shape[1]
        g = torch.Generator().manual_seed(D)
        eng.decisions = [(torch.randn((D * n, 48), generator=g), n, torch.randint(0, n, (D,), generator=g))
                         for n in (3, 2)]
        target = sel[:-1].sum(dim=0).float()
        logps, values = [], []
        for rows, n, best in eng.decisions:
            out = actor(rows)[0].reshape(D, n, 2)
            logps.append(torch.log_softmax(out[:, :, 0], dim=1).gather(1, best[:, None])[:, 0])
            values.append(out[:, :, 1].gather(1, best[:, None])[:, 0])
        logps, values = torch.stack(logps, dim=1), torch.stack(values, dim=1)
        want = (((values - target[:, None]) ** 2).mean(dim=1) - logps.sum(dim=1)).sum()
        got = eng.loss(_per_step())
        assert torch.allclose(got, want, rtol=1e-5, atol=0.0), (float(got), float(want))


@pytest.mark.parametrize("history,seats,capacity", [(1000, 192, 4096), (100000, 192, 131072), (8, 0.75, 16)])
def test_dqn_league_capacity(history, seats, capacity):
    """the next power of two of max(history max_length, int(2 * 10 * seats), 2)"""
    from rl_6_nimmt.dqn import league_capacity

    assert league_capacity(history, seats) == capacity


def test_dqn_league_capacity_of_an_unbounded_history():
    from rl_6_nimmt.dqn import league_capacity

    assert league_capacity(None, 192) == 4096 and league_capacity(None, 0.01) == 2


@pytest.mark.parametrize("warmup,batch,rollout_len,seats,capacity",
                         [(100, 5, 10, 192, 2), (100, 5, 10, 0.75, 102), (100, 5, 4, 10, 5)])
def test_acer_league_capacity(warmup, batch, rollout_len, seats, capacity):
    """max(2, ceil((max(warmup, batch) + 1) / max(1.0, seats * ceil(10 / rollout_len))) + 1)"""
    from rl_6_nimmt.acer import league_capacity

    assert league_capacity(warmup, batch, rollout_len, seats) == capacity


def test_from_agent_builds_each_agents_engine():
    from rl_6_nimmt import agents as A
    from rl_6_nimmt import league
    from rl_6_nimmt.acer import BatchedACER, league_capacity
    from rl_6_nimmt.puct import BatchedPUCT, BatchedPUCTCustomed
    from rl_6_nimmt.reinforce import BatchedReinforce

    assert set(league.ENGINES) == set(league.NET_KINDS)
    slots, seats = 8, 8 * 3 / 5
    cases = [(A.PUCTAgent(mc_max=6, c_puct=1.5), BatchedPUCT, ("mc_per_card", "mc_max", "c_puct")),
             (A.PolicyMCSAgent(mc_max=6), BatchedPUCT, ("mc_per_card", "mc_max")),
             (A.PUCTCustomedAgent(mc_max=6), BatchedPUCTCustomed, ()),
             (A.BatchedReinforceAgent(gamma=0.9, r_factor=0.5), BatchedReinforce,
              ("gamma", "r_factor", "actor_weight", "entropy_weight")),
             (A.BatchedACERAgent(minibatch=3, rollout_len=4, warmup=7), BatchedACER,
              ("gamma", "r_factor", "rollout_len", "warmup", "truncate", "critic_weight", "log_epsilon"))]
    for agent, cls, copied in cases:
        engine = league.ENGINES[league.engine_kind(agent)]
        assert engine is cls
        eng = engine.from_agent(_HostEnv(slots, 4), agent, seed=5, net_dtype=torch.float32, slots=slots, seats=seats)
        assert type(eng) is cls and eng.seed == 5 and eng.net_dtype == torch.float32
        assert eng.D == 0 and eng.D_max == slots and eng.dec is None
        for name in copied:
            assert getattr(eng, name) == getattr(agent, name), (cls.__name__, name)
        if cls is BatchedPUCT:
            assert eng.actor is agent.actor and eng.puct_root == agent._puct_root and eng.mcs_num_cards == agent.num_cards
        if cls is BatchedACER:
            assert eng.actor is agent.actor_critic and eng.minibatch == agent.batchsize == 3
            assert eng.capacity == league_capacity(7, 3, 4, seats) == 2
    assert BatchedPUCT.from_agent(_HostEnv(slots, 4), A.PolicyMCSAgent(), seed=0, net_dtype=torch.float32, slots=slots,
                                  seats=seats).c_puct == 2.0  # no c_puct on the agent: the engine's default


def _acer(capacity):
    from rl_6_nimmt.acer import BatchedACER

    return BatchedACER(_HostEnv(2, 2), net_dtype=torch.float32, capacity=capacity, minibatch=1, warmup=1)


def _replay(eng):
    return [x.clone() for x in (eng.rep_rows, eng.rep_act, eng.rep_logp, eng.rep_rew)] + [list(eng.rep_nd), eng.episodes]


def _same(a, b):
    return all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b))


def test_inherit_takes_the_parents_newest_episodes():
    from rl_6_nimmt.acer import BatchedACER
    from rl_6_nimmt.reinforce import BatchedReinforce

    parent, child = _acer(3), _acer(2)
    for e in range(5):  # episode e is written into slot e % 3, every value e + 1
        s = e % 3
        parent.rep_rows[s], parent.rep_act[s], parent.rep_logp[s], parent.rep_rew[s] = e + 1.0, e + 1, -(e + 1.0), e + 1.5
        parent.rep_nd[s] = e + 1
    parent.episodes = 5
    child.inherit(parent)
    assert child.episodes == 2 and child.rep_nd == [4, 5]  # episodes 3 and 4 in slots 0 and 1
    for slot, e in ((0, 3), (1, 4)):
        assert bool((child.rep_rows[slot] == e + 1.0).all()) and bool((child.rep_act[slot] == e + 1).all())
        assert bool((child.rep_logp[slot] == -(e + 1.0)).all()) and bool((child.rep_rew[slot] == e + 1.5).all())
    # another decider count: the child stays as it is
    other = BatchedACER(_HostEnv(3, 2), net_dtype=torch.float32, capacity=2, minibatch=1, warmup=1)
    before = _replay(other)
    other.inherit(parent)
    assert _same(_replay(other), before) and other.episodes == 0
    # engines without a replay: nothing to take, from or by them
    rf = BatchedReinforce(_HostEnv(2, 2), net_dtype=torch.float32)
    rf.decisions = ["kept"]
    rf.inherit(parent)
    rf.inherit(rf)
    assert rf.decisions == ["kept"] and not hasattr(rf, "rep_rows")
    before = _replay(child)
    child.inherit(rf)
    assert _same(_replay(child), before)


def test_league_names_no_engine_class_in_an_isinstance():
    from rl_6_nimmt import league

    assert not re.search(r"isinstance\([^\n]*\bBatched(PUCT|PUCTCustomed|Reinforce|ACER|DQN)\b", inspect.getsource(league))


# ---------------------------------------------------------------- the base and the search
SEARCH_STATE = ("avail", "ro", "stats", "hist", "root_probs", "mc_per_card", "mc_max", "c_puct", "puct_root", "graph",
                "deal_batch", "fused_rollouts")
SEARCH_POINTERS = ("avail", "rollouts", "stats", "hist", "root_probs", "step_dev")


def _non_search(**kw):
    """the four engines without a search, built as the league (max_decisions) or a seats mask builds them"""
    from torch import nn

    from rl_6_nimmt.acer import BatchedACER
    from rl_6_nimmt.dqn import BatchedDQN
    from rl_6_nimmt.puct import BatchedPUCTCustomed, make_actor_value
    from rl_6_nimmt.reinforce import BatchedReinforce
    from rl_6_nimmt.utils.nets import MultiHeadedMLP

    q_net = MultiHeadedMLP(47, (64,), (104,), nn.ReLU(), (None,))
    return [BatchedPUCTCustomed(_HostEnv(B, N), make_actor_value(), **kw), BatchedReinforce(_HostEnv(B, N), **kw),
            BatchedACER(_HostEnv(B, N), **kw), BatchedDQN(_HostEnv(B, N), q_net, capacity=64, **kw)]


def _puct(**kw):
    from rl_6_nimmt.puct import BatchedPUCT, make_actor

    return BatchedPUCT(_HostEnv(B, N), make_actor(), **kw)


def test_only_the_search_engine_is_a_batched_puct():
    from rl_6_nimmt.engine import BatchedEngine
    from rl_6_nimmt.puct import BatchedPUCT

    assert issubclass(BatchedPUCT, BatchedEngine)
    for eng in _non_search(max_decisions=12):
        assert isinstance(eng, BatchedEngine) and not isinstance(eng, BatchedPUCT), type(eng).__name__


@pytest.mark.parametrize("kw", [{"max_decisions": 12}, {"seats_mask": MASK}], ids=["listed", "masked"])
def test_non_search_engines_carry_no_search_state(kw):
    for eng in _non_search(**kw):
        name = type(eng).__name__
        assert [a for a in SEARCH_STATE if hasattr(eng, a)] == [], name
        eng.seed, eng.step_id = 7, 3
        q = eng._params(4)
        assert [f for f in SEARCH_POINTERS if getattr(q, f) is not None] == [], name
        assert (q.seats_mask, q.n, q.seed, q.step) == (eng.seats_mask, 4, 7, 3), name
        if "max_decisions" in kw:
            assert q.dec_list is None and q.num_dec == 0 and eng.D == 0, name
            eng.use_decisions(DEC)
            q = eng._params(4)
            assert q.num_dec == 3 and q.dec_list == eng.dec.data_ptr() and eng.D == 3, name
        else:
            assert q.dec_list is None and q.num_dec == 0 and eng.D == B * len(SEATS), name


def test_batched_puct_keeps_its_search_state():
    eng = _puct(max_decisions=12)
    shapes = {"ro": (12, 48), "stats": (12, 24), "hist": (12, 172), "root_probs": (12, 10), "avail": (4, B * N)}
    assert {a: tuple(getattr(eng, a).shape) for a in shapes} == shapes
    assert all(hasattr(eng, a) for a in SEARCH_STATE)
    q = eng._params(4)
    for field, attr in (("avail", "avail"), ("rollouts", "ro"), ("stats", "stats"), ("hist", "hist"),
                        ("root_probs", "root_probs")):
        assert getattr(q, field) == getattr(eng, attr).data_ptr(), field
    assert q.step_dev is None and q.puct_root == 1 and q.c_puct == 2.0
    assert eng._params(4, step_dev=True).step_dev == eng._step_dev.data_ptr()
    assert eng._params(4, rollout=5).rollout == 5


def test_decide_without_a_seat_makes_no_native_call(monkeypatch):
    from rl_6_nimmt import _native

    def no_lib():
        raise AssertionError("a native call without a deciding seat")

    monkeypatch.setattr(_native, "lib", no_lib)
    for eng in _non_search(max_decisions=12) + [_puct(max_decisions=12)]:
        assert eng.D == 0
        before = eng.step_id
        assert eng.decide(4, memorize=False, record=True) is eng.actions, type(eng).__name__
        assert eng.step_id == before + 1, type(eng).__name__


def test_only_the_search_prepares_rollouts_in_sync_net():
    """the default actor in bf16 has the one-kernel rollout form (FusedMLP.fused): BatchedPUCT packs it and
    allocates the rollout logits when it builds its copy of the net, an engine that never rolls out does neither"""
    from rl_6_nimmt.reinforce import BatchedReinforce

    rf = BatchedReinforce(_HostEnv(B, N), max_decisions=12, net_dtype=torch.bfloat16)
    net = rf.sync_net()
    assert net is rf._net and not hasattr(rf, "_fbufs") and not hasattr(net, "_fused")
    assert net.fused() is not None  # the pack exists for this net: nobody asked for it until now
    eng = _puct(max_decisions=12, net_dtype=torch.bfloat16)
    net = eng.sync_net()
    assert getattr(net, "_fused", None) is not None
    assert eng._fbufs.numel() == eng.D_max * N * 10 == 12 * 4 * 10
