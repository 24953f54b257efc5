"""CPU checks of the noisy DQN agents (utils/nets.py NoisyFactorizedLinear,
agents/dqn.py Noisy_DQN / Noisy_D3QN / Noisy_D3QN_PRB_NStep, the host models
of rl_6_nimmt/dqn.py): no GPU, no kernel call.

* the noisy nets load the reference's state dicts (golden F18) strict=True;
* a forward draws torch.randn((1, K)) then torch.randn((J, 1)) per layer, in
  eval mode too, and returns the reference's formula on those buffers, bit for
  bit;
* the classes: bases, MRO, registry names, engine_kind "dqn"; `forward` leaves
  Python's `random` alone and reports no epsilon;
* FusedMLP.of does not take a noisy net for a plain one;
* noisy_eps_host -- the model sn_noisy_eps is held to on the GPU: its Philox
  against the oracle's, and the law of 2^20 values of a fixed key;
* noisy_forward_host against the module's forward.
"""
import json
import math
import os
import random

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

from conftest import GOLDEN

SPEC = json.load(open(os.path.join(GOLDEN, "dqn_noisy_games.json")))
NOISY_NAMES = {"noisy_dqn": "Noisy_DQN", "noisy_d3qn": "Noisy_D3QN", "noisy_d3qn_prb_nstep": "Noisy_D3QN_PRB_NStep"}
LAYER_KEYS = ["weight", "bias", "sigma_weight", "sigma_bias", "epsilon_input", "epsilon_output"]


def _noisy_mlp(hidden=(64,), sigma=0.5):
    from rl_6_nimmt.utils.nets import MultiHeadedMLP, NoisyFactorizedLinear

    return MultiHeadedMLP(47, hidden_sizes=hidden, head_sizes=(104,), activation=nn.ReLU(), head_activations=(None,),
                          linear=NoisyFactorizedLinear, init_sigma=sigma)


def _noisy_duel(hidden=(64,), sigma=0.5):
    from rl_6_nimmt.utils.nets import DuellingDQNNet, NoisyFactorizedLinear

    return DuellingDQNNet(47, hidden_sizes=hidden, out_size=104, activation=nn.ReLU(), linear=NoisyFactorizedLinear,
                          init_sigma=sigma)


def _f(x):
    return torch.sign(x) * torch.sqrt(torch.abs(x))


def test_fixture_holds_the_three_sessions():
    got = [(s["agent"], s["kwargs"].get("n_steps", 1)) for s in SPEC["sessions"]]
    assert got == [("Noisy_DQN", 1), ("Noisy_D3QN", 1), ("Noisy_D3QN_PRB_NStep", 3)]
    W = np.load(os.path.join(GOLDEN, "dqn_noisy_weights.npz"))
    assert not [k for k in W.files if "epsilon_" in k or "_init_dqn_net_target." in k]
    assert [k for k in W.files if k.startswith("s2_per_idx")] and "s0_eps" not in W.files


def test_noisy_nets_load_the_reference_state_dicts():
    from rl_6_nimmt.utils.nets import NoisyFactorizedLinear

    W = np.load(os.path.join(GOLDEN, "dqn_noisy_weights.npz"))
    for si, net, prefixes in ((0, _noisy_mlp(), ["latent_net.0.", "head_nets.0.0."]),
                              (1, _noisy_duel(), ["mlp.latent_net.0.", "mlp.head_nets.0.0.", "mlp.head_nets.1.0."])):
        assert sorted(net.state_dict()) == sorted(p + k for p in prefixes for k in LAYER_KEYS)
        assert len(net.state_dict()) == 6 * len(prefixes)  # twelve per two-layer net, six more for the V head
        pre = f"s{si}_final_dqn_net_local."
        sd = {k[len(pre):]: torch.from_numpy(W[k]) for k in W.files if k.startswith(pre)}
        for name, buf in net.named_buffers():  # the fixture leaves the redrawn buffers out
            sd[name] = torch.zeros_like(buf)
        assert all(v.shape == net.state_dict()[k].shape for k, v in sd.items())
        net.load_state_dict(sd, strict=True)
        lin = [m for m in net.modules() if isinstance(m, NoisyFactorizedLinear)]
        assert len(lin) == len(prefixes)
        assert lin[0].epsilon_input.shape == (1, 47) and lin[0].epsilon_output.shape == (64, 1)
        assert lin[-1].sigma_weight.shape == (104, 64) and lin[-1].sigma_bias.shape == (104,)


@pytest.mark.parametrize("evaluate", [False, True])
@pytest.mark.parametrize("make", [_noisy_mlp, _noisy_duel])
def test_forward_draws_input_then_output_noise_and_applies_the_formula(make, evaluate):
    from rl_6_nimmt.dqn import noisy_linears

    torch.manual_seed(5)
    net = make(hidden=(24, 40))
    if evaluate:
        net.eval()
    x = torch.randint(-1, 104, (3, 47), generator=torch.Generator().manual_seed(1)).float()
    torch.manual_seed(77)
    with torch.no_grad():
        (got,) = net(x)
    torch.manual_seed(77)
    lin = noisy_linears(net)
    assert [m.in_features for m in lin] == [47, 24, 40] + ([40] if make is _noisy_duel else [])
    outs, h = [], x
    with torch.no_grad():
        for i, m in enumerate(lin):
            e_in, e_out = torch.randn((1, m.in_features)), torch.randn((m.out_features, 1))
            assert torch.equal(m.epsilon_input, e_in) and torch.equal(m.epsilon_output, e_out), i
            y = F.linear(h, m.weight + m.sigma_weight * (_f(e_out) * _f(e_in)), m.bias + m.sigma_bias * _f(e_out).view(-1))
            if i < 2:
                h = torch.relu(y)
            else:
                outs.append(y)
    if make is _noisy_duel:
        V, A = outs
        want = V + (A - A.mean(dim=-1, keepdim=True))
    else:
        (want,) = outs
    assert torch.equal(got, want)
    torch.manual_seed(78)
    with torch.no_grad():
        assert not torch.equal(net(x)[0], got)  # the next forward has its own noise


def test_initial_sigma():
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.utils.nets import NoisyFactorizedLinear

    for K, J, s in ((47, 64, 0.5), (64, 104, 0.5), (10, 3, 0.4), (7, 1, 2.0)):
        m = NoisyFactorizedLinear(K, J, sigma_init=s)
        assert isinstance(m, nn.Linear)
        want = torch.full((J, K), s / math.sqrt(K))
        assert torch.equal(m.sigma_weight.detach(), want) and torch.equal(m.sigma_bias.detach(), want[:, 0])
    net = _noisy_mlp(hidden=(24,), sigma=0.3)
    assert torch.equal(net.head_nets[0][0].sigma_bias.detach(), torch.full((104,), 0.3 / math.sqrt(24)))
    for cls in A.DQN_NOISY_AGENTS.values():
        a = cls(history_length=32, minibatch=4)
        assert a.noisy_init_sigma == 0.5
        for m in a.dqn_net_local.modules():
            if isinstance(m, NoisyFactorizedLinear):
                assert torch.equal(m.sigma_weight.detach(),
                                   torch.full_like(m.sigma_weight, 0.5 / math.sqrt(m.in_features)))
    assert A.Noisy_DQN(history_length=32, noisy_init_sigma=0.1).dqn_net_local.latent_net[0].sigma_bias[0].item() == \
        pytest.approx(0.1 / math.sqrt(47), rel=1e-6)


def test_class_layout_registry_and_engine_kind():
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.agents import dqn as M
    from rl_6_nimmt.league import engine_kind
    from rl_6_nimmt.utils.nets import DuellingDQNNet, MultiHeadedMLP, NoisyFactorizedLinear
    from rl_6_nimmt.utils.replay_buffer import History, PriorityReplayBuffer

    assert {k: v.__name__ for k, v in A.DQN_NOISY_AGENTS.items()} == NOISY_NAMES
    assert (A.NOISY_DQN, A.NOISY_D3QN, A.NOISY_D_QN_PRB_NSTEP) == ("noisy_dqn", "noisy_d3qn", "noisy_d3qn_prb_nstep")
    assert sorted(A.DQN_AGENTS) == ["ddqn", "ddqn_prb", "dqn", "dqn_prb"]
    assert not set(A.DQN_NOISY_AGENTS) & (set(A.DQN_AGENTS) | set(A.DQN_VARIANT_AGENTS) | set(A.AGENTS))
    assert M.Noisy_DQN.__bases__ == (M.DQNVanilla,)
    assert M.Noisy_D3QN.__bases__ == (M.DuellingDDQNAgent, M.Noisy_DQN)
    assert M.Noisy_D3QN_PRB_NStep.__bases__ == (M.Noisy_D3QN, M.D3QN_PRB_NStep)
    assert M.Noisy_D3QN_PRB_NStep.__mro__[:10] == (
        M.Noisy_D3QN_PRB_NStep, M.Noisy_D3QN, M.D3QN_PRB_NStep, M.DQN_NStep_Agent, M.DuellingDDQN_PRBAgent,
        M.DQN_PRBAgent, M.DuellingDDQNAgent, M.DDQNAgent, M.Noisy_DQN, M.DQNVanilla)
    was = torch.cuda.is_initialized()
    for name, cls in A.DQN_NOISY_AGENTS.items():
        a = cls(history_length=32, minibatch=4, n_steps=3 if "nstep" in name else 1)
        a.train()
        assert engine_kind(a) == "dqn", name
        duel = name != "noisy_dqn"
        assert type(a.dqn_net_local) is (DuellingDQNNet if duel else MultiHeadedMLP)
        layers = [m for m in a.dqn_net_local.modules() if isinstance(m, nn.Linear)]
        assert len(layers) == (3 if duel else 2) and all(type(m) is NoisyFactorizedLinear for m in layers)
        assert hasattr(a, "dqn_net_target") == duel
        if duel:
            assert all(torch.equal(p, q) for p, q in zip(a.dqn_net_local.parameters(), a.dqn_net_target.parameters()))
            assert any(isinstance(m, NoisyFactorizedLinear) for m in a.dqn_net_target.modules())
        assert type(a.history) is (PriorityReplayBuffer if "prb" in name else History)
        assert hasattr(a, "n_step_buffer") == ("nstep" in name)
    assert torch.cuda.is_initialized() == was


def test_soft_update_carries_the_sigmas_and_not_the_noise_buffers():
    from rl_6_nimmt import agents as A

    a = A.Noisy_D3QN(history_length=32, minibatch=4)
    with torch.no_grad():
        a.dqn_net_local(torch.zeros(1, 47))  # fills the local net's buffers
        for p in a.dqn_net_local.parameters():
            p.add_(1.0)
    before = {k: v.clone() for k, v in a.dqn_net_target.state_dict().items()}
    a.soft_update(a.dqn_net_local, a.dqn_net_target, 0.25)
    local, after = a.dqn_net_local.state_dict(), a.dqn_net_target.state_dict()
    for k in after:
        if "epsilon_" in k:
            assert torch.equal(after[k], before[k]) and not torch.equal(after[k], local[k])
        else:
            assert torch.equal(after[k], 0.25 * local[k] + 0.75 * before[k]), k
    assert any("sigma_weight" in k for k in after)


def test_forward_is_the_argmax_over_the_legal_cards_without_python_random():
    from rl_6_nimmt import agents as A

    for cls in A.DQN_NOISY_AGENTS.values():
        torch.manual_seed(3)
        a = cls(history_length=32, minibatch=4)
        a.train()
        assert a.eps == 1.0  # the schedule still runs; nothing reads it
        state = torch.randint(-1, 104, (47,), generator=torch.Generator().manual_seed(2)).float()
        legal = [3, 17, 40, 99]
        random.seed(11)
        before = random.getstate()
        torch.manual_seed(21)
        action, info = a.forward(state, legal_actions=legal)
        assert random.getstate() == before
        assert set(info) == {"value"}
        torch.manual_seed(21)
        with torch.no_grad():
            scores = a.dqn_net_local(state)[0]
        assert action == legal[int(torch.argmax(scores[legal]))] and float(info["value"]) == float(scores[legal].max())
        torch.manual_seed(21)
        action, info = a.forward(state)  # no legal list: all 104 actions
        assert action == int(torch.argmax(scores)) and float(info["value"]) == float(scores.max())
        torch.manual_seed(21)
        assert a.forward(state, legal_actions=[])[0] == int(torch.argmax(scores))
        assert a.dqn_net_local.training


def test_learn_updates_eps_and_trains_the_sigmas():
    from rl_6_nimmt import agents as A

    torch.manual_seed(4)
    a = A.Noisy_DQN(history_length=64, minibatch=4, eps_func=lambda episode: 0.25 + episode)
    a.train()
    before = {k: v.detach().clone() for k, v in a.dqn_net_local.named_parameters()}
    g = torch.Generator().manual_seed(5)
    for t in range(8):
        s, s2 = (torch.randint(-1, 104, (47,), generator=g).float() for _ in range(2))
        loss = a.learn(state=s, reward=-t, action=t, done=t == 7, next_state=s2, next_reward=0.0,
                       episode_end=t == 7, num_episode=2, legal_actions=[1, 2])
        assert isinstance(loss, np.ndarray) and loss.shape == (1,)
    assert a.eps == 2.25 and float(loss[0]) > 0
    for k, v in a.dqn_net_local.named_parameters():
        assert not torch.equal(v.detach(), before[k]), k  # weight, bias, sigma_weight, sigma_bias of both layers


def test_fused_mlp_does_not_take_a_noisy_net_for_a_plain_one():
    from rl_6_nimmt.engine import FusedMLP
    from rl_6_nimmt.utils.nets import MultiHeadedMLP

    for net in (_noisy_mlp(), _noisy_duel().mlp):
        f = FusedMLP.of(net)
        assert f.layers is None and f.module is net
    plain = MultiHeadedMLP(47, (64,), (104,), nn.ReLU(), (None,))
    assert FusedMLP.of(plain).layers is not None
    with pytest.raises(NotImplementedError):
        MultiHeadedMLP(47, (64,), (104,), nn.ReLU(), (None,), linear=nn.Bilinear)


# ---------------------------------------------------------------- the host models
def test_host_philox_is_the_oracles():
    from oracle import oracle
    from rl_6_nimmt.dqn import philox4x32_10_host

    rng = np.random.default_rng(9)
    ctr = rng.integers(0, 2 ** 32, (64, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, (64, 2), dtype=np.uint64).astype(np.uint32)
    ctr[0], key[0] = 0, 0
    ctr[1], key[1] = 0xFFFFFFFF, 0xFFFFFFFF
    got = philox4x32_10_host(ctr, key)
    assert got.dtype == np.uint32 and got.shape == (64, 4)
    for i in range(64):
        assert np.array_equal(got[i], oracle.philox(ctr[i], key[i])), i
    one = philox4x32_10_host(ctr, key[5])  # a key broadcast over the counters
    assert np.array_equal(one[5], got[5]) and not np.array_equal(one[6], got[6])


def test_noisy_eps_host_keys_and_law():
    """2^20 values of one fixed key: |mean e| <= 4.4e-3 (5 sigma: Var e = E|n| = 0.798), |mean e^2 - sqrt(2/pi)|
    <= 3.0e-3 (5 sigma: Var |n| = 1 - 2/pi), Kolmogorov distance of n = sign(e) e^2 from Phi <= 1.95 / sqrt(2^20)
    (the 0.1 % critical value).  Derived, not measured; the key is fixed, so the test is deterministic."""
    from rl_6_nimmt.dqn import NOISY_TAG0, noisy_eps_host, noisy_normals_host, noisy_tag

    assert (noisy_tag(0, 0), noisy_tag(0, 1), noisy_tag(63, 1)) == (NOISY_TAG0, NOISY_TAG0 + 1, 0xFFF7F) and \
        noisy_tag(63, 1) < 0xFFFFE
    with pytest.raises(AssertionError):
        noisy_tag(64, 0)
    N = 1 << 20
    e = noisy_eps_host(0x1234567890ABCDEF, 7, 3, 2, 1, 0, N)
    assert e.dtype == np.float64 and e.shape == (N,) and bool(np.isfinite(e).all())
    n = np.sign(e) * e * e
    assert np.allclose(n, noisy_normals_host(0x1234567890ABCDEF, 7, 3, 2, 1, 0, N), rtol=1e-14, atol=0)
    assert float(np.abs(n).max()) <= math.sqrt(48 * math.log(2))
    m1, m2 = abs(float(e.mean())), abs(float((e * e).mean()) - math.sqrt(2 / math.pi))
    xs = np.sort(n)
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(xs) / math.sqrt(2.0))).numpy()
    ks = max(float(np.max(np.arange(1, N + 1) / N - cdf)), float(np.max(cdf - np.arange(N) / N)))
    print("mean e", m1, "mean e^2 - sqrt(2/pi)", m2, "KS", ks, "bound", 1.95 / math.sqrt(N))
    assert m1 <= 4.4e-3 and m2 <= 3.0e-3 and ks <= 1.95 / math.sqrt(N)
    # a prefix is a prefix (an odd width uses half of its last pair); every key field gives another row
    base = (5, 7, 3, 2, 1, 0)
    row = noisy_eps_host(*base, 47)
    assert np.array_equal(row, noisy_eps_host(*base, 104)[:47]) and np.array_equal(row[:1], noisy_eps_host(*base, 1))
    for i in range(6):
        other = list(base)
        other[i] += 1
        assert not np.array_equal(noisy_eps_host(*other, 47), row), i
    assert np.array_equal(noisy_eps_host(5 + (1 << 64), *base[1:], 47), row)  # the seed is 64 bits


@pytest.mark.parametrize("make", [_noisy_mlp, _noisy_duel])
def test_noisy_forward_host_is_the_modules_forward(make):
    from rl_6_nimmt.dqn import noisy_forward_host, noisy_linears

    torch.manual_seed(6)
    net = make(hidden=(24, 40)).double()
    with torch.no_grad():
        for m in noisy_linears(net):  # sigmas of their own, as after training
            m.sigma_weight.mul_(1.0 + torch.rand_like(m.sigma_weight))
            m.sigma_bias.mul_(1.0 + torch.rand_like(m.sigma_bias))
    x = torch.randint(-1, 104, (5, 47), generator=torch.Generator().manual_seed(1)).double()
    with torch.no_grad():
        (want,) = net(x)
    eps = [(_f(m.epsilon_input).expand(5, -1), _f(m.epsilon_output).t().expand(5, -1)) for m in noisy_linears(net)]
    (got,) = noisy_forward_host(net, x, eps)
    assert got.dtype == torch.float64 and got.shape == (5, 104)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-12 * max(scale, 1.0)
    # rows with noise of their own: each row is the module under that row's buffers
    g = torch.Generator().manual_seed(2)
    eps = [(_f(torch.randn((5, m.in_features), generator=g, dtype=torch.float64)),
            _f(torch.randn((5, m.out_features), generator=g, dtype=torch.float64))) for m in noisy_linears(net)]
    (got,) = noisy_forward_host(net, x, eps)
    for r in (0, 4):
        h, outs = x[r], []
        with torch.no_grad():
            for i, m in enumerate(noisy_linears(net)):
                e_in, e_out = eps[i][0][r], eps[i][1][r]
                y = F.linear(h, m.weight + m.sigma_weight * torch.outer(e_out, e_in), m.bias + m.sigma_bias * e_out)
                if i < 2:
                    h = torch.relu(y)
                else:
                    outs.append(y)
        want = outs[0] if make is _noisy_mlp else outs[0] + (outs[1] - outs[1].mean())
        assert float((got[r] - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)
