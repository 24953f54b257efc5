"""GPU checks of the noisy DQN agents: the noise kernels sn_noisy_eps,
sn_noisy_scale and sn_noisy_combine against their host models
(rl_6_nimmt/dqn.py: noisy_eps_host, noisy_forward_host -- tied to the
reference's layer by test_dqn_noisy_cpu.py), the engine built on them (every
decision row under its own noise), its seat in the batched league, and the
drop-in agents on the recorded sessions of golden F18.
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

SPEC = json.load(open(os.path.join(GOLDEN, "dqn_noisy_games.json")))

EB, N, MASK, SEATS = 16, 4, 0b0101, [0, 2]
ED = EB * len(SEATS)
SEED = 3
U = 2.0 ** -24  # fp32 unit roundoff


def _noisy_net(seed, duelling, hidden=(64,), sigma=0.5):
    from rl_6_nimmt.utils.nets import DuellingDQNNet, MultiHeadedMLP, NoisyFactorizedLinear

    torch.manual_seed(seed)
    if duelling:
        return DuellingDQNNet(47, hidden_sizes=hidden, out_size=104, activation=nn.ReLU(), linear=NoisyFactorizedLinear,
                              init_sigma=sigma)
    return MultiHeadedMLP(47, hidden_sizes=hidden, head_sizes=(104,), activation=nn.ReLU(), head_activations=(None,),
                          linear=NoisyFactorizedLinear, init_sigma=sigma)


def _engine(seed=SEED, duelling=False, hidden=(64,), target=False, prioritised=False, games=EB, game_offset=0, **kw):
    from rl_6_nimmt.dqn import BatchedDQN
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(games, N, seed=seed, game_offset=game_offset)
    net = _noisy_net(seed, duelling, hidden).to(env.device)
    tgt = copy.deepcopy(net) if target else None
    kw.setdefault("capacity", 1024)
    kw.setdefault("net_dtype", torch.float32)
    return env, BatchedDQN(env, net, target_net=tgt, prioritised=prioritised, seats_mask=MASK, seed=seed, **kw)


def _eps(env, q, layer, side, width, D=ED):
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.dqn import noisy_tag

    out = torch.full((D, width), float("nan"), device=env.device)
    nat.check(nat.lib().sn_noisy_eps(env._h, ctypes.byref(q), noisy_tag(layer, side), width, nat.ptr(out), env._stream()),
              "sn_noisy_eps")
    return out


def _normal(e):
    return torch.sign(e) * e * e


# ---------------------------------------------------------------- sn_noisy_eps
def test_eps_follows_the_host_law_for_every_decider():
    """|sign(e) e^2 - n_host| <= 2^-16: at r <= 5.77 the argument rounding of 2 pi u2 (2^-22 r), 3 ulp of logf
    through r, 4 ulp of cosf / sinf and the roundings of sqrt and the square stay below it -- a bound, not a
    measurement"""
    from rl_6_nimmt.dqn import noisy_normals_host

    env, eng = _engine()
    env.reset()
    eng.step_id = 5
    q = eng._params(10)
    worst = 0.0
    for layer in range(3):
        for side in (0, 1):
            for width in (1, 47, 48, 64, 104):
                e = _eps(env, q, layer, side, width).cpu()
                assert bool(torch.isfinite(e).all())
                for d in range(ED):
                    want = noisy_normals_host(SEED, 5, d // 2, SEATS[d % 2], layer, side, width)
                    worst = max(worst, float(np.abs(_normal(e[d]).double().numpy() - want).max()))
    print("sn_noisy_eps |n - n_host| max", worst, "bound", 2.0 ** -16)
    assert worst <= 2.0 ** -16


def test_eps_rows_depend_on_every_key_field_and_on_nothing_else():
    env, eng = _engine()
    env.reset()
    eng.step_id = 5
    q = eng._params(10)
    base = _eps(env, q, 1, 0, 64)
    assert torch.equal(base, _eps(env, q, 1, 0, 64))  # the same key, the same rows
    assert torch.equal(base[:, :47], _eps(env, q, 1, 0, 47))
    eng.step_id = 6
    assert not bool((base == _eps(env, eng._params(10), 1, 0, 64)).all(dim=1).any())  # the step
    assert not bool((base == _eps(env, q, 2, 0, 64)).all(dim=1).any())  # the layer
    assert not bool((base == _eps(env, q, 1, 1, 64)).all(dim=1).any())  # the side
    rows = base.cpu()
    assert len({tuple(r.tolist()) for r in rows}) == ED  # every seat of every game its own row
    # the hand size and the position take no part
    eng.step_id = 5
    env.step()
    assert torch.equal(base, _eps(env, eng._params(7), 1, 0, 64))
    # two handles of 8 games, the second from game 8 on: the 16-game rows
    for half in (0, 1):
        env8, eng8 = _engine(games=8, game_offset=8 * half)
        env8.reset()
        eng8.step_id = 5
        got = _eps(env8, eng8._params(10), 1, 0, 64, D=ED // 2)
        assert torch.equal(got.cpu(), rows[half * (ED // 2): (half + 1) * (ED // 2)]), half


def test_eps_with_a_decision_list():
    env, eng = _engine()
    env.reset()
    eng.step_id = 2
    full = _eps(env, eng._params(10), 0, 1, 48).cpu()
    dec = torch.tensor([g * N + p for g, p in ((3, 2), (0, 0), (15, 2))], dtype=torch.int32)
    eng.use_decisions(dec)
    got = _eps(env, eng._params(10), 0, 1, 48, D=3).cpu()
    assert torch.equal(got, full[[3 * 2 + 1, 0, 15 * 2 + 1]])


# ---------------------------------------------------------------- sn_noisy_scale
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_scale_is_the_fp32_product_rounded_once(dtype):
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.dqn import noisy_tag

    env, eng = _engine()
    env.reset()
    q = eng._params(10)
    L, st, dev = nat.lib(), env._stream(), env.device
    bf16 = int(dtype == torch.bfloat16)
    g = torch.Generator().manual_seed(4)
    for width, x_stride, out_stride, off in ((48, 48, 48, 0), (64, 64, 128, 64), (47, 48, 48, 0), (41, 41, 43, 1),
                                             (104, 112, 104, 0), (1, 1, 1, 0)):
        e = _eps(env, q, 2, 0, width)
        for ones in (True, False):
            x = torch.ones((ED, x_stride)) if ones else torch.randn((ED, x_stride), generator=g) * 7.0
            x = x.to(dev, dtype)
            buf = torch.full((ED, out_stride), 77.0, dtype=dtype, device=dev)
            out = ctypes.c_void_p(buf.data_ptr() + off * buf.element_size())
            width_out = min(width, out_stride - off)
            nat.check(L.sn_noisy_scale(env._h, ctypes.byref(q), noisy_tag(2, 0), nat.ptr(x), x_stride, width_out, bf16,
                                       out, out_stride, st), "sn_noisy_scale")
            want = (x[:, :width_out].float() * e[:, :width_out]).to(dtype)
            assert torch.equal(buf[:, off: off + width_out], want), (width, ones)
            if ones and dtype == torch.float32:
                assert torch.equal(buf[:, off: off + width_out], e[:, :width_out])
            rest = torch.ones((out_stride,), dtype=torch.bool)
            rest[off: off + width_out] = False
            assert bool((buf[:, rest.to(dev)] == 77.0).all())  # nothing outside the width
    x = torch.ones((ED, 48), device=dev, dtype=dtype)
    for tag, xs, width, os_ in ((noisy_tag(2, 0), 48, 0, 48), (noisy_tag(2, 0), 47, 48, 48), (noisy_tag(2, 0), 48, 48, 47),
                                (0xFFF00 + 128, 48, 48, 48), (0xFFEFF, 48, 48, 48)):
        assert L.sn_noisy_scale(env._h, ctypes.byref(q), tag, nat.ptr(x), xs, width, bf16, nat.ptr(x), os_, st) == \
            nat.SN_EINVAL
    assert L.sn_noisy_scale(None, ctypes.byref(q), noisy_tag(2, 0), nat.ptr(x), 48, 48, bf16, nat.ptr(x), 48, st) == \
        nat.SN_EINVAL


# ---------------------------------------------------------------- sn_noisy_combine
def _combine(env, q, layer, mu, sg, col0, width, sigma_b, relu, out):
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.dqn import noisy_tag

    return nat.lib().sn_noisy_combine(env._h, ctypes.byref(q), noisy_tag(layer, 1), nat.ptr(mu), nat.ptr(sg),
                                      mu.stride(0), col0, width, nat.ptr(sigma_b), relu, nat.ptr(out), env._stream())


def test_combine_is_the_torch_fp32_expression_bit_for_bit():
    env, eng = _engine()
    env.reset()
    eng.step_id = 9
    q = eng._params(10)
    dev = env.device
    g = torch.Generator().manual_seed(6)
    for stride, col0, width in ((64, 0, 64), (112, 0, 104), (112, 104, 1), (41, 0, 41), (43, 1, 41), (40, 0, 24),
                                (48, 7, 40)):
        e = _eps(env, q, 1, 1, width)
        mu = (torch.randn((ED, stride), generator=g) * 5.0).to(dev)
        sg = (torch.randn((ED, stride), generator=g) * 3.0).to(dev)
        sb = torch.randn((stride,), generator=g).to(dev)
        cols = slice(col0, col0 + width)
        for relu in (0, 1):
            want = mu[:, cols] + e * (sg[:, cols] + sb[cols])
            if relu:
                want = want.clamp_min(0)
            out = torch.full((ED, stride), -77.0, device=dev)
            assert _combine(env, q, 1, mu, sg, col0, width, sb, relu, out) == 0
            assert torch.equal(out[:, cols], want), (stride, col0, width, relu)
            outside = torch.ones((stride,), dtype=torch.bool, device=dev)
            outside[cols] = False
            assert bool((out[:, outside] == -77.0).all())
            if relu:
                assert bool((want == 0).any()) and bool((want > 0).any())
            inplace = mu.clone()  # out = mu
            assert _combine(env, q, 1, inplace, sg, col0, width, sb, relu, inplace) == 0
            assert torch.equal(inplace[:, cols], want) and torch.equal(inplace[:, outside], mu[:, outside])
        zero, zb = torch.zeros_like(sg), torch.zeros_like(sb)
        out = torch.full((ED, stride), -77.0, device=dev)
        assert _combine(env, q, 1, mu, zero, col0, width, zb, 0, out) == 0
        assert torch.equal(out[:, cols], mu[:, cols])  # no noise term: mu exactly


def test_combine_rejects_what_it_cannot_do():
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.dqn import noisy_tag

    env, eng = _engine()
    env.reset()
    q = eng._params(10)
    dev, L, st = env.device, nat.lib(), env._stream()
    mu = torch.zeros((ED, 64), device=dev)
    sb = torch.zeros((64,), device=dev)
    args = lambda tag, col0, width: (ctypes.byref(q), tag, nat.ptr(mu), nat.ptr(mu), 64, col0, width, nat.ptr(sb), 0,
                                     nat.ptr(mu), st)
    ok = noisy_tag(0, 1)
    assert L.sn_noisy_combine(env._h, *args(ok, 0, 64)) == nat.SN_OK
    assert L.sn_noisy_combine(env._h, *args(noisy_tag(63, 1), 0, 64)) == nat.SN_OK
    for tag, col0, width in ((ok, 0, 0), (ok, 0, -3), (ok, 1, 64), (ok, 64, 1), (ok, -1, 8), (ok, 0, 65),
                             (0xFFF00 + 2 * 64, 0, 64), (0xFFF00 + 2 * 64 + 1, 0, 64), (0xFFFFE, 0, 64), (0, 0, 64)):
        assert L.sn_noisy_combine(env._h, *args(tag, col0, width)) == nat.SN_EINVAL, (tag, col0, width)
    assert L.sn_noisy_combine(None, *args(ok, 0, 64)) == nat.SN_EINVAL
    out = torch.zeros((ED, 8), device=dev)
    assert L.sn_noisy_eps(None, ctypes.byref(q), ok, 8, nat.ptr(out), st) == nat.SN_EINVAL
    assert L.sn_noisy_eps(env._h, ctypes.byref(q), ok, 0, nat.ptr(out), st) == nat.SN_EINVAL
    assert L.sn_noisy_eps(env._h, ctypes.byref(q), 0xFFF00 + 128, 8, nat.ptr(out), st) == nat.SN_EINVAL
    assert not bool(mu.any()) and not bool(out.any())


# ---------------------------------------------------------------- the engine against the reference's formula
def _error_bound(net, x, eps):
    """the running error bound of the engine's fp32 forward against the exact formula, in float64, for any
    summation order: per layer, out = (W h + b) + e_out o (S (h o e_in) + s_b) takes at most K + 4 roundings per
    output (the scaling, K - 1 additions and the product roundings of a dot product counted as K, the bias, the
    sigma bias, the product with e_out, the final sum), each at most u = 2^-24 of the sum of absolute values
    M = |W||h| + |b| + |e_out| o (|S| (|h| o |e_in|) + |s_b|); an input error d propagates as
    |W| d + |e_out| o (|S| (d o |e_in|)); ReLU does not grow it.  Returns (the formula's value, the bound) per head."""
    from rl_6_nimmt.dqn import noisy_linears

    mlp = getattr(net, "mlp", net)
    lin = noisy_linears(net)
    n_lat = len(lin) - len(mlp.head_nets)

    def layer(l, h, d):
        m = lin[l]
        W, S = m.weight.detach().double().cpu(), m.sigma_weight.detach().double().cpu()
        b, sb = m.bias.detach().double().cpu(), m.sigma_bias.detach().double().cpu()
        e_in, e_out = eps[l][0].double(), eps[l][1].double()
        K = W.shape[1]
        y = h @ W.t() + b + e_out * ((h * e_in) @ S.t() + sb)
        mag = (h.abs() + d) @ W.abs().t() + b.abs() + e_out.abs() * (((h.abs() + d) * e_in.abs()) @ S.abs().t() + sb.abs())
        gamma = (K + 4) * U / (1 - (K + 4) * U)
        return y, d @ W.abs().t() + e_out.abs() * ((d * e_in.abs()) @ S.abs().t()) + gamma * mag

    h, d = x.double(), torch.zeros_like(x, dtype=torch.float64)
    for l in range(n_lat):
        h, d = layer(l, h, d)
        h = h.clamp_min(0)
    return [layer(n_lat + k, h, d) for k in range(len(mlp.head_nets))]


@pytest.mark.parametrize("hidden", [(64,), (24, 40)])
@pytest.mark.parametrize("duelling", [False, True])
def test_engine_q_is_the_reference_formula_under_each_rows_own_noise(duelling, hidden):
    from rl_6_nimmt.dqn import noisy_forward_host, noisy_linears

    env, eng = _engine(duelling=duelling, hidden=hidden)
    assert eng.noisy and eng.duelling == duelling
    with torch.no_grad():
        for m in noisy_linears(eng.actor):  # sigmas of their own, as after training
            m.sigma_weight.mul_(0.5 + torch.rand_like(m.sigma_weight))
            m.sigma_bias.mul_(0.5 + torch.rand_like(m.sigma_bias))
    env.reset()
    eng.step_id = 4
    q = eng._params(10)
    x = env.obs()[:, SEATS].reshape(ED, 47).float().cpu()
    hands = env.hands()[:, SEATS].reshape(ED, 10).long().cpu()
    acts = eng.decide(10)[:, SEATS].reshape(ED).long().cpu()
    assert eng.step_id == 5 and eng.eps_used == 0.0
    handed = eng.q_handed.cpu()
    assert handed.shape == (ED, 112) and handed.dtype == torch.float32
    lin = noisy_linears(eng.actor)
    eps = [(_eps(env, q, l, 0, m.in_features).cpu(), _eps(env, q, l, 1, m.out_features).cpu()) for l, m in enumerate(lin)]
    (want,) = noisy_forward_host(eng.actor, x, eps)
    heads = _error_bound(eng.actor, x, eps)
    if duelling:
        (V, dV), (A, dA) = heads
        assert float((V + (A - A.mean(-1, keepdim=True)) - want).abs().max()) <= 1e-9 * float(want.abs().max())
        gA, gV = handed[:, :104].double(), handed[:, 104:105].double()
        got = gV + (gA - gA.mean(-1, keepdim=True))
        tol = dV + dA + dA.mean(-1, keepdim=True) + 2.0 ** -17 * (V.abs() + 2 * A.abs().max(dim=1, keepdim=True).values)
    else:
        ((Q, tol),) = heads
        assert float((Q - want).abs().max()) <= 1e-9 * float(want.abs().max())
        got = handed[:, :104].double()
    err = (got - want).abs()
    print("engine |Q - formula| max", float(err.max()), "bound min", float(tol.min()), "max", float(tol.max()),
          "worst err / bound", float((err / tol).max()))
    assert bool((err <= tol).all())
    assert float(tol.max()) < 0.05 * float(want.abs().max())  # the bound says something
    # the noise matters: the noiseless net is far outside the bound
    zero = [(torch.zeros_like(a), torch.zeros_like(b)) for a, b in eps]
    assert float((noisy_forward_host(eng.actor, x, zero)[0] - want).abs().max()) > 100 * float(tol.max())
    # and the value the select kernel reports is that Q at its card
    rows = torch.arange(ED)
    verr = (eng.value[:ED].cpu().double() - want[rows, acts]).abs()
    assert bool((verr <= tol.expand(ED, 104)[rows, acts]).all())
    assert bool((hands == acts[:, None]).any(dim=1).all())


# ---------------------------------------------------------------- sigma zero: the plain engine, exactly
@pytest.mark.parametrize("hidden", [(64,), (24, 40)])
@pytest.mark.parametrize("duelling", [False, True])
def test_with_zero_sigmas_the_noisy_engine_is_the_plain_engine(duelling, hidden):
    from rl_6_nimmt.dqn import BatchedDQN
    from rl_6_nimmt.utils.nets import DuellingDQNNet, MultiHeadedMLP
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env, eng = _engine(duelling=duelling, hidden=hidden, eps_func=lambda e: 1.0)
    sd = {}
    for k, v in eng.actor.state_dict().items():
        if "sigma_" in k:
            v.zero_()
        elif "epsilon_" not in k:
            sd[k] = v.clone()
    if duelling:
        plain = DuellingDQNNet(47, hidden_sizes=hidden, out_size=104, activation=nn.ReLU())
    else:
        plain = MultiHeadedMLP(47, hidden_sizes=hidden, head_sizes=(104,), activation=nn.ReLU(), head_activations=(None,))
    plain.load_state_dict(sd, strict=True)
    env2 = VecSechsNimmtEnv(EB, N, seed=SEED)
    eng2 = BatchedDQN(env2, plain.to(env2.device), seats_mask=MASK, seed=SEED, net_dtype=torch.float32, capacity=1024,
                      eps_func=lambda e: 0.0)
    assert eng.noisy and not eng2.noisy
    env.reset()
    env2.reset()
    assert torch.equal(env.hands(), env2.hands())
    for _ in range(2):  # the same position twice: the step advances, the noise has nothing to act on
        a, b = eng.decide(10), eng2.decide(10)
        assert torch.equal(a[:, SEATS], b[:, SEATS])
        assert torch.equal(eng.value[:ED], eng2.value[:ED]) and bool(torch.isfinite(eng.value[:ED]).all())
        assert not bool((eng.value[:ED] == -1).any())
        assert bool(torch.isfinite(eng.q_handed).all())


# ---------------------------------------------------------------- selection
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("duelling", [False, True])
def test_engine_plays_the_first_argmax_of_its_own_noisy_q(duelling, dtype):
    """plain net: exact.  Duelling: the kernel forms Q = V + (A - mean A) in its own summation order, so the value
    is held to test_select_duel_on_random_heads_within_the_summation_bound's tolerance 2^-17 (|V| + 2 max|A|) and
    the card is checked where the two best legal Q lie 16 tolerances apart."""
    for eps_func in (None, lambda e: 1.0):
        env, eng = _engine(duelling=duelling, net_dtype=dtype, eps_func=eps_func)
        env.reset()
        hands = env.hands()[:, SEATS].reshape(ED, 10).long()
        rows = torch.arange(ED, device=env.device)
        seen = []
        for _ in range(2):
            acts = eng.decide(10)[:, SEATS].reshape(ED).long()
            assert eng.eps_used == 0.0
            out = eng.q_handed
            assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
            if duelling:
                A, V = out[:, :104], out[:, 104:105]
                Q = V + (A - A.mean(-1, keepdim=True))
                tol = 2.0 ** -17 * (V.abs()[:, 0] + 2 * A.abs().max(dim=1).values)
            else:
                Q, tol = out[:, :104], torch.zeros((ED,), device=env.device)
            legal_q = Q[rows[:, None], hands]
            best = legal_q.argmax(dim=1)  # the first maximum
            top = legal_q.sort(dim=1, descending=True).values
            clear = (top[:, 0] - top[:, 1]) >= 16 * tol
            assert int(clear.sum()) >= (ED if not duelling else ED // 2)
            assert torch.equal(acts[clear], hands[rows, best][clear])
            assert torch.equal(eng.best_index[:ED].long()[clear], best[clear])
            assert bool(((eng.value[:ED] - top[:, 0]).abs() <= tol).all())
            assert not bool((eng.value[:ED] == -1).any())
            seen.append(Q.clone())
        assert bool((seen[0] != seen[1]).any(dim=1).any())  # the step advanced: other noise on the same position
        assert eng.eps_history == [] and eng.current_eps() == 0.0


# ---------------------------------------------------------------- learning
def test_learn_moves_the_sigmas_the_target_follows_and_the_device_copy_is_rebuilt():
    from rl_6_nimmt.dqn import noisy_linears

    tau = 0.125
    env, eng = _engine(seed=5, duelling=True, target=True, prioritised=True, n_steps=3, minibatch=64, updates=1,
                       retrain_interval=1, tau=tau)
    net, tgt = eng.actor, eng.target_net
    with torch.no_grad():
        for p in tgt.parameters():
            p.add_(0.05 * torch.randn_like(p))
    eng.play_episode(record=True)
    assert len(eng.replay) == 10 * ED > 64 and eng.eps_history == [0.0]
    local0 = [p.detach().clone() for p in net.parameters()]
    target0 = [p.detach().clone() for p in tgt.parameters()]
    device_net = eng.sync_net()
    assert eng.sync_net() is device_net  # nothing changed: kept
    losses = eng.learn(torch.optim.Adam(net.parameters(), lr=1e-2))
    assert len(losses) == 1 and bool(torch.isfinite(losses[0]))
    for m in noisy_linears(net):
        assert m.sigma_weight.grad is not None and bool((m.sigma_weight.grad != 0).any())
        assert m.sigma_bias.grad is not None
    names = [k for k, _ in net.named_parameters()]
    for k, p, p0 in zip(names, net.parameters(), local0):
        assert not torch.equal(p.detach(), p0), k  # sigma_weight and sigma_bias of every layer among them
    assert sum("sigma_weight" in k for k in names) == 3
    for k, t, l0, t0 in zip(names, tgt.parameters(), local0, target0):  # the soft update precedes the optimiser step
        assert torch.equal(t.detach(), tau * l0 + (1 - tau) * t0), k
    env.reset()
    eng.decide(10)
    rebuilt = eng._net
    assert rebuilt is not device_net
    lin = noisy_linears(net)
    assert torch.equal(rebuilt.layers[0][2][:, :47], lin[0].sigma_weight.detach())
    assert torch.equal(rebuilt.head_s[64:128, :104], lin[2].sigma_weight.detach().t())  # A: the second head's block
    assert torch.equal(rebuilt.head_s[:64, 104], lin[1].sigma_weight.detach()[0])  # V
    assert not bool(rebuilt.head_s[:64, :104].any()) and not bool(rebuilt.head_s[64:, 104:].any())


def test_loss_terms_of_the_noisy_d3qn_prb_nstep_engine_follow_the_dropin():
    """test_loss_terms_of_the_d3qn_prb_nstep_engine_follow_the_dropin with the torch generator seeded before the
    forwards: Noisy_D3QN_PRB_NStep._learn forwards the local net on the states, then (DDQNAgent._calc_reward) the
    target net and the local net on the next states -- one noise draw per forward, in that order"""
    from rl_6_nimmt.dqn import bellman_target_host, unpack_rows_nstep_host

    gamma = 0.97
    env, eng = _engine(seed=5, duelling=True, target=True, prioritised=True, n_steps=3, minibatch=64, updates=1,
                       gamma=gamma)
    net, tgt = eng.actor, eng.target_net
    with torch.no_grad():
        for p in tgt.parameters():
            p.add_(0.05 * torch.randn_like(p))
    eng.play_episode(record=True)
    u = torch.rand(64, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    batch = eng.sample_batch(u=u)
    torch.manual_seed(31)
    q_eval, target, weights, loss = eng.loss_terms(batch)
    s, s2, a, r, nd = (x.to(env.device) for x in unpack_rows_nstep_host(batch["rows"].cpu()))
    assert not torch.equal(r, r.round())
    torch.manual_seed(31)
    want_eval = torch.squeeze(net(s[:, :47])[0].gather(1, a.view(-1, 1)))
    with torch.no_grad():
        qt = tgt(s2[:, :47])[0]
        qn = net(s2[:, :47])[0]
    want_target = bellman_target_host(qn, qt, r, nd, gamma ** 3)
    assert target.dtype == torch.float32 and torch.equal(target, want_target)
    assert torch.equal(q_eval, want_eval)
    assert weights.dtype == torch.float32 and torch.equal(weights, batch["weights"].float())
    want_loss = (weights * (want_eval - want_target) ** 2).mean()
    assert loss.dtype == torch.float32 and torch.equal(loss, want_loss)
    torch.manual_seed(32)  # other noise, another loss: the minibatch forward is noisy
    assert not torch.equal(eng.loss_terms(batch)[3], loss)


# ---------------------------------------------------------------- the league
KINDS = ["noisy_dqn", "noisy_d3qn", "noisy_d3qn_prb_nstep"]


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


def _noisy_agent(kind, **kw):
    from rl_6_nimmt.agents import DQN_NOISY_AGENTS

    if "nstep" in kind:
        kw["n_steps"] = 3
    return DQN_NOISY_AGENTS[kind](history_length=1000, **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_league_seats_and_trains_a_noisy_agent(kind, monkeypatch):
    from rl_6_nimmt.dqn import BatchedDQN
    from rl_6_nimmt.league import T_STEPS, decode_seats
    from rl_6_nimmt.utils.nets import DuellingDQNNet

    losses = []
    learn = BatchedDQN.learn

    def learn_rec(self, optimizer):
        out = learn(self, optimizer)
        losses.extend(out)
        return out

    monkeypatch.setattr(BatchedDQN, "learn", learn_rec)
    torch.manual_seed(2)
    agent = _noisy_agent(kind, minibatch=64)
    before = {k: p.detach().clone() for k, p in agent.dqn_net_local.named_parameters()}
    t = _league(agent, train=True)
    rec = t.play_games(1)
    rec = torch.cat((rec, t.play_games(1)), dim=0)  # an illegal move of the engine would raise in the round
    eng = t.engines["Q"]
    assert isinstance(eng, BatchedDQN) and eng.noisy and eng.prioritised == ("prb" in kind)
    assert (eng.target_net is not None) == (kind != "noisy_dqn")
    assert eng.duelling == isinstance(agent.dqn_net_local, DuellingDQNNet) == (kind != "noisy_dqn")
    assert eng.n_steps == (3 if "nstep" in kind else 1)
    assert eng.minibatch == 256 and eng.updates == T_STEPS and eng.capacity == 4096
    k, ids = decode_seats(rec[..., 0], 4)
    seated = (ids == 2).sum(dim=(1, 2)).tolist()  # "Q" is the third active agent
    assert min(seated) > 0
    assert t.env.pipe_errors() == 0
    assert (eng.replay.pointer, len(eng.replay)) == _model_counters([10 * s for s in seated], eng.capacity)
    assert len(losses) == 2 * T_STEPS and all(bool(torch.isfinite(x)) for x in losses)
    after = dict(agent.dqn_net_local.named_parameters())
    assert all(not torch.equal(after[k].detach().cpu(), v) for k, v in before.items() if "sigma_weight" in k)
    assert any(not torch.equal(after[k].detach().cpu(), v) for k, v in before.items() if k.endswith(".weight"))
    assert t.optimizer_steps["Q"] == 2 * T_STEPS and eng.update_count == 2 * T_STEPS
    assert eng.eps_history == [0.0, 0.0]
    t.close()


@pytest.mark.parametrize("kind", KINDS)
def test_league_with_a_noisy_agent_is_deterministic(kind):
    torch.manual_seed(3)
    agent = _noisy_agent(kind)
    recs = []
    for _ in range(2):
        t = _league(copy.deepcopy(agent), train=False, seed=22)
        recs.append(t.play_games(2).cpu())
        assert len(t.engines["Q"].replay) == 0 and t.engines["Q"].eps_history == [0.0, 0.0]
        t.close()
    assert torch.equal(recs[0], recs[1])


# ---------------------------------------------------------------- the drop-ins on golden F18
@pytest.mark.parametrize("si", range(len(SPEC["sessions"])))
def test_dropin_noisy_agents_replay_reference_training_sessions(si):
    """test_dropin_variants_replay_reference_training_sessions' comparisons and tolerances on the noisy
    sessions: torch's CPU generator, seeded once, drives the initial weights and every noise draw"""
    from rl_6_nimmt import GameSession
    from rl_6_nimmt.agents import DQN_NOISY_AGENTS, DrunkHamster

    sess = SPEC["sessions"][si]
    W = np.load(os.path.join(GOLDEN, "dqn_noisy_weights.npz"))
    cls = {c.__name__: c for c in DQN_NOISY_AGENTS.values()}[sess["agent"]]
    torch.manual_seed(sess["seed"])
    agent = cls(**sess["kwargs"])
    agents = [agent] + [DrunkHamster() for _ in range(3)]
    agent.train()

    def weights():
        return {k: v for k, v in agent.state_dict().items() if ".epsilon_" not in k}

    for k, v in weights().items():  # the target net starts as the local net's copy: stored once
        assert np.array_equal(v.numpy(), W[f"s{si}_init_{k.replace('dqn_net_target.', 'dqn_net_local.', 1)}"]), k
    steps, losses, per_idx = [], [], []
    fwd, lrn = agent.forward, agent.learn

    def fwd_rec(state, **k):
        act, info = fwd(state, **k)
        assert set(info) == {"value"}
        steps.append([int(act), float(info["value"])])
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
    assert np.array_equal(got[:, 0], W[f"s{si}_actions"].astype(np.float64))  # every move
    assert np.allclose(got[:, 1], W[f"s{si}_values"], rtol=0, atol=1e-3)
    assert len(losses) == len(W[f"s{si}_losses"])
    assert np.allclose(losses, W[f"s{si}_losses"], rtol=1e-3, atol=1e-4)
    if prb:
        assert per_idx == W[f"s{si}_per_idx"].tolist()
        assert agent.history.beta == sess["beta"] and len(agent.history) == sess["len"]
        assert agent.history.total_priority == pytest.approx(sess["total_priority"], rel=1e-3)
    for k, v in weights().items():
        d = np.abs(v.detach().numpy() - W[f"s{si}_final_{k}"])
        assert np.mean(d <= 1e-4) >= 0.5 and d.max() <= 3e-3 * sess["games"], (k, d.max())
