"""Batched DQN family on one MI355X: the engine that seats DQNVanilla,
DDQNAgent, DQN_PRBAgent, DDQN_PRBAgent, their duelling and n-step variants
(DuellingDQNAgent, DuellingDDQNAgent, DuellingDDQN_PRBAgent, DQN_NStep_Agent,
D3QN_PRB_NStep) and the noisy ones (Noisy_DQN, Noisy_D3QN,
Noisy_D3QN_PRB_NStep; agents/dqn.py; reference agents/dqn.py:42-441) in the
batched league.

Every deciding seat of every game acts together.  Per decision batch:
    sn_dqn_obs     the raw _create_states rows (env.py:174-212), as int8 replay
                   rows and as the Q net's float input
    Q net          MultiHeadedMLP(47, hidden, (104,)) forward on PyTorch-ROCm
                   (a device copy in net_dtype, its input weight padded with a
                   zero column so the 48-wide rows go in unsliced)
    sn_dqn_select  epsilon-greedy over the hand (_action_selection), Philox
A duelling net (utils.nets.DuellingDQNNet) runs as the FusedMLP of its `mlp`
with the head rows ordered [A | V | pad]: one GEMM, and sn_dqn_select_duel
forms Q = V + (A - mean A) per decision from that output in place.
At the end of an episode sn_dqn_pack turns the staged observations, actions
and rewards into 112-byte transition rows, stored in a DevicePER(capacity,
112) -- for the uniform variants too: they draw slots and `gather`.  With
n_steps > 1 sn_dqn_pack_nstep writes the n-step rows instead (the same T rows
per decider; the return as f32 in the row's spare bytes), sn_dqn_unpack_nstep
reads that return, and the targets discount by gamma ** n_steps.

Learning (`learn`, once per round): `updates` minibatches of `minibatch`
rows; per minibatch sample / gather -> sn_dqn_unpack -> fp32 forwards of
state and next_state on the agent's own module -> sn_dqn_target (both
Bellman targets) -> loss -> (PER) priorities written back -> (DDQN) soft
update of the target net every `retrain_interval` updates -> optimiser step.

Kept from the reference: the reward a transition carries is the PREVIOUS
step's (GameSession's one-step lag, play.py:29,57,72: r_0 = 0 and the last
step's reward never reaches the agent; REINFORCE here keeps the same lag),
done is set at the last step only, the length gate `len(replay) > minibatch`,
the maximum over all 104 actions, unmasked, in the targets.
Different by construction: exploration draws are Philox, not Python's
`random` (parity unpinned, like the other engines' samplers), a round
trains on `updates` x `minibatch` rows, not 10 x 64 per game, and the n-step
targets and losses are fp32 (the reference's are float64: its n-step reward
is a Python float).  A clone's engine inherits its parent's replay and
counters (`inherit`).

A noisy net (utils.nets.NoisyFactorizedLinear layers, plain or duelling:
`BatchedDQN.noisy`) explores by its noise, and every decision row has its
own: per layer  y = (x W^T + b) + e_out o ((x o e_in) S^T + s_b)  with the
row's e_in / e_out from a Philox stream on the device -- sn_noisy_scale, the
plain GEMM, a sigma GEMM of the same shape, sn_noisy_combine; no effective
weights are rebuilt.  Selection is the select kernels' greedy branch (eps 0).
The noise is keyed by (seed, step, global game, seat, layer, side, unit) and
drawn in training and evaluation alike; `learn` runs the agent's own module
(one torch.randn sample per minibatch forward, as the reference's _learn).
`noisy_eps_host` is the float64 model of the noise law, `noisy_forward_host`
the reference's formula in float64 on given noise rows.

`pack_rows_host`, `unpack_rows_host`, `bellman_target_host`,
`pack_rows_nstep_host`, `unpack_rows_nstep_host` and `duelling_q_host` are
the torch models of the kernels (they run on any device); the tests hold the
kernels to them.
"""
import copy
import ctypes

import numpy as np
import torch
from torch import nn

from . import _native as nat
from .engine import (BatchedEngine, FusedMLP, ctypes_ref, decision_words_host,
                     philox4x32_10_host)  # noqa: F401  (philox4x32_10_host: re-exported)
from .replay import DevicePER

T_STEPS = 10
OBS = 48  # 47 observation values + one zero pad
NUM_ACTIONS = 104
ROW_BYTES = 112
OFF_STATE, OFF_NEXT_STATE, OFF_ACTION, OFF_DONE, OFF_HAND, OFF_REWARD = 0, 48, 96, 97, 98, 100
OFF_TERMS, OFF_RETURN = 99, 104  # the n-step rows: rewards summed, the return as f32


# ---------------------------------------------------------------- host models of the kernels
def pack_rows_host(obs, actions, rewards_seen):
    """sn_dqn_pack in torch.  obs int8 [T+1, D, 47 or 48], actions [T, D],
    rewards_seen [T, D] -> uint8 [T*D, 112], t-major then decider."""
    obs = torch.as_tensor(obs).to(torch.int8)
    actions, rewards_seen = torch.as_tensor(actions), torch.as_tensor(rewards_seen)
    T, D = actions.shape
    if obs.shape[-1] == OBS - 1:
        obs = torch.cat((obs, torch.zeros_like(obs[..., :1])), dim=-1)
    assert obs.shape == (T + 1, D, OBS)
    rows = torch.zeros((T, D, ROW_BYTES), dtype=torch.uint8, device=obs.device)
    rows[..., OFF_STATE: OFF_STATE + OBS] = obs[:-1].contiguous().view(torch.uint8)
    rows[..., OFF_NEXT_STATE: OFF_NEXT_STATE + OBS] = obs[1:].contiguous().view(torch.uint8)
    rows[..., OFF_ACTION] = actions.to(obs.device).to(torch.uint8)
    rows[T - 1, :, OFF_DONE] = 1
    rows[..., OFF_HAND] = (obs[:-1, :, :10] >= 0).sum(dim=-1).to(torch.uint8)
    rew = rewards_seen.to(obs.device).to(torch.int32).contiguous()
    rows[..., OFF_REWARD: OFF_REWARD + 4] = rew.view(torch.uint8).reshape(T, D, 4)  # little endian, as the GPU's
    return rows.reshape(T * D, ROW_BYTES)


def unpack_rows_host(rows):
    """sn_dqn_unpack in torch: uint8 [n, 112] -> (states f32 [n, 48],
    next_states f32 [n, 48], action int64 [n], reward f32 [n], not_done f32 [n])"""
    rows = torch.as_tensor(rows).reshape(-1, ROW_BYTES)
    states = rows[:, OFF_STATE: OFF_STATE + OBS].contiguous().view(torch.int8).float()
    nxt = rows[:, OFF_NEXT_STATE: OFF_NEXT_STATE + OBS].contiguous().view(torch.int8).float()
    action = rows[:, OFF_ACTION].to(torch.int64)
    reward = rows[:, OFF_REWARD: OFF_REWARD + 4].contiguous().view(torch.int32).reshape(-1).float()
    not_done = 1.0 - rows[:, OFF_DONE].float()
    return states, nxt, action, reward, not_done


def bellman_target_host(q_next_local, q_next_target, reward, not_done, gamma):
    """sn_dqn_target in torch (fp32): DQNVanilla._calc_reward when
    q_next_target is None, else DDQNAgent._calc_reward.  The Q tensors may be
    wider than 104 columns (a padded head); only the first 104 count."""
    with torch.no_grad():
        q = q_next_local[:, :NUM_ACTIONS]
        if q_next_target is None:
            best = q.max(dim=-1).values
        else:
            pick = torch.argmax(q, dim=-1)
            best = q_next_target[torch.arange(q.shape[0], device=q.device), pick]
        return reward + gamma * (best * not_done)


def gamma_powers(gamma):
    """gamma ** i for i < T_STEPS as CPython computes them (the reference's `self.gamma ** i`)"""
    return [float(gamma) ** i for i in range(T_STEPS)]


def nstep_returns_host(rewards_seen, n, gamma):
    """float64 [T, D]: row s = sum([r[s + i] * gamma ** i for i in range(min(n, T - s))]), summed left to
    right from 0 as Python's sum does (DQN_NStep_Agent._store / _finish_episode)"""
    r = torch.as_tensor(rewards_seen).to(torch.float64)
    T = r.shape[0]
    gpow = gamma_powers(gamma)
    out = torch.zeros_like(r)
    for s in range(T):
        acc = torch.zeros_like(r[s])
        for i in range(min(int(n), T - s)):
            acc = acc + r[s + i] * gpow[i]
        out[s] = acc
    return out


def pack_rows_nstep_host(obs, actions, rewards_seen, n, gamma):
    """sn_dqn_pack_nstep in torch: the rows DQN_NStep_Agent stores for an episode of T learn calls, in store
    order.  Row s: state obs[s], next_state obs[min(s + n, T)], done = (s + n > T) or (n == 1 and s == T - 1),
    byte 99 = m = min(n, T - s), bytes 100-103 r_s (int32), bytes 104-107 the n-step return
    (nstep_returns_host) rounded once to float32.  T <= T_STEPS."""
    obs = torch.as_tensor(obs).to(torch.int8)
    actions, rewards_seen = torch.as_tensor(actions), torch.as_tensor(rewards_seen)
    T, D = actions.shape
    n = int(n)
    assert 1 <= T <= T_STEPS and n >= 1
    if obs.shape[-1] == OBS - 1:
        obs = torch.cat((obs, torch.zeros_like(obs[..., :1])), dim=-1)
    assert obs.shape == (T + 1, D, OBS)
    dev = obs.device
    start = torch.arange(T, device=dev)
    nxt = torch.clamp(start + n, max=T)
    rows = torch.zeros((T, D, ROW_BYTES), dtype=torch.uint8, device=dev)
    rows[..., OFF_STATE: OFF_STATE + OBS] = obs[:-1].contiguous().view(torch.uint8)
    rows[..., OFF_NEXT_STATE: OFF_NEXT_STATE + OBS] = obs[nxt].contiguous().view(torch.uint8)
    rows[..., OFF_ACTION] = actions.to(dev).to(torch.uint8)
    done = (start + n > T) | ((start == T - 1) & (n == 1))
    rows[..., OFF_DONE] = done.to(torch.uint8)[:, None]
    rows[..., OFF_HAND] = (obs[:-1, :, :10] >= 0).sum(dim=-1).to(torch.uint8)
    rows[..., OFF_TERMS] = (nxt - start).to(torch.uint8)[:, None]
    rew = rewards_seen.to(dev).to(torch.int32).contiguous()
    rows[..., OFF_REWARD: OFF_REWARD + 4] = rew.view(torch.uint8).reshape(T, D, 4)
    ret = nstep_returns_host(rew, n, gamma).to(torch.float32).contiguous()
    rows[..., OFF_RETURN: OFF_RETURN + 4] = ret.view(torch.uint8).reshape(T, D, 4)
    return rows.reshape(T * D, ROW_BYTES)


def unpack_rows_nstep_host(rows):
    """sn_dqn_unpack_nstep in torch: unpack_rows_host with reward = the float32 n-step return at byte 104"""
    rows = torch.as_tensor(rows).reshape(-1, ROW_BYTES)
    states, nxt, action, _, not_done = unpack_rows_host(rows)
    reward = rows[:, OFF_RETURN: OFF_RETURN + 4].contiguous().view(torch.float32).reshape(-1)
    return states, nxt, action, reward, not_done


def duelling_q_host(V, A):
    """DuellingDQNNet.forward's combination: V [n, 1], A [n, 104] -> Q [n, 104] (sn_dqn_select_duel's model)"""
    return V + (A - A.mean(-1, keepdim=True))


# ---------------------------------------------------------------- the noisy nets' device noise (sn_noisy_*)
NOISY_TAG0 = 0xFFF00
NOISY_MAX_LAYERS = 64


def noisy_tag(layer, side):
    """the Philox rollout tag of linear layer `layer` (forward order: the latent layers, then the heads in
    head_nets order), side 0 = its inputs, 1 = its outputs (SN_NOISY_TAG, include/sechs.h)"""
    assert 0 <= int(layer) < NOISY_MAX_LAYERS and int(side) in (0, 1)
    return NOISY_TAG0 + 2 * int(layer) + int(side)


def noisy_normals_host(seed, step, gid, seat, layer, side, width):
    """the standard normals behind noisy_eps_host, float64 [width]"""
    pairs = (int(width) + 1) // 2
    o = decision_words_host(seed, step, int(gid), int(seat), noisy_tag(layer, side), 0, np.arange(pairs))
    o = o.astype(np.float64)
    u1, u2 = (np.floor(o[:, 0] / 256.0) + 1.0) * 2.0 ** -24, np.floor(o[:, 1] / 256.0) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    n = np.stack((r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)), axis=1).reshape(-1)
    return n[: int(width)]


def noisy_eps_host(seed, step, gid, seat, layer, side, width):
    """sn_noisy_eps' law in numpy float64: e = sign(n) sqrt|n| of the units 0 .. width - 1 of decision (global
    game gid, seat) at decision counter `step`, linear layer `layer`, side 0 (inputs) or 1 (outputs)"""
    n = noisy_normals_host(seed, step, gid, seat, layer, side, width)
    return np.sign(n) * np.sqrt(np.abs(n))


def noisy_linears(net):
    """the linear layers of a MultiHeadedMLP (a DuellingDQNNet's `mlp`) in forward order: the latent layers,
    then the heads in head_nets order -- the order the noise tags count"""
    mlp = getattr(net, "mlp", net)
    return [m for m in mlp.latent_net if isinstance(m, nn.Linear)] + [h[0] for h in mlp.head_nets]


def noisy_forward_host(net, x, eps):
    """NoisyFactorizedLinear's formula in float64, row by row: x [n, 47]; eps[l] = (e_in [n, K_l], e_out
    [n, J_l]), the shaped noise of layer l (noisy_linears order) for every row.  Returns what the module
    returns: [Q [n, 104]] (a DuellingDQNNet: V + (A - mean A)), as float64 tensors.  ReLU between the latent
    layers, heads without activation."""
    mlp = getattr(net, "mlp", net)
    lin = noisy_linears(net)
    n_lat = len(lin) - len(mlp.head_nets)

    def layer(l, h):
        m = lin[l]
        W, S = m.weight.detach().double().cpu(), m.sigma_weight.detach().double().cpu()
        b, sb = m.bias.detach().double().cpu(), m.sigma_bias.detach().double().cpu()
        e_in, e_out = (torch.as_tensor(e, dtype=torch.float64) for e in eps[l])
        rows = []
        for r in range(h.shape[0]):
            Wn = W + S * (e_out[r][:, None] * e_in[r][None, :])
            rows.append(Wn @ h[r] + b + sb * e_out[r])
        return torch.stack(rows)

    h = torch.as_tensor(x, dtype=torch.float64).cpu()
    for l in range(n_lat):
        h = layer(l, h).clamp_min(0)
    outs = [layer(n_lat + k, h) for k in range(len(mlp.head_nets))]
    if hasattr(net, "mlp"):
        V, A = outs
        return [V + (A - A.mean(-1, keepdim=True))]
    return outs


class NoisyDeviceNet:
    """the device form of a noisy Q net: per latent layer (W [J, K], b, S = sigma_weight [J, K] in net_dtype,
    sigma_bias f32); the heads as one padded GEMM [K, pad] like FusedMLP's, their sigmas block-diagonal
    [heads * K, pad] (every head scales the latent by its own input noise), sigma_bias f32 [pad];
    `heads`: (layer index, first column, width) per head in the padded output"""

    def __init__(self, net, duelling, dtype, device):
        from .utils.nets import NoisyFactorizedLinear

        mlp = net.mlp if duelling else net
        lat = list(mlp.latent_net)
        assert all(isinstance(m, NoisyFactorizedLinear) for m in lat[0::2]) and \
            all(isinstance(m, nn.ReLU) for m in lat[1::2]) and all(len(h) == 1 for h in mlp.head_nets), \
            "a noisy engine net is NoisyFactorizedLinear / ReLU layers and heads without activation"
        lin = noisy_linears(net)
        assert len(lin) <= NOISY_MAX_LAYERS
        self.layers = []
        for m in lat[0::2]:
            w, sg = m.weight.detach(), m.sigma_weight.detach()
            if w.shape[1] == OBS - 1:  # the 48-wide observation rows go in unsliced
                w, sg = nn.functional.pad(w, (0, 1)), nn.functional.pad(sg, (0, 1))
            self.layers.append((w.to(device, dtype).contiguous(), m.bias.detach().to(device, dtype),
                                sg.to(device, dtype).contiguous(), m.sigma_bias.detach().to(device, torch.float32)))
        heads = [h[0] for h in mlp.head_nets]
        n_lat, K, dev = len(self.layers), heads[0].in_features, device
        order = [1, 0] if duelling else list(range(len(heads)))  # [A | V | pad]: A starts every row aligned
        total = sum(h.out_features for h in heads)
        pad = max(16, -(-total // 16) * 16)
        self.head_w = torch.zeros((K, pad), dtype=dtype, device=dev)
        self.head_s = torch.zeros((len(heads) * K, pad), dtype=dtype, device=dev)
        self.head_b = torch.zeros((pad,), dtype=dtype, device=dev)
        self.head_sb = torch.zeros((pad,), dtype=torch.float32, device=dev)
        self.heads, c = [None] * len(heads), 0
        for k in order:
            h, J = heads[k], heads[k].out_features
            self.head_w[:, c: c + J] = h.weight.detach().t()
            self.head_s[k * K: (k + 1) * K, c: c + J] = h.sigma_weight.detach().t()
            self.head_b[c: c + J], self.head_sb[c: c + J] = h.bias.detach(), h.sigma_bias.detach()
            self.heads[k] = (n_lat + k, c, J)
            c += J
        self.head_sizes = [heads[k].out_features for k in order]
        self.K, self.pad = K, pad


def league_capacity(history_length, seats):
    """replay rows of a league engine: the drop-in's history length and at least two expected rounds of
    transitions (`seats` expected seats of the agent per round, T_STEPS rows each), as a power of two"""
    need = max(int(history_length or 0), int(2 * T_STEPS * seats), 2)
    return 1 << (need - 1).bit_length()


# ---------------------------------------------------------------- the engine
class BatchedDQN(BatchedEngine):
    def __init__(self, env, q_net, target_net=None, prioritised=False, gamma=0.99, eps_func=None, minibatch=64,
                 updates=T_STEPS, retrain_interval=4, tau=1e-2, capacity=1 << 16, seed=0, net_dtype=torch.bfloat16,
                 seats_mask=None, max_decisions=None, n_steps=1):
        """target_net given: the double-DQN target; prioritised: the PRB
        variants (importance-weighted loss, priorities written back); a
        DuellingDQNNet as q_net (or target_net): the duelling variants;
        n_steps > 1: the n-step rows and the discount gamma ** n_steps"""
        from .agents.dqn import eps_func_decay
        from .utils.nets import DuellingDQNNet, NoisyFactorizedLinear

        super().__init__(env, q_net, seed=seed, seats_mask=seats_mask, net_dtype=net_dtype, max_decisions=max_decisions)
        self.target_net, self.prioritised = target_net, bool(prioritised)
        self.gamma, self.tau = float(gamma), tau
        self.n_steps = int(n_steps)
        assert self.n_steps >= 1
        self.duelling = isinstance(q_net, DuellingDQNNet)
        # NoisyFactorizedLinear layers: every decision row draws its own noise on the device, no epsilon
        self.noisy = any(isinstance(m, NoisyFactorizedLinear) for m in q_net.modules())
        assert target_net is None or isinstance(target_net, DuellingDQNNet) == self.duelling, \
            "the local and the target net are of one kind"
        self.eps_func = eps_func_decay if eps_func is None else eps_func
        self.minibatch, self.updates, self.retrain_interval = int(minibatch), int(updates), int(retrain_interval)
        self.capacity = int(capacity)
        self.replay = DevicePER(self.capacity, ROW_BYTES, device=env.device)
        # training: epsilon = eps_func(episode), episode = the rounds this engine
        # has finished (the reference's eps_func(num_episode)); else the agent's
        # own `eps`, which the owner sets
        self.training, self.eps, self.episode = True, 0.0, 0
        self.eps_used = None     # the epsilon of the latest decide
        self.eps_history = []    # ... of every finished round
        self.update_count = 0    # minibatch updates so far (the drop-in's `step`)
        self.value = torch.zeros((self.D_max,), dtype=torch.float32, device=env.device)
        self._t, self._obs, self._acts = 0, None, None

    # ------------------------------------------------------------ the Q net on the device
    def sync_net(self):
        """(re)build the device copy of the Q net in net_dtype; Linear/ReLU
        layouts get the input weight padded to the 48-wide rows.  A duelling
        net: the FusedMLP of its `mlp`, the head rows reordered [A | V | pad]
        so that A starts every output row 16-byte aligned"""
        version = tuple(p._version for p in self.actor.parameters())
        if self._net is None or version != self._net_version:
            if self.noisy:
                self._net = NoisyDeviceNet(self.actor, self.duelling, self.net_dtype, self.env.device)
                self._net_version = version
                return self._net
            net = copy.deepcopy(self.actor).to(self.env.device, self.net_dtype)
            net.eval()
            f = FusedMLP.of(net.mlp if self.duelling else net)
            if self.duelling and f.layers is not None:
                order = list(range(1, 1 + NUM_ACTIONS)) + [0] + list(range(1 + NUM_ACTIONS, f.head_w.shape[1]))
                f.head_w, f.head_b = f.head_w[:, order].contiguous(), f.head_b[order].contiguous()
                f.head_sizes = [NUM_ACTIONS, 1]
            if f.layers is not None:
                w, b = f.layers[0]
                if w.shape[1] == OBS - 1:
                    wp = torch.zeros((w.shape[0], OBS), dtype=w.dtype, device=w.device)
                    wp[:, : OBS - 1] = w
                    f.layers[0] = (wp, b)
            self._net, self._net_version = f, version
        return self._net

    def _q_values(self, states):
        """[D, >= 104] f32 with unit column stride (the padded head's view: no copy in fp32)"""
        net = self._net
        with torch.no_grad():
            x = states if net.layers is not None and net.layers[0][0].shape[1] == OBS else states[:, : OBS - 1]
            (out,) = net(x)
        self.rows_evaluated += states.shape[0]
        out = out.float()
        return out if out.stride(1) == 1 else out.contiguous()

    def _head_values(self, states):
        """a duelling net's head output [D, stride] f32 with A in columns 0..103 and V in column 104: the
        padded GEMM output as it is (stride 112), or [A | V] packed when the module runs unfused"""
        net = self._net
        with torch.no_grad():
            if net.layers is not None:
                out = net.head_out(states if net.layers[0][0].shape[1] == OBS else states[:, : OBS - 1])
            else:
                V, A = net(states[:, : OBS - 1])
                out = torch.cat((A, V), dim=1)
        self.rows_evaluated += states.shape[0]
        return out.float().contiguous()

    def _noisy_values(self, q, states):
        """a noisy net's padded head output [D, pad] f32 (the plain net: Q in columns 0..103; the duelling
        net: [A | V | pad]), every row under its own noise of decision counter q.step.  Per layer: x o e_in
        (sn_noisy_scale), the plain GEMM with bias and the sigma GEMM of the same shape, then mu + e_out o
        (sg + sigma_b) (sn_noisy_combine; ReLU on the latent layers).  The heads' sigma GEMM is one GEMM over
        the latent scaled once per head, side by side, against the block-diagonal sigmas."""
        L, h, st = nat.lib(), self.env._h, self.env._stream()
        net, D, bf16 = self._net, int(states.shape[0]), int(self.net_dtype == torch.bfloat16)
        qr = ctypes_ref(q)

        def scale(layer, x, out, col):
            nat.check(L.sn_noisy_scale(h, qr, noisy_tag(layer, 0), nat.ptr(x), x.stride(0), x.shape[1], bf16,
                                       ctypes.c_void_p(out.data_ptr() + col * out.element_size()), out.stride(0), st),
                      "sn_noisy_scale")

        def combine(layer, mu, sg, col0, width, sigma_b, relu):
            nat.check(L.sn_noisy_combine(h, qr, noisy_tag(layer, 1), nat.ptr(mu), nat.ptr(sg), mu.stride(0), col0, width,
                                         nat.ptr(sigma_b), relu, nat.ptr(mu), st), "sn_noisy_combine")

        with torch.no_grad():
            x = states
            for l, (w, b, s, sb) in enumerate(net.layers):
                xs = torch.empty_like(x)
                scale(l, x, xs, 0)
                mu, sg = torch.addmm(b, x, w.t()).float(), torch.mm(xs, s.t()).float()
                combine(l, mu, sg, 0, mu.shape[1], sb, 1)
                x = mu.to(self.net_dtype)
            K = net.K
            xs = torch.empty((D, len(net.heads) * K), dtype=self.net_dtype, device=x.device)
            for k, (layer, _, _) in enumerate(net.heads):
                scale(layer, x, xs, k * K)
            mu, sg = torch.addmm(net.head_b, x, net.head_w).float(), torch.mm(xs, net.head_s).float()
            for layer, col0, width in net.heads:
                combine(layer, mu, sg, col0, width, net.head_sb, 0)
        self.rows_evaluated += D
        return mu

    def current_eps(self):
        if self.noisy:
            return 0.0  # the noise explores: the select kernels take their greedy branch
        return float(self.eps_func(self.episode)) if self.training else float(self.eps)

    # ------------------------------------------------------------ acting
    def decide(self, n, memorize=False, record=False):
        """epsilon-greedy card of every deciding seat at hand size n: actions [B, N] int32"""
        self.eps_used = self.current_eps()  # of a round without a seat too: end_episode logs it
        return super().decide(n, record=record)

    def _decide(self, q, n, record):
        L, h, st = nat.lib(), self.env._h, self.env._stream()
        D, dev = self.D, self.env.device
        self.sync_net()
        obs_t = None
        if record:
            if self._t == 0 or self._obs.shape[1] != D:
                self._obs = torch.zeros((T_STEPS + 1, D, OBS), dtype=torch.int8, device=dev)
                self._acts = torch.zeros((T_STEPS, D), dtype=torch.int32, device=dev)
                self._t = 0
            assert self._t < T_STEPS, "end_episode() closes a recorded episode"
            obs_t = self._obs[self._t]
        states = torch.empty((D, OBS), dtype=self.net_dtype, device=dev)
        nat.check(L.sn_dqn_obs(h, ctypes_ref(q), nat.ptr(obs_t), nat.ptr(states),
                               int(self.net_dtype == torch.bfloat16), st), "sn_dqn_obs")
        if self.noisy:
            out = self.q_handed = self._noisy_values(q, states)  # kept: what the select kernel reads
        else:
            out = self._head_values(states) if self.duelling else self._q_values(states)
        if self.duelling:
            nat.check(L.sn_dqn_select_duel(h, ctypes_ref(q), nat.ptr(out), out.stride(0), NUM_ACTIONS, 0,
                                           self.eps_used, nat.ptr(self.actions), nat.ptr(self.best_index),
                                           nat.ptr(self.value), st), "sn_dqn_select_duel")
        else:
            nat.check(L.sn_dqn_select(h, ctypes_ref(q), nat.ptr(out), out.stride(0), self.eps_used,
                                      nat.ptr(self.actions), nat.ptr(self.best_index), nat.ptr(self.value), st),
                      "sn_dqn_select")
        if record:
            self._acts[self._t] = self.actions.view(-1)[self.decider_index()]
            self._t += 1

    def rewards_seen(self, per_step, T=None):
        """[T, D] int32: the reward learn() gets at step t is step t-1's (0 at t = 0)"""
        T = per_step.shape[0] if T is None else T
        r = self.decider_rewards(per_step)[: T - 1].to(torch.int32)
        seen = torch.zeros((T, r.shape[1]), dtype=torch.int32, device=r.device)
        seen[1:] = r
        return seen

    def end_episode(self, per_step):
        """close the round: the terminal observation, the lagged rewards, the
        packed transition rows into the replay (returned; None if nothing
        was recorded)"""
        rows = None
        if self.D and self._t:
            L, h, st = nat.lib(), self.env._h, self.env._stream()
            T, D = self._t, self.D
            q = self._params(0)
            nat.check(L.sn_dqn_obs(h, ctypes_ref(q), nat.ptr(self._obs[T]), None, 0, st), "sn_dqn_obs")
            seen = self.rewards_seen(per_step, T).contiguous()
            rows = torch.empty((T * D, ROW_BYTES), dtype=torch.uint8, device=self.env.device)
            if self.n_steps > 1:
                gpow = nat.SnDqnGpow()
                gpow.v[:] = gamma_powers(self.gamma)
                nat.check(L.sn_dqn_pack_nstep(T, D, self.n_steps, gpow, nat.ptr(self._obs), nat.ptr(self._acts),
                                              nat.ptr(seen), nat.ptr(rows), st), "sn_dqn_pack_nstep")
            else:
                nat.check(L.sn_dqn_pack(T, D, nat.ptr(self._obs), nat.ptr(self._acts), nat.ptr(seen), nat.ptr(rows),
                                        st), "sn_dqn_pack")
            for i in range(0, T * D, self.capacity):  # ring order = sequential stores
                self.replay.store(rows[i: i + self.capacity])
        self._t = 0
        self.eps_history.append(self.eps_used)
        self.episode += 1
        return rows

    def play_episode(self, others=None, record=False):
        """one whole game of every env game (non-deciding seats: uniform
        moves); returns (summed rewards [B, N] int32, per-step rewards
        [10, B, N] int32)"""
        per_step = self._play_steps(record)
        self.end_episode(per_step)
        return per_step.sum(dim=0), per_step

    # ------------------------------------------------------------ learning
    def sample_batch(self, u=None, slots=None):
        """one minibatch of replay rows: prioritised -> DevicePER.sample (u:
        the uniforms, drawn on the device when None); uniform -> distinct
        slots of [0, min(len, capacity)) (History.sample's random.sample,
        drawn on the device when `slots` is None) and DevicePER.gather"""
        if self.prioritised:
            idx, _, weights, rows = self.replay.sample(self.minibatch, u)
            return {"idx": idx, "weights": weights, "rows": rows}
        if slots is None:
            held = min(len(self.replay), self.capacity)  # host counters: no device sync
            slots = torch.randperm(held, device=self.env.device)[: self.minibatch].to(torch.int32)
        return {"idx": None, "weights": None, "rows": self.replay.gather(slots)}

    def unpack(self, rows):
        n, dev = int(rows.shape[0]), self.env.device
        s = torch.empty((n, OBS), dtype=torch.float32, device=dev)
        s2 = torch.empty((n, OBS), dtype=torch.float32, device=dev)
        action = torch.empty((n,), dtype=torch.int64, device=dev)
        reward = torch.empty((n,), dtype=torch.float32, device=dev)
        not_done = torch.empty((n,), dtype=torch.float32, device=dev)
        name = "sn_dqn_unpack_nstep" if self.n_steps > 1 else "sn_dqn_unpack"  # the f32 return, or the i32 reward
        nat.check(getattr(nat.lib(), name)(n, nat.ptr(rows), nat.ptr(s), nat.ptr(s2), nat.ptr(action), nat.ptr(reward),
                                           nat.ptr(not_done), self.env._stream()), name)
        return s, s2, action, reward, not_done

    def bellman_target(self, q_next_local, q_next_target, reward, not_done):
        """sn_dqn_target on device tensors [n, stride >= 104] f32, discounting by gamma ** n_steps"""
        assert q_next_local.stride(1) == 1 and (q_next_target is None or q_next_target.stride() == q_next_local.stride())
        n = int(q_next_local.shape[0])
        target = torch.empty((n,), dtype=torch.float32, device=q_next_local.device)
        nat.check(nat.lib().sn_dqn_target(n, nat.ptr(q_next_local), nat.ptr(q_next_target), q_next_local.stride(0),
                                          nat.ptr(reward), nat.ptr(not_done), self.gamma ** self.n_steps,
                                          nat.ptr(target), self.env._stream()), "sn_dqn_target")
        return target

    def loss_terms(self, batch):
        """(q_eval, target, weights, loss) of one minibatch (_learn,
        agents/dqn.py:125-134): fp32 on the agent's own module"""
        s, s2, action, reward, not_done = self.unpack(batch["rows"])
        dev, here = self.actor_device(), self.env.device
        q = self.actor(s.to(dev)[:, : OBS - 1])[0]
        q_eval = q.gather(1, action.to(dev).view(-1, 1)).squeeze(1)
        with torch.no_grad():  # the drop-in's order of forwards (DDQNAgent._calc_reward): a noisy net draws in each
            qt = None
            if self.target_net is not None:
                tdev = next(self.target_net.parameters()).device
                qt = self.target_net(s2.to(tdev)[:, : OBS - 1])[0].to(here).contiguous()
            qn = self.actor(s2.to(dev)[:, : OBS - 1])[0].to(here).contiguous()
            target = self.bellman_target(qn, qt, reward, not_done).to(dev)
        if self.prioritised:
            weights = batch["weights"].to(dev, torch.float32)
            loss = (weights * (q_eval - target) ** 2).mean()
        else:
            weights = None
            loss = nn.functional.mse_loss(q_eval, target)
        return q_eval, target, weights, loss

    def soft_update(self, tau):
        """theta_target = tau * theta_local + (1 - tau) * theta_target (DDQNAgent.soft_update)"""
        for target_param, local_param in zip(self.target_net.parameters(), self.actor.parameters()):
            target_param.data.copy_(tau * local_param.data + (1 - tau) * target_param.data)

    def learn(self, optimizer):
        """`updates` minibatch steps once the replay holds more than a
        minibatch (the reference's gate); returns the losses (device scalars)"""
        if len(self.replay) <= self.minibatch:
            return []
        losses = []
        for _ in range(self.updates):
            batch = self.sample_batch()
            q_eval, target, weights, loss = self.loss_terms(batch)
            if self.prioritised:  # DQN_PRBAgent._update_memory, before the optimiser step
                self.replay.update(batch["idx"], torch.abs(q_eval.detach() - target))
            self.update_count += 1
            if self.target_net is not None and self.update_count % self.retrain_interval == 0:
                self.soft_update(self.tau)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            losses.append(loss.detach())
        return losses

    # ------------------------------------------------------------ the league's protocol (engine.BatchedEngine)
    closes_round = True

    @classmethod
    def from_agent(cls, env, agent, *, seed, net_dtype, slots, seats):
        """T_STEPS minibatch updates per round (the reference's learn calls per game), each on at least one
        row per slot.  agent.history, the drop-in's host buffer, stays unused (copy_player's deepcopy works)."""
        from .agents.dqn import DQN_PRBAgent

        return cls(env, agent.dqn_net_local, target_net=getattr(agent, "dqn_net_target", None),
                   prioritised=isinstance(agent, DQN_PRBAgent), gamma=agent.gamma, eps_func=agent.eps_func,
                   minibatch=max(int(agent.minibatch), slots), updates=T_STEPS,
                   retrain_interval=getattr(agent, "retrain_interval", 4), tau=getattr(agent, "tau", 1e-2),
                   capacity=league_capacity(agent.history.max_length, seats), seed=seed, net_dtype=net_dtype,
                   max_decisions=slots, n_steps=getattr(agent, "n_steps", 1))

    def begin_round(self, dec, agent, train):
        """training: eps_func(rounds finished); else the agent's own eps"""
        super().begin_round(dec, agent, train)
        self.training, self.eps = train, agent.eps

    def end_round(self, per_step):
        self.end_episode(per_step)  # terminal observation, lagged rewards, rows into the replay

    def learn_round(self, optimizer, per_step, updates_per_round):
        """its own schedule: `updates` minibatches per round, every one counted"""
        return len(self.learn(optimizer)) if self.D else None

    def inherit(self, parent):
        """a clone's engine goes on where its parent's stands, as the
        reference's copy_player carries the whole agent through its torch.save
        round trip (tournament.py:54-60): the replay with its priorities and
        beta (DevicePER.inherit: verbatim at equal capacity, else the newest
        rows), the episode count behind the epsilon schedule, the update
        count behind the soft-update cadence, the epsilon log.  Nothing from
        another kind of engine or another n_steps: those rows carry a
        different reward field."""
        if not isinstance(parent, BatchedDQN) or parent.n_steps != self.n_steps:
            return
        self.replay.inherit(parent.replay)
        self.episode, self.update_count = parent.episode, parent.update_count
        self.eps_history = list(parent.eps_history)

    def state_dict(self):
        """the base counters, the replay through DevicePER's own export (its pickle form: leaves, ring,
        pointer, num_items, hyper-parameters with beta -- no second format), the episode count behind the
        epsilon schedule, the update count behind the soft-update cadence and the epsilon log"""
        sd = super().state_dict()
        sd.update(replay=self.replay.__getstate__(), episode=self.episode, update_count=self.update_count,
                  eps_history=list(self.eps_history))
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        rep = sd["replay"]
        if rep["capacity"] != self.replay.capacity or rep["row_bytes"] != self.replay.row_bytes:
            raise ValueError(f"BatchedDQN.load_state_dict: the checkpoint's replay holds {rep['capacity']} rows of "
                             f"{rep['row_bytes']} bytes, this engine's {self.replay.capacity} of {self.replay.row_bytes}")
        self.replay.close()  # whatever it held is gone; the saved arrays load when the handle is next created
        self.replay.__setstate__(dict(rep, device=self.env.device))
        self.episode, self.update_count = int(sd["episode"]), int(sd["update_count"])
        self.eps_history = list(sd["eps_history"])
