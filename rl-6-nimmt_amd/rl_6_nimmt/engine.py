"""What the batched net-agent engines share (puct.BatchedPUCT / BatchedPUCTCustomed, reinforce.BatchedReinforce,
acer.BatchedACER, dqn.BatchedDQN): the deciding seats of a batch of games (a seats mask, or a tournament's
decision list), the device copy of the agent's net, the root candidate rows, the ten-step play loop and the
protocol the batched league drives its engines through (league.py).  An engine adds `_decide`, the launches of
one decision batch.  The search and its buffers are puct.BatchedPUCT's alone: the sn_puct a BatchedEngine fills
leaves them NULL (include/sechs.h, at sn_puct, lists the calls that need them)."""
import copy
import ctypes

import numpy as np
import torch
from torch import nn

from . import _native as nat
from .splitk import train_forward
from .utils.nets import MultiHeadedMLP, NoisyFactorizedLinear

ROW = 48
ctypes_ref = ctypes.byref

# ---------------------------------------------------------------- the decisions' Philox streams, on the host
# Every random word a kernel draws for a decision is Philox4x32-10 keyed (seed lo ^ step, seed hi) at the counter
# (c, 0, stream lo, stream hi); the stream word and its reserved tags are csrc/sechs_decide.h's (dec_stream).  This
# is the format's one host owner: the models the kernels are tested against are built on it.
SELECT_TAG = 0xFFFFE       # the epsilon-greedy draws (sn_dqn_select, sn_dqn_select_duel)
SAMPLE_TAG = 0xFFFFF       # the policy sample (sn_policy_sample)
ROLLOUT_TAG_END = 0xFFF00  # a PUCT rollout's tag is its number, below this; the noisy layers' tags start here
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10_host(ctr, key):
    """Philox4x32-10 on numpy arrays: ctr [..., 4], key [..., 2] (uint32, broadcast together) -> [..., 4] uint32"""
    ctr, key = np.asarray(ctr, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., j], shape).copy() for j in range(4)]
    k = [np.broadcast_to(key[..., j], shape).copy() for j in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c[0], np.uint64(_PHILOX_M1) * c[2]  # 32 x 32 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _U32]
        k = [(k[0] + np.uint64(_PHILOX_W0)) & _U32, (k[1] + np.uint64(_PHILOX_W1)) & _U32]
    return np.stack(c, axis=-1).astype(np.uint32)


def dec_stream_host(gid, seat, tag, low=0):
    """dec_stream's word as uint64: (gid's low 32 bits) << 32 | seat << 28 | tag << 8 | low byte.  gid is the
    global game id, game_offset + g; seat < 16, tag < 2**20 and low < 256 keep the fields apart.  The arguments
    broadcast together."""
    gid, seat, tag, low = (np.asarray(v, dtype=np.uint64) for v in (gid, seat, tag, low))
    assert bool((seat < 16).all()) and bool((tag < (1 << 20)).all()) and bool((low < 256).all())
    return ((gid & _U32) << np.uint64(32)) | (seat << np.uint64(28)) | (tag << np.uint64(8)) | low


def decision_words_host(seed, step, gid, seat, tag, low, counters):
    """the four Philox words of every (decision, counter): uint32 [..., 4] over gid, seat and counters broadcast
    together.  seed: the engine's 64-bit seed, step: its 32-bit decision counter (sn_puct.seed / .step)."""
    seed = int(seed) & (2**64 - 1)
    stream, counters = dec_stream_host(gid, seat, tag, low), np.asarray(counters, dtype=np.uint64)
    ctr = np.zeros(np.broadcast_shapes(stream.shape, counters.shape) + (4,), dtype=np.uint64)
    ctr[..., 0], ctr[..., 2], ctr[..., 3] = counters & _U32, stream & _U32, stream >> np.uint64(32)
    key = np.array([(seed & 0xFFFFFFFF) ^ (int(step) & 0xFFFFFFFF), seed >> 32], dtype=np.uint64)
    return philox4x32_10_host(ctr, key)


def make_actor(hidden_sizes=(100, 100), activation=None):
    """the reference's policy net: MultiHeadedMLP(48, (100, 100), (1,), ReLU, (None,))"""
    return MultiHeadedMLP(ROW, hidden_sizes=hidden_sizes, head_sizes=(1,), activation=activation or nn.ReLU(),
                          head_activations=(None,))


class FusedMLP:
    """Inference form of MultiHeadedMLP(48, hidden, heads, ReLU, (None,)) on
    PyTorch-ROCm (north_star: the net runs through PyTorch): every hidden
    layer one hipBLASLt GEMM with the bias + ReLU fused into its epilogue
    (torch._addmm_activation: no separate clamp pass over the [rows, 100]
    activations), the heads one GEMM over the head rows zero-padded to 16
    outputs (a [rows,100]x[100,1] GEMV runs 2x slower than the padded GEMM on
    gfx950).  Measured on 1.31 M bf16 rows: 1091 -> 839 us (tools/mlp_bench.py).
    Other layouts fall back to the module."""

    def __init__(self, module, layers, head_w, head_b, head_sizes):
        self.module, self.layers = module, layers
        self.head_w, self.head_b, self.head_sizes = head_w, head_b, head_sizes

    @classmethod
    def of(cls, net):
        lat = list(net.latent_net)
        heads = list(net.head_nets)
        def plain(m):  # a NoisyFactorizedLinear is an nn.Linear too: its forward is not W x + b
            return isinstance(m, nn.Linear) and not isinstance(m, NoisyFactorizedLinear)

        ok = len(lat) % 2 == 0 and all(plain(m) for m in lat[0::2]) and \
            all(isinstance(m, nn.ReLU) for m in lat[1::2]) and all(len(h) == 1 and plain(h[0]) for h in heads)
        if not ok:
            return cls(net, None, None, None, None)
        layers = [(m.weight.detach(), m.bias.detach()) for m in lat[0::2]]
        w = torch.cat([h[0].weight.detach() for h in heads], dim=0)
        b = torch.cat([h[0].bias.detach() for h in heads], dim=0)
        pad = max(16, -(-w.shape[0] // 16) * 16)
        wp = torch.zeros((pad, w.shape[1]), dtype=w.dtype, device=w.device)
        bp = torch.zeros((pad,), dtype=b.dtype, device=b.device)
        wp[: w.shape[0]], bp[: b.shape[0]] = w, b
        return cls(net, layers, wp.t().contiguous(), bp, [h[0].out_features for h in heads])

    def refresh_from(self, actor):
        """copy new weights of the same architecture into this net's tensors
        in place (every derived tensor too): addresses stay, so captured
        hipGraphs stay valid.  False if the layout differs."""
        src, dst = dict(actor.named_parameters()), dict(self.module.named_parameters())
        if src.keys() != dst.keys() or any(src[k].shape != dst[k].shape for k in dst):
            return False
        with torch.no_grad():
            for k, v in dst.items():
                v.copy_(src[k])
            if self.layers is not None:
                fresh = FusedMLP.of(self.module)
                self.head_w.copy_(fresh.head_w)
                self.head_b.copy_(fresh.head_b)
                if getattr(self, "_fused", None) is not None:
                    for old, new in zip(self._fused, fresh.fused()):
                        old.copy_(new)
        return True

    def fused(self):
        """the one-kernel rollout form (sn_puct_mlp_seats / sn_puct_rollouts)
        for MultiHeadedMLP(48, (H, H2), (1,)) in bf16 with H <= 111, H2 <= 127:
        w1c [112] f32 (W1[:, 0], then 0), W2 [128][112] bf16 ([W2 | b2 | 0]
        rows, the ones pass-through row H2), head [128] f32 ([wh | bh | 0]),
        w1s [128][64] bf16 ([W1 | b1 | 0] rows, 1 at (H, 48): the ones
        feature); None for other layouts (they run sn_puct_rows + __call__)"""
        if getattr(self, "_fused", "unset") != "unset":
            return self._fused
        self._fused = None
        if self.layers is None or len(self.layers) != 2 or self.head_sizes != [1] or \
                self.layers[0][0].shape[1] != ROW or self.layers[0][0].dtype != torch.bfloat16:
            return None
        w1, b1 = self.layers[0]
        H = w1.shape[0]
        w2, b2 = self.layers[1]
        H2 = w2.shape[0]
        if H > 111 or H2 > 127 or w2.shape[1] != H:
            return None
        dev = w1.device
        c = torch.zeros((112,), dtype=torch.float32, device=dev)
        c[:H] = w1[:, 0].float()
        w2p = torch.zeros((128, 112), dtype=torch.bfloat16, device=dev)
        w2p[:H2, :H], w2p[:H2, H], w2p[H2, H] = w2, b2, 1.0
        head = torch.zeros((128,), dtype=torch.float32, device=dev)
        head[:H2] = self.head_w[:, 0].float()
        head[H2] = self.head_b[0].float()
        w1s = torch.zeros((128, 64), dtype=torch.bfloat16, device=dev)  # [W1 | b1 | 0] rows
        w1s[:H, :ROW], w1s[:H, ROW] = w1, b1
        w1s[H, ROW] = 1.0
        self._fused = (c, w2p, head, w1s)
        return self._fused

    def head_out(self, rows):
        """the padded head GEMM's output [rows, pad] as it is (fused layouts only)"""
        h = rows
        for w, b in self.layers:
            h = torch._addmm_activation(b, h, w.t())
        return torch.addmm(self.head_b, h, self.head_w)

    def __call__(self, rows):
        if self.layers is None:
            return self.module(rows)
        out = self.head_out(rows)
        res, c = [], 0
        for n in self.head_sizes:
            res.append(out[:, c: c + n])
            c += n
        return res


class BatchedEngine:
    def __init__(self, env, actor, seed=0, seats_mask=None, net_dtype=torch.bfloat16, max_decisions=None):
        # `actor` stays where the caller keeps it (the drop-in agents run it
        # on the host): inference uses a device copy in net_dtype (sync_net),
        # the training losses run on the actor's own device (actor_device).
        self.env, self.actor = env, actor
        self.seed = int(seed)
        self.net_dtype = net_dtype
        B, N, dev = env.num_games, env.num_players, env.device
        self.seats_mask = ((1 << N) - 1) if seats_mask is None else int(seats_mask)
        self.M = bin(self.seats_mask & ((1 << N) - 1)).count("1")
        self.D = B * self.M
        # tournament mode (max_decisions given): the deciding seats are a
        # decision list (use_decisions: g * N + p of this agent's seats in the
        # slots' current games), at most max_decisions of them
        self.dec, self._flat = None, None
        if max_decisions is not None:
            self.D = 0
        self.D_max = B * self.M if max_decisions is None else int(max_decisions)
        self.best_index = torch.zeros((self.D_max,), dtype=torch.int32, device=dev)
        self.actions = torch.zeros((B, N), dtype=torch.int32, device=dev)
        self.step_id = 0
        self.decisions = []  # (root rows, n, best index) per decision batch, for the losses
        self._net = None
        self._net_version = None
        self.rows_evaluated = 0

    # ------------------------------------------------------------ the net on the device
    def sync_net(self):
        """(re)build the device copy of the actor in net_dtype"""
        version = tuple(p._version for p in self.actor.parameters())
        if self._net is not None and version != self._net_version and self._net.refresh_from(self.actor):
            self._net_version = version  # updated in place: the tensors' addresses stay
        if self._net is None or version != self._net_version:
            net = copy.deepcopy(self.actor).to(self.env.device, self.net_dtype)
            net.eval()
            self._net, self._net_version = FusedMLP.of(net), version
        return self._net

    def actor_device(self):
        return next(self.actor.parameters()).device

    def _logits(self, rows):
        with torch.no_grad():
            (out,) = self._net(rows)
        self.rows_evaluated += rows.shape[0]
        return out.reshape(-1).float().contiguous()

    def use_decisions(self, dec):
        """tournament mode: the seats to decide for, int32 [D] = g * N + p on
        the device (sn_puct.dec_list); a game of k players rolls out k seats"""
        dec = torch.as_tensor(dec, device=self.env.device).to(torch.int32).contiguous()
        assert dec.numel() <= self.D_max, "more decisions than max_decisions"
        self.dec, self.D = dec, int(dec.numel())

    def decider_index(self):
        """flat g * N + p of every decision, in decision order"""
        if self.dec is not None:
            return self.dec.long()
        if self._flat is None:
            N = self.env.num_players
            seats = torch.tensor([p for p in range(N) if (self.seats_mask >> p) & 1], device=self.env.device)
            self._flat = (torch.arange(self.env.num_games, device=self.env.device)[:, None] * N + seats[None, :]).reshape(-1)
        return self._flat

    def decider_rewards(self, per_step):
        """per_step [T, B, N] -> [T, D]: the deciding seats' rewards in decision order"""
        return per_step.reshape(per_step.shape[0], -1)[:, self.decider_index()]

    def _params(self, n):
        """the deciding seats, seed and decision counter; the search fields stay NULL (BatchedPUCT fills its own)"""
        q = nat.SnPuct()
        if self.dec is not None:
            q.dec_list, q.num_dec = self.dec.data_ptr(), self.D
        q.seats_mask, q.n = self.seats_mask, n
        q.seed, q.step = self.seed & (2**64 - 1), self.step_id & 0xFFFFFFFF
        return q

    # ------------------------------------------------------------ one decision per deciding seat
    def _root_rows(self, q, n):
        """the normalised candidate rows [D * n, ROW] of every decision, in net_dtype"""
        rows = torch.empty((self.D * n, ROW), dtype=self.net_dtype, device=self.env.device)
        bf16 = int(self.net_dtype == torch.bfloat16)
        nat.check(nat.lib().sn_puct_root_rows(self.env._h, ctypes_ref(q), nat.ptr(rows), bf16, self.env._stream()),
                  "sn_puct_root_rows")
        return rows

    def _train_rows(self, q, n, rows):
        """the root rows of a recorded decision in fp32, as the reference's
        training forward sees them (inference may run on bf16 rows)"""
        if rows is not None and rows.dtype == torch.float32:
            return rows.clone()
        r32 = torch.empty((self.D * n, ROW), dtype=torch.float32, device=self.env.device)
        nat.check(nat.lib().sn_puct_root_rows(self.env._h, ctypes_ref(q), nat.ptr(r32), 0, self.env._stream()),
                  "sn_puct_root_rows")
        return r32

    def _record(self, q, n, rows):
        """keep the decision batch for the loss: fp32 root rows, hand size, chosen indices"""
        self.decisions.append((self._train_rows(q, n, rows), n, self.best_index[: self.D].clone()))

    def decide(self, n, memorize=False, record=False):
        """every deciding seat's card at hand size n (_decide); returns actions [B, N] int32, those seats filled in"""
        if self.D:  # tournament mode: D == 0 when this agent has no seat in any current game
            self._decide(self._params(n), n, record)
        self.step_id += 1
        return self.actions

    def _play_steps(self, record):
        """reset, then the ten steps: the deciding seats play decide()'s moves, the other seats (if any)
        uniform legal ones; returns the per-step rewards [10, B, N] int32"""
        env = self.env
        env.reset()
        N = env.num_players
        per_step = torch.zeros((10, env.num_games, N), dtype=torch.int32, device=env.device)
        keep = torch.tensor([(self.seats_mask >> p) & 1 for p in range(N)], device=env.device, dtype=torch.bool)
        for t in range(10):
            acts = self.decide(10 - t, record=record)
            if self.M < N:
                acts = torch.where(keep[None, :], acts, self._random_moves())
            per_step[t] = env.step(acts)[0]
        return per_step

    def _random_moves(self):
        """uniform legal moves for the non-deciding seats (host-side torch RNG)"""
        hands = self.env.hands().long()
        n = (hands >= 0).sum(dim=2)
        k = (torch.rand(hands.shape[:2], device=hands.device) * n).long().clamp(max=9)
        return hands.gather(2, k[..., None])[..., 0].to(torch.int32)

    # ------------------------------------------------------------ the league's protocol (league.py)
    closes_round = False  # end_round does work: the league times it as its "store" phase

    @classmethod
    def from_agent(cls, env, agent, *, seed, net_dtype, slots, seats):
        """the tournament-mode engine of a drop-in agent: at most `slots` decisions per step; `seats`,
        the agent's expected seats per round, sizes the replay of the engines that keep one"""
        raise NotImplementedError(f"{cls.__name__}.from_agent")

    def begin_round(self, dec, agent, train):
        """a round starts: `dec`, this agent's seats in the slots' new games"""
        self.use_decisions(dec)
        self.decisions = []

    def end_round(self, per_step):
        """the round's ten steps are played (per_step [10, B, N] int32)"""

    def round_loss(self, per_step, *span):
        """the loss learn_round steps on, over deciders `span` = (d0, d1) or all of them"""
        raise NotImplementedError(f"{type(self).__name__}.round_loss")

    def learn_round(self, optimizer, per_step, updates_per_round):
        """train on the round: one optimiser step per loss of k contiguous decider ranges (a decider per
        game of this agent: k chunks of games; "games": every game).  Returns the steps to count, or None."""
        if self.D == 0 or not self.decisions:
            return None
        D = int(self.D)
        k = D if updates_per_round == "games" else min(int(updates_per_round), D)
        bounds = [D * c // k for c in range(k + 1)]
        for span in zip(bounds[:-1], bounds[1:]):
            loss = self.round_loss(per_step, *(span if k > 1 else ()))
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        self.decisions = []
        return k

    def inherit(self, parent):
        """a clone's engine takes over what its parent's engine keeps across rounds (nothing here)"""

    def state_dict(self):
        """what the engine keeps across rounds, on the CPU (checkpoints: BatchedTournament.save): the decision
        counter every Philox draw is keyed by, and the rows counter.  The net and its optimiser are the
        agent's; the device copy of the net, the decision list and the recorded decisions are rebuilt by the
        next round."""
        return {"step_id": self.step_id, "rows_evaluated": self.rows_evaluated}

    def load_state_dict(self, sd):
        """restore `state_dict()` into an engine built as usual (from_agent) over the restored handle"""
        self.step_id, self.rows_evaluated = int(sd["step_id"]), int(sd["rows_evaluated"])


def decision_forwards(actor, decisions, d0, d1, dev):
    """the training forward of every recorded decision batch's root rows in ONE
    pass (the batches' rows concatenated: one GEMM chain forward and backward
    instead of one per hand size), split back per batch: yields (the net's
    outputs, n, chosen indices) of deciders [d0, d1) per decision batch"""
    parts, segs = [], []
    for rows, n, best in decisions:
        e = best.shape[0] if d1 is None else d1
        parts.append(rows[d0 * n: e * n])
        segs.append((n, (e - d0) * n, best[d0:e].to(dev).long()))
    if not parts:
        return
    outs = train_forward(actor, torch.cat(parts).to(dev))
    off = 0
    for n, m, best in segs:
        yield [o[off: off + m] for o in outs], n, best
        off += m
