"""Batched "Alpha0.5" PUCT search on one MI355X (BASELINE config 4).

Reference: PUCTAgent / PolicyMCSAgent (agents/mcts.py:191-323).  A decision
runs n_mc = min(mc_max, mc_per_card * n!) rollouts; at each rollout's first
step the deciding seat picks its move by PUCT over the statistics so far,
every other move is sampled from the policy net, and the return is backed
up to the root move; finally the move with the best mean return is played.

Here all decisions of a batch (every deciding seat of every game) advance
together: for each rollout r and rollout step t, the HIP kernels emit the
normalised candidate rows of every seat, the policy MLP (PyTorch-ROCm,
bf16 by default) turns them into logits, and sn_puct_step selects / samples,
plays the step and, at the end, backs up.  Rollouts of one decision stay a
sequential chain, exactly as in the reference.
"""
import math
import os

import torch
from torch import nn

from . import _native as nat
from .engine import ROW, BatchedEngine, FusedMLP, ctypes_ref, decision_forwards, make_actor  # noqa: F401  (re-exported)
from .utils.nets import MultiHeadedMLP


class BatchedPUCT(BatchedEngine):
    def __init__(self, env, actor, mc_per_card=10, mc_max=100, c_puct=2.0, seed=0, seats_mask=None, puct_root=True,
                 net_dtype=torch.bfloat16, mcs_num_cards=104, graph=False, max_decisions=None, fused_rollouts=None):
        super().__init__(env, actor, seed=seed, seats_mask=seats_mask, net_dtype=net_dtype, max_decisions=max_decisions)
        self.mc_per_card, self.mc_max, self.c_puct = mc_per_card, mc_max, float(c_puct)
        self.puct_root = bool(puct_root)
        self.mcs_num_cards = mcs_num_cards
        B, N, dev = env.num_games, env.num_players, env.device
        D = self.D_max
        self.avail = torch.zeros((4, B * N), dtype=torch.int32, device=dev)
        self.ro = torch.zeros((D, 48), dtype=torch.int32, device=dev)
        self.stats = torch.zeros((D, 24), dtype=torch.int32, device=dev)
        self.hist = torch.zeros((D, 172), dtype=torch.int32, device=dev)
        self.root_probs = torch.zeros((D, 10), dtype=torch.float32, device=dev)
        # graph=True: a decision's rollout chain (n_mc x [deal, n x (rows,
        # MLP, step)] launches) is captured once per hand size as a hipGraph
        # (torch.cuda.CUDAGraph) and replayed for every decision; the kernels
        # read the decision counter from step_dev, new weights are copied
        # into the captured tensors in place (FusedMLP.refresh_from).
        # graph_after: uses of a shape that run eagerly before it is captured
        # (1 for one-game drop-in agents, whose one-off shapes would cost a
        # capture each)
        self.graph = bool(graph) and max_decisions is None
        self.graph_after = 0
        self._graphs, self._graphs_seen = {}, {}
        # bf16 nets of the reference's shape (FusedMLP.fused) run the rollout MLP as one MFMA
        # kernel (sn_puct_mlp_seats / sn_puct_rollouts); other nets run sn_puct_rows + the net
        # the rollout loop deals this many rollouts per launch
        # (sn_puct_deal_batch into a [deal_batch][D][48] buffer, each rollout
        # then running on its slice); 0: one sn_puct_deal per rollout (A/B, tests)
        self.deal_batch = int(os.environ.get("SECHS_PUCT_DEAL_BATCH", "16"))
        # whole rollouts in one kernel per deal batch (sn_puct_rollouts: a wave per group of 8
        # decisions, logits in LDS; round 6: 1.10 G playout env-steps/s on config 4, and the
        # tournament's engines too) or a launch per step (fused_rollouts=False);
        # SECHS_PUCT_ROLLOUTS=0 / 1 overrides (A/B runs, tests); SECHS_PUCT_GROUP=k (read by
        # sn_puct_rollouts itself) forces k decisions per wave's group instead of the device-sized count
        env_ro = os.environ.get("SECHS_PUCT_ROLLOUTS")
        self.fused_rollouts = (env_ro != "0") if env_ro is not None else (True if fused_rollouts is None
                                                                            else bool(fused_rollouts))
        self._step_dev = torch.zeros((1,), dtype=torch.int32, device=dev)

    # ------------------------------------------------------------ policy net on the device
    def sync_net(self):
        """BatchedEngine.sync_net; a rebuilt copy drops the captured graphs (an in-place refresh keeps them)"""
        old = self._net
        net = super().sync_net()
        if net is not old:
            self._graphs = {}
            if net.fused() is not None:  # built here: a graph capture may not allocate
                self._fused_bufs()
        return net

    def n_mc(self, n):
        return min(self.mc_max, self.mc_per_card * math.factorial(n))

    def _params(self, n, rollout=0, step_dev=False):
        q = super()._params(n)
        q.step_dev = self._step_dev.data_ptr() if step_dev else None
        q.puct_root, q.c_puct, q.rollout = int(self.puct_root), self.c_puct, rollout
        q.avail, q.rollouts, q.stats = self.avail.data_ptr(), self.ro.data_ptr(), self.stats.data_ptr()
        q.hist, q.root_probs = self.hist.data_ptr(), self.root_probs.data_ptr()
        return q

    # ------------------------------------------------------------ one decision per deciding seat
    def memorize(self):
        nat.check(nat.lib().sn_mcs_memorize(self.env._h, nat.ptr(self.avail), self.mcs_num_cards, self.env._stream()),
                  "sn_mcs_memorize")

    def decide(self, n, memorize=True, record=False):
        """Search every deciding seat at hand size n; returns actions [B, N]
        (int32, deciding seats filled in)."""
        if memorize:
            self.memorize()
        return super().decide(n, record=record)

    def _decide(self, q, n, record):
        L, h, st = nat.lib(), self.env._h, self.env._stream()
        if n > 1:
            self.sync_net()
            rows = self._root_rows(q, n)
            nat.check(L.sn_puct_init(h, ctypes_ref(q), nat.ptr(self._logits(rows)), st), "sn_puct_init")
            if self.graph:
                # the same 32-bit counter as the eager path's q.step, as int32 bits
                sid = self.step_id & 0xFFFFFFFF
                self._step_dev.fill_(sid - (1 << 32) if sid >= (1 << 31) else sid)
                key = (n, self.n_mc(n), self.c_puct, self.puct_root, self.D)  # everything a capture bakes in
                g = self._graphs.get(key)
                if g is None and self._graphs_seen.get(key, 0) >= self.graph_after:
                    g = self._capture(n)
                    self._graphs[key] = g
                if g is None:
                    self._graphs_seen[key] = self._graphs_seen.get(key, 0) + 1
                    self._rollouts(n, q)
                else:
                    g[0].replay()
                    self.rows_evaluated += g[1]
            else:
                self._rollouts(n, q)
        nat.check(L.sn_puct_choose(h, ctypes_ref(q), nat.ptr(self.actions), nat.ptr(self.best_index), st),
                  "sn_puct_choose")
        if record and n > 1:
            self._record(q, n, rows)

    def _rollouts(self, n, q):
        """the decision's rollout chain: n_mc x [deal, n x (rows, MLP, step)]"""
        L, h, st = nat.lib(), self.env._h, self.env._stream()
        bf16 = int(self.net_dtype == torch.bfloat16)
        N = self.env.num_players
        fz = self._net.fused()
        if fz is not None:
            # the reference-shaped bf16 net: per rollout step the seats' [0, obs, 1] rows, layer 1's
            # per-seat part on MFMA, the card column + ReLU, layer 2 + ReLU and the head in one MFMA
            # kernel (f32 logits, packed) -- no activation tensor in HBM
            w1c, w2p, head, w1s = fz
            S = self.D * N
            logits = self._fused_bufs()
            # the arguments built once (the league's engines run this loop eagerly: host time per launch)
            qr, deal, step, mlp = ctypes_ref(q), L.sn_puct_deal, L.sn_puct_step, L.sn_puct_mlp_seats
            wargs = (nat.ptr(w1s), nat.ptr(w1c), nat.ptr(w2p), nat.ptr(head), nat.ptr(logits), st)
            lp = nat.ptr(logits)
            RB, nmc = self.deal_batch, self.n_mc(n)
            if self.fused_rollouts and RB > 0 and 3 <= N <= 8:
                rob = self._deal_buf(RB)
                for r0 in range(0, nmc, RB):
                    nr = min(RB, nmc - r0)
                    nat.check(L.sn_puct_deal_batch(h, qr, r0, nr, rob.data_ptr(), st), "sn_puct_deal_batch")
                    nat.check(L.sn_puct_rollouts(h, qr, r0, nr, rob.data_ptr(), nat.ptr(w1s), nat.ptr(w1c),
                                                 nat.ptr(w2p), nat.ptr(head), st), "sn_puct_rollouts")
                self.rows_evaluated += nmc * S * (n * (n + 1) // 2)
                return
            if RB > 0:
                rob = self._deal_buf(RB)
                stride = self.D * 48 * 4  # bytes of one rollout's states
            for r in range(nmc):
                q.rollout = r
                if RB > 0:
                    if r % RB == 0:
                        nat.check(L.sn_puct_deal_batch(h, qr, r, min(RB, nmc - r), rob.data_ptr(), st),
                                  "sn_puct_deal_batch")
                    q.rollouts = rob.data_ptr() + (r % RB) * stride
                else:
                    nat.check(deal(h, qr, st), "sn_puct_deal")
                for t in range(n):
                    nat.check(mlp(h, qr, n - t, *wargs), "sn_puct_mlp_seats")
                    nat.check(step(h, qr, lp, t, n - t, st), "sn_puct_step")
            q.rollouts = self.ro.data_ptr()
            self.rows_evaluated += nmc * S * (n * (n + 1) // 2)
            return
        # any other net (fp32, other widths or depths): the candidate rows + the net's forward
        bufs = self._bufs(n)
        views = {m: bufs[m][: self.D * N * m] for m in range(1, n + 1)}  # this batch's decisions
        for r in range(self.n_mc(n)):
            q.rollout = r
            nat.check(L.sn_puct_deal(h, ctypes_ref(q), st), "sn_puct_deal")
            for t in range(n):
                m = n - t
                nat.check(L.sn_puct_rows(h, ctypes_ref(q), m, nat.ptr(views[m]), bf16, st), "sn_puct_rows")
                nat.check(L.sn_puct_step(h, ctypes_ref(q), nat.ptr(self._logits(views[m])), t, m, st), "sn_puct_step")

    def _deal_buf(self, RB):
        """[RB][D_max][48] int32: the initial states of RB rollouts (sn_puct_deal_batch)"""
        if getattr(self, "_robuf", None) is None or self._robuf.shape[0] != RB:
            self._robuf = torch.zeros((RB, self.D_max, 48), dtype=torch.int32, device=self.env.device)
        return self._robuf

    def _fused_bufs(self):
        """the rollout logits [D_max*N*10] f32 of sn_puct_mlp_seats"""
        S = self.D_max * self.env.num_players
        if getattr(self, "_fbufs", None) is None or self._fbufs.shape[0] != S * 10:
            self._fbufs = torch.empty((S * 10,), dtype=torch.float32, device=self.env.device)
        return self._fbufs

    def _bufs(self, n):
        N = self.env.num_players
        if not hasattr(self, "_rowbufs"):
            self._rowbufs = {}
        for m in range(1, n + 1):
            if m not in self._rowbufs:
                self._rowbufs[m] = torch.empty((self.D_max * N * m, ROW), dtype=self.net_dtype, device=self.env.device)
        return self._rowbufs

    def _capture(self, n):
        """capture _rollouts(n) with the decision counter read from step_dev"""
        q = self._params(n, step_dev=True)
        self._bufs(n)
        before = self.rows_evaluated
        torch.cuda.synchronize(self.env.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._rollouts(n, q)
        rows = self.rows_evaluated - before
        self.rows_evaluated = before
        return g, rows

    def play_episode(self, others=None, record=False):
        """One whole game of every env game (_play_steps); returns the summed rewards [B, N] int32."""
        return self._play_steps(record).sum(dim=0, dtype=torch.int32)

    # ------------------------------------------------------------ training (mcts.py:230-261)
    def policy_loss(self, d0=0, d1=None):
        """-sum over recorded decisions of log pi(chosen root move) under the
        current weights (the reference stores log(probs[best]) from the
        rollout that first chose it -- same weights during an episode, so the
        same value).  n == 1 decisions play without search and add log 1 = 0
        (mcts.py:50-51), so they are not recorded.  [d0, d1): the deciders
        (games) whose terms are summed -- one decider's term is the
        reference's per-episode loss (mcts.py:244-255)."""
        dev = self.actor_device()
        loss = torch.zeros((), device=dev)
        for (logits,), n, best in decision_forwards(self.actor, self.decisions, d0, d1, dev):
            logp = torch.log_softmax(logits.reshape(-1, n), dim=1)
            loss = loss - logp.gather(1, best[:, None]).sum()
        return loss

    # ------------------------------------------------------------ the league's protocol (engine.BatchedEngine)
    @classmethod
    def from_agent(cls, env, agent, *, seed, net_dtype, slots, seats):
        return cls(env, agent.actor, mc_per_card=agent.mc_per_card, mc_max=agent.mc_max,
                   c_puct=getattr(agent, "c_puct", 2.0), seed=seed, puct_root=agent._puct_root, net_dtype=net_dtype,
                   mcs_num_cards=agent.num_cards, max_decisions=slots)

    def round_loss(self, per_step, *span):
        return self.policy_loss(*span)


def make_actor_value(hidden_sizes=(100, 100), activation=None):
    """PUCTCustomedAgent's net (mcts.py:334-335): MultiHeadedMLP(48, (100, 100), (2,)) -- column 0 the
    policy logit, column 1 the value"""
    return MultiHeadedMLP(ROW, hidden_sizes=hidden_sizes, head_sizes=(2,), activation=activation or nn.ReLU(),
                          head_activations=(None,))


class BatchedPUCTCustomed(BatchedEngine):
    """PUCTCustomedAgent (agents/mcts.py:325-451) for every deciding seat of
    a batch of games.  The reference's "search" draws an environment and
    evaluates the 2-head net once on the root candidates -- no rollouts
    (_play_out_with_NN, mcts.py:366-376): the move is the first argmax of
    the value head, its log-probability comes from the policy head and the
    chosen value is the step's outcome.  Per decision batch: one
    sn_puct_root_rows launch (normalised rows straight from the device
    state), one MLP forward (PyTorch-ROCm), one sn_pcv_choose launch.

    Training (mcts.py:421-451) from stored rows instead of retained graphs:
    per (game, deciding seat), loss = MSE(values of the chosen moves,
    reward_sum) - sum(log pi(chosen)), with reward_sum = the rewards of the
    first 9 steps (GameSession hands learn() the previous step's reward,
    play.py:29,57,72, so the last step's never reaches the agent); the batch
    loss is the sum over games (the reference steps Adam after every game)."""

    def __init__(self, env, actor, seats_mask=None, net_dtype=torch.bfloat16, seed=0, max_decisions=None):
        super().__init__(env, actor, seed=seed, seats_mask=seats_mask, net_dtype=net_dtype, max_decisions=max_decisions)
        D = self.D_max
        self.log_prob = torch.zeros((D,), dtype=torch.float32, device=env.device)
        self.value = torch.zeros((D,), dtype=torch.float32, device=env.device)

    def _decide(self, q, n, record):
        self.sync_net()
        rows = self._root_rows(q, n)
        with torch.no_grad():
            (heads,) = self._net(rows)
        self.rows_evaluated += rows.shape[0]
        heads = heads.float().contiguous()
        nat.check(nat.lib().sn_pcv_choose(self.env._h, ctypes_ref(q), nat.ptr(heads), nat.ptr(self.actions),
                                          nat.ptr(self.best_index), nat.ptr(self.log_prob), nat.ptr(self.value),
                                          self.env._stream()), "sn_pcv_choose")
        if record:
            self._record(q, n, rows)

    def play_episode(self, others=None, record=False):
        """one whole game of every env game; returns (summed rewards [B, N]
        int32, per-step rewards [10, B, N] int32)"""
        self.episode_rewards = per_step = self._play_steps(record)
        return per_step.sum(dim=0), per_step

    @classmethod
    def from_agent(cls, env, agent, *, seed, net_dtype, slots, seats):
        return cls(env, agent.actor, net_dtype=net_dtype, seed=seed, max_decisions=slots)

    def loss(self, per_step=None, d0=0, d1=None):
        """reference loss of the recorded episode (mcts.py:431-451), summed over
        the games of deciders [d0, d1) (all by default)"""
        per_step = self.episode_rewards if per_step is None else per_step
        dev = self.actor_device()
        target = self.decider_rewards(per_step)[:-1].sum(dim=0).float().to(dev)  # [D]
        target = target[d0:d1]
        logps, values = [], []
        for (out,), n, best in decision_forwards(self.actor, self.decisions, d0, d1, dev):
            out = out.reshape(-1, n, 2)
            best = best[:, None]
            logp = torch.log_softmax(out[:, :, 0], dim=1)
            logps.append(logp.gather(1, best)[:, 0])
            values.append(out[:, :, 1].gather(1, best)[:, 0])
        logps, values = torch.stack(logps, dim=1), torch.stack(values, dim=1)  # [D, steps]
        outcome_loss = ((values - target[:, None]) ** 2).mean(dim=1)
        policy_loss = -logps.sum(dim=1)
        return (outcome_loss + policy_loss).sum()

    round_loss = loss  # what learn_round steps on
