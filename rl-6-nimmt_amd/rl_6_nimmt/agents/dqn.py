"""Drop-in DQN agents (reference: rl_6_nimmt/agents/dqn.py:42-441).

    DQNVanilla     Q(s,a) <- r + gamma * max_a' Q(s',a')
    DDQNAgent      Q(s,a) <- r + gamma * Q_target(s', argmax_a' Q(s',a')), the
                   target net following softly (tau) every `retrain_interval`
                   steps
    DQN_PRBAgent   DQNVanilla on the prioritised replay: loss = mean(w * err^2),
                   priorities |Q(s,a) - target| written back before the
                   optimiser step
    DDQN_PRBAgent  both
    DuellingDQNAgent, DuellingDDQNAgent, DuellingDDQN_PRBAgent
                   the same three on DuellingDQNNet: Q = V + (A - mean A)
    DQN_NStep_Agent
                   rows of n_steps rewards: reward = sum_i r_{s+i} * gamma ** i,
                   next_state n_steps on, target discount gamma ** n_steps;
                   the last n_steps - 1 rows of an episode are flushed when it
                   ends (fewer terms, done = True)
    D3QN_PRB_NStep all of it: duelling, double, prioritised, n-step -- the
                   agent the reference's author trains

Host-side torch agents with the reference's constructor keywords and
`forward` / `learn` contract, like the other drop-ins; the prioritised replay's
sum tree is the device one (utils/replay_buffer.py -> DevicePER).  Kept from
the reference, because seeded sessions depend on it:
  * epsilon = max(exp(-0.0025 * episode), 0.05) unless `eps_func` is given;
    `train()` resets it to eps_func(0);
  * illegal cards are masked with -1e8 before the arg-max;
  * exploring takes two draws from Python's global `random`: one over all
    actions (discarded when legal actions are given), then one over the legal
    ones; `info["value"]` is -1 then;
  * every step is stored (with the *previous* step's reward, as GameSession
    passes it) and one minibatch is learned once `len(history) > minibatch`;
    `learn` returns np.array([loss]);
  * the n-step reward is a Python float (float64): the target and the loss of
    D3QN_PRB_NStep are float64.  DQN_NStep_Agent on the uniform replay keeps
    the reference's failure too: MSELoss of a float32 q_eval and a float64
    target raises in `backward`;
  * for n_steps > 1 the row that starts n_steps before the end points at the
    terminal observation with done False, and the target uses gamma ** n_steps
    for the truncated rows as well.

    Noisy_DQN, Noisy_D3QN, Noisy_D3QN_PRB_NStep (reference :234-261,404-424,439)
                   DQNVanilla, DuellingDDQNAgent and D3QN_PRB_NStep on
                   NoisyFactorizedLinear layers (noisy_init_sigma = 0.5): the
                   card is the arg-max of the noisy scores over the legal cards
                   (all 104 when none are given).  No epsilon is used and
                   Python's `random` is not touched; `info` is {"value": ...};
                   `eps` is still updated in `learn`.  The noise of a forward
                   is torch's global generator's: randn for the input buffer,
                   then for the output buffer, layer after layer, in eval mode
                   too.  soft_update runs over parameters(): the sigmas follow,
                   the epsilon buffers do not.
"""
import math
import random

import numpy as np
import torch
from torch import nn

from ..utils.nets import DuellingDQNNet, MultiHeadedMLP, NoisyFactorizedLinear
from ..utils.replay_buffer import History, PriorityReplayBuffer
from .base import Agent

STATE, ACTION, REWARD, NEXT_STATE, DONE = "state", "action", "reward", "next_state", "done"


def eps_func_decay(episode):
    return max(math.exp(-episode * 0.0025), 0.05)


def _q_net(agent, hidden_sizes, activation, **noisy):
    return MultiHeadedMLP(agent.state_length, hidden_sizes=hidden_sizes, head_sizes=(agent.num_actions,),
                          activation=activation, head_activations=(None,), **noisy)


def _duelling_net(agent, hidden_sizes, activation, **noisy):
    return DuellingDQNNet(agent.state_length, hidden_sizes=hidden_sizes, out_size=agent.num_actions,
                          activation=activation, **noisy)


class DQNVanilla(Agent):
    """Deep Q-learning"""

    def __init__(self, *args, hidden_sizes=(64,), activation=nn.ReLU(), n_steps=1, eps_func=None, minibatch=64,
                 summary_writer=None, **kwargs):
        super().__init__(*args, **kwargs)
        self._init_replay_buffer(self.history.max_length)  # the base class made the list-like History
        self.summary_writer = summary_writer
        self.n_steps = n_steps
        self.minibatch = minibatch
        self.eps_func = eps_func_decay if eps_func is None else eps_func
        self.step = 0
        self.eps = 0  # 0: always the best learned action, 1: always a random one
        self._setup_networks(hidden_sizes, activation)

    def _setup_networks(self, hidden_sizes, activation):
        self.dqn_net_local = _q_net(self, hidden_sizes, activation)

    def _init_replay_buffer(self, history_length):
        self.history = History(max_length=history_length, dtype=self.dtype, device=self.device)

    def train(self, mode=True):
        super().train(mode=mode)
        self.dqn_net_local.train()
        self.eps = self.eps_func(0)
        return self

    # ------------------------------------------------------------ acting
    def forward(self, state, **kwargs):
        self.dqn_net_local.eval()
        with torch.no_grad():
            scores = self.dqn_net_local(state)[0]
        self.dqn_net_local.train()
        return self._action_selection(scores, **kwargs)

    def _action_selection(self, scores, **kwargs):
        """epsilon-greedy over the legal cards"""
        legal_actions = kwargs.get("legal_actions", None)
        legal = None if legal_actions is None or len(legal_actions) == 0 else [int(a) for a in legal_actions]
        if legal:
            mask = torch.ones(self.num_actions, dtype=torch.bool)
            mask[legal] = False
            scores[mask] = -1e8
        if random.random() > self.eps:
            q = scores.cpu().numpy()
            action, value = np.argmax(q), np.max(q)
        else:
            action = random.choice(range(self.num_actions))
            if legal:
                action = random.choice(legal)
            value = -1
        return action, {"value": value, "eps": self.eps}

    # ------------------------------------------------------------ learning
    def learn(self, state, reward, action, done, next_state, next_reward, episode_end, num_episode, legal_actions,
              *args, **kwargs):
        self.step += 1
        loss = 0
        self.eps = self.eps_func(num_episode)
        if self.summary_writer is not None and episode_end:
            self.summary_writer.add_scalar("debug/eps", self.eps, num_episode)
        self._store(state=state, reward=reward, action=action, next_state=next_state, done=done)
        if len(self.history) > self._min_history_length():
            loss = self._learn(num_episode, episode_end)
        if done:
            self._finish_episode()
        return np.array([loss])

    def _min_history_length(self):
        return self.minibatch

    def _store(self, **kwargs):
        self.history.store(**kwargs)

    def _finish_episode(self):
        pass

    def _prep_minibatch(self, experiences):
        out = {}
        for key, items in experiences.items():
            if isinstance(items[0], torch.Tensor):
                out[key] = torch.stack(items, dim=0).to(self.device)
            else:
                out[key] = torch.from_numpy(np.array(items))
        return out

    def _learn(self, num_episode, episode_end):
        memory_idx, weights, experiences = self.history.sample(n=self.minibatch)
        batch = self._prep_minibatch(experiences)
        q = self.dqn_net_local(batch[STATE])[0]
        q_eval = torch.squeeze(q.gather(1, batch[ACTION].view(-1, 1)))
        q_target = torch.squeeze(self._calc_reward(batch[NEXT_STATE], batch[REWARD], batch[DONE]))
        if self.summary_writer is not None and episode_end and num_episode % 10 == 0:
            self.summary_writer.add_scalar("debug/bellman_target", q_target.max(), num_episode)
        self._update_memory(q_eval.detach(), q_target.detach(), memory_idx)
        return self._optimize_loss(q_eval, q_target, weights).item()

    def _calc_reward(self, next_states, rewards, done):
        """the vanilla target: the local net's own maximum at the next state"""
        with torch.no_grad():
            best = self.dqn_net_local(next_states)[0].max(dim=-1).values
            return rewards + self.gamma ** self.n_steps * (best * ~(done == 1))

    def _update_memory(self, q_eval, q_target, memory_idx):
        pass

    def _optimize_loss(self, q_eval, q_target, weights):
        loss = nn.functional.mse_loss(q_eval, q_target)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        return loss


class DDQNAgent(DQNVanilla):
    def __init__(self, *args, retrain_interval=4, tau=1e-2, **kwargs):
        self.tau = tau
        self.retrain_interval = retrain_interval
        super().__init__(*args, **kwargs)

    def _setup_networks(self, hidden_sizes, activation):
        self.dqn_net_local = _q_net(self, hidden_sizes, activation)
        self.dqn_net_target = _q_net(self, hidden_sizes, activation)
        self.dqn_net_target.eval()
        self.soft_update(self.dqn_net_local, self.dqn_net_target, 1)  # start from the same parameters

    def _calc_reward(self, next_states, rewards, done):
        """the double-DQN target: the local net picks the action, the target net values it"""
        with torch.no_grad():
            q_target_net = self.dqn_net_target(next_states)[0]
            pick = torch.argmax(self.dqn_net_local(next_states)[0], dim=-1)
            q_next = q_target_net[torch.arange(q_target_net.shape[0]), pick] * ~(done == 1).squeeze()
            q_targets = rewards + self.gamma ** self.n_steps * q_next
        if self.step % self.retrain_interval == 0:
            self.soft_update(self.dqn_net_local, self.dqn_net_target, self.tau)
        return q_targets

    def soft_update(self, local_model, target_model, tau):
        """theta_target = tau * theta_local + (1 - tau) * theta_target"""
        for target_param, local_param in zip(target_model.parameters(), local_model.parameters()):
            target_param.data.copy_(tau * local_param.data + (1 - tau) * target_param.data)


class DQN_PRBAgent(DQNVanilla):
    def _init_replay_buffer(self, history_length):
        self.history = PriorityReplayBuffer(history_length, device=self.device, dtype=self.dtype)

    def _update_memory(self, q_eval, q_target, memory_idx):
        self.history.batch_update(memory_idx, torch.abs(q_eval - q_target).view(memory_idx.shape))

    def _optimize_loss(self, q_eval, q_target, weights):
        weights = torch.from_numpy(weights).to(self.device, self.dtype)
        loss = (weights * (q_eval - q_target) ** 2).mean()
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        return loss


class DDQN_PRBAgent(DQN_PRBAgent, DDQNAgent):
    pass


class DuellingDQNAgent(DQNVanilla):
    """V and A heads on one latent net, Q = V + (A - mean_a A)"""

    def _setup_networks(self, hidden_sizes, activation):
        self.dqn_net_local = _duelling_net(self, hidden_sizes, activation)


class DuellingDDQNAgent(DDQNAgent):
    def _setup_networks(self, hidden_sizes, activation):
        self.dqn_net_local = _duelling_net(self, hidden_sizes, activation)
        self.dqn_net_target = _duelling_net(self, hidden_sizes, activation)  # left in train mode, as the reference's
        self.soft_update(self.dqn_net_local, self.dqn_net_target, 1)


class DQN_NStep_Agent(DQNVanilla):
    def __init__(self, *args, **kwargs):
        self.n_step_buffer = []
        super().__init__(*args, **kwargs)

    def _store(self, **kwargs):
        self.n_step_buffer.append(kwargs)
        if len(self.n_step_buffer) < self.n_steps:
            return
        R = sum([self.n_step_buffer[i][REWARD] * (self.gamma ** i) for i in range(self.n_steps)])
        experience = self.n_step_buffer.pop(0)
        experience[REWARD] = R
        experience[NEXT_STATE] = kwargs[NEXT_STATE]
        self.history.store(**experience)

    def _finish_episode(self):
        if len(self.n_step_buffer) == 0:
            return
        last = self.n_step_buffer[-1]
        while len(self.n_step_buffer) > 0:
            R = sum([self.n_step_buffer[i][REWARD] * (self.gamma ** i) for i in range(len(self.n_step_buffer))])
            experience = self.n_step_buffer.pop(0)
            experience[REWARD] = R
            experience[NEXT_STATE] = last[NEXT_STATE]
            experience[DONE] = True
            self.history.store(**experience)


class DuellingDDQN_PRBAgent(DQN_PRBAgent, DuellingDDQNAgent):
    pass


class D3QN_PRB_NStep(DQN_NStep_Agent, DuellingDDQN_PRBAgent):
    pass


class Noisy_DQN(DQNVanilla):
    """NoisyNet exploration: every forward of the net draws fresh factorised noise, the card is the arg-max"""

    def __init__(self, *args, noisy_init_sigma=0.5, **kwargs):
        self.noisy_init_sigma = noisy_init_sigma
        super().__init__(*args, **kwargs)

    def _setup_networks(self, hidden_sizes, activation):
        self.dqn_net_local = _q_net(self, hidden_sizes, activation, linear=NoisyFactorizedLinear,
                                    init_sigma=self.noisy_init_sigma)

    def _action_selection(self, scores, **kwargs):
        """the best legal card by the noisy scores: no epsilon, no draw from `random`"""
        legal_actions = kwargs.get("legal_actions", None)
        actions = np.arange(self.num_actions)
        q = scores.cpu().numpy()
        if legal_actions is not None and len(legal_actions) > 0:
            legal = [int(a) for a in legal_actions]
            q, actions = q[legal], actions[legal]
        best = np.argmax(q)
        return actions[best], {"value": q[best]}


class Noisy_D3QN(DuellingDDQNAgent, Noisy_DQN):
    def _setup_networks(self, hidden_sizes, activation):
        noisy = dict(linear=NoisyFactorizedLinear, init_sigma=self.noisy_init_sigma)
        self.dqn_net_local = _duelling_net(self, hidden_sizes, activation, **noisy)
        self.dqn_net_target = _duelling_net(self, hidden_sizes, activation, **noisy)
        self.soft_update(self.dqn_net_local, self.dqn_net_target, 1)  # the sigmas too; the epsilon buffers not


class Noisy_D3QN_PRB_NStep(Noisy_D3QN, D3QN_PRB_NStep):
    pass
