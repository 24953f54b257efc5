"""Agents on the hot path (reference registry: rl_6_nimmt/agents/__init__.py:33-53).

Kept: Agent, DrunkHamster ("random"), MCSAgent ("mcts"), PolicyMCSAgent
("pmcs"), PUCTAgent ("puct"), BatchedReinforceAgent ("reinforce"),
BatchedACERAgent ("acer") and PUCTCustomedAgent (exported, not in the
registry -- as in the reference).

The DQN family's four base agents -- DQNVanilla ("dqn"), DDQNAgent ("ddqn"),
DQN_PRBAgent ("dqn_prb"), DDQN_PRBAgent ("ddqn_prb") -- are drop-ins on the
device prioritised replay (rl_6_nimmt/replay.py) and registered in
DQN_AGENTS, not in AGENTS.  The batched league seats them through
league.engine_kind -> "dqn" (dqn.BatchedDQN on the replay's payload ring);
league.agent_kind, the registry's map, still raises NotImplementedError for
them.  The duelling and n-step variants -- DuellingDQNAgent ("duelling_dqn"),
DuellingDDQNAgent ("duelling_ddqn"), DuellingDDQN_PRBAgent
("duelling_ddqn_prb"), DQN_NStep_Agent ("dqn_nstep"), D3QN_PRB_NStep
("d3qn_prb_nstep") -- are registered in DQN_VARIANT_AGENTS and take the same
seat.  So do the noisy variants -- Noisy_DQN ("noisy_dqn"), Noisy_D3QN
("noisy_d3qn"), Noisy_D3QN_PRB_NStep ("noisy_d3qn_prb_nstep") -- registered in
DQN_NOISY_AGENTS: the engine gives every decision its own factorised noise
(dqn.BatchedDQN.noisy).  The *_PRB agents deep-copy and pickle with their
device replay (replay.DevicePER.clone), so Tournament.copy_player and evolve
clone a trained one.  A whole league of these agents is checkpointed with
league.BatchedTournament.save / load (the agents through torch.save, their
engines through engine.BatchedEngine.state_dict / load_state_dict, the
handle through VecSechsNimmtEnv.state_dict / load_state_dict).  Not built:
the human UI.
"""
from .base import Agent
from .random import DrunkHamster
from .mcts import BaseMCAgent, MCSAgent, PolicyMCSAgent, PUCTAgent, PUCTCustomedAgent
from .policy import BatchedReinforceAgent
from .actor_critic import BatchedACERAgent
from .dqn import DQNVanilla, DDQNAgent, DQN_PRBAgent, DDQN_PRBAgent
from .dqn import DuellingDQNAgent, DuellingDDQNAgent, DuellingDDQN_PRBAgent, DQN_NStep_Agent, D3QN_PRB_NStep
from .dqn import Noisy_DQN, Noisy_D3QN, Noisy_D3QN_PRB_NStep

HUMAN = "human"
RANDOM_AGENT = "random"
REINFORCE = "reinforce"
ACER = "acer"
DQN = "dqn"
DDQN = "ddqn"
DQN_PRB = "dqn_prb"
DDQN_PRB = "ddqn_prb"
DUELLING_DQN = "duelling_dqn"
DUELLING_DDQN = "duelling_ddqn"
DUELLING_DDQN_PRB = "duelling_ddqn_prb"
DQN_NSTEP = "dqn_nstep"
D3QN_PRB_NSTEP = "d3qn_prb_nstep"
NOISY_DQN = "noisy_dqn"
NOISY_D3QN = "noisy_d3qn"
NOISY_D_QN_PRB_NSTEP = "noisy_d3qn_prb_nstep"
MCS = "mcts"
PMCS = "pmcs"
PUCT = "puct"

AGENTS = {
    RANDOM_AGENT: DrunkHamster,
    REINFORCE: BatchedReinforceAgent,
    ACER: BatchedACERAgent,
    MCS: MCSAgent,
    PMCS: PolicyMCSAgent,
    PUCT: PUCTAgent,
}

DQN_AGENTS = {
    DQN: DQNVanilla,
    DDQN: DDQNAgent,
    DQN_PRB: DQN_PRBAgent,
    DDQN_PRB: DDQN_PRBAgent,
}

DQN_VARIANT_AGENTS = {
    DUELLING_DQN: DuellingDQNAgent,
    DUELLING_DDQN: DuellingDDQNAgent,
    DUELLING_DDQN_PRB: DuellingDDQN_PRBAgent,
    DQN_NSTEP: DQN_NStep_Agent,
    D3QN_PRB_NSTEP: D3QN_PRB_NStep,
}

DQN_NOISY_AGENTS = {
    NOISY_DQN: Noisy_DQN,
    NOISY_D3QN: Noisy_D3QN,
    NOISY_D_QN_PRB_NSTEP: Noisy_D3QN_PRB_NStep,
}
