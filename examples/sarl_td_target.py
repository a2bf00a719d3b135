#!/usr/bin/env python3
"""The first thing the single-agent learner does with a sampled batch (Simulation-SARL/ddpg_torch.py:67-88), after a
short rollout of E envs (examples/sarl_rollout.py): `sample_buffer` on the device, then the TD target

    target_actions = target_actor(states_);  q' = target_critic(states_, target_actions);  q'[done] = 0
    target = rewards + gamma q'

as two launches (`ddpg_td_target`: `BatchedActor.forward`, then `BatchedCritic.td_target` with the mask and the target
in the critic's own launch), reading the sampled tensors in place.  Trained weights come in with
`load_state_dict(agent.target_actor.state_dict())` / `load_state_dict(agent.target_critic.state_dict())`; the losses,
their gradients and the soft update stay with the learner.

    python examples/sarl_td_target.py [n_envs] [episodes]

Needs an MI355X and the built librisvec.so."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import (BatchedActor, BatchedCritic, OUNoise, SarlReplayBuffer, VecEnviron, ddpg_td_target,  # noqa: E402
                              reference_lanes)

E = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
EPISODES = int(sys.argv[2]) if len(sys.argv) > 2 else 2
V, M, N_STEP, GAMMA = 8, 40, 20, 0.99                    # ddpg_train.py:30-32; a short episode; ddpg_torch.py:13
A, TN = 2 * V + M, M // V
BATCH = E                                                 # E new transitions per step: the learner's batch is of that order
dev = torch.device("cuda:0")

L = reference_lanes()
env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3,
                 n_envs=E, device=dev, seed=0)
env.make_new_game()
actor = BatchedActor(V * (TN + 5), A, 512, 256, device=dev, seed=0)                # ddpg_torch.py:17-19
target_actor = BatchedActor(V * (TN + 5), A, 512, 256, device=dev, seed=0)         # ddpg_torch.py:20-22: starts as a copy
target_critic = BatchedCritic(V * (TN + 5), A, 1024, 512, 256, device=dev, seed=1)  # ddpg_torch.py:23-25
noise = OUNoise(E, A, device=dev, seed=0)
memory = SarlReplayBuffer(4 * N_STEP * E, TN + 5, A, V, device=dev)
mu = torch.zeros(E, A, device=dev)
rollout = env.bind_sarl_rollout(mu, noise=noise, replay=memory)
target_actions, target = torch.empty(BATCH, A, device=dev), torch.empty(BATCH, device=dev)

for ep in range(EPISODES):
    if ep % 100 == 0:
        env.renew_positions()
        env.compute_parms()
    obs = env.sarl_observation()
    for st in range(N_STEP):
        actor.forward(obs, out=mu)
        rollout(done=st == N_STEP - 1)
    states, actions, rewards, states_, dones = memory.sample_buffer(BATCH)
    ddpg_td_target(target_actor, target_critic, states_, rewards, dones, GAMMA, out=target, actions_=target_actions)
    print("episode %d  batch %d rows (%d terminal)  mean reward %.4f  mean target %.4f"
          % (ep, BATCH, int(dones.sum()), float(rewards.mean()), float(target.mean())))
