#!/usr/bin/env python3
"""The multi-agent learner's TD target (`Global_SAC_Critic.global_learn`, Simulation-MARL-BCD/global_sac_critic.py:287-353
and :394-400) in three launches from a sampled batch, after a short rollout of E envs (examples/rollout.py and
examples/marl_td_target.py, whose loop this is):

    1  policy forward on the sampled next states                       (`risvec_policy_mlp`, inside `sample_normal`)
    2  `BatchedPolicy.sample_normal(states_, masks, out=...)`: per agent `policy.sample_normal(obs_j, mask=mask_j)`
       (:312), the arg-max one-hot and the powers written into next_actions (:326-333) and the log-probabilities added
       up over the agents in agent order (:335-336)                    (`risvec_policy_sample_normal`)
    3  `BatchedTwinCritic.td_target`: both target critics, the minimum, the entropy term, the `done` select (:339-352)

next_actions and the two sums are caller-owned tensors that launch 2 writes and launch 3 reads in place: nothing is
allocated for them per learn step.  The soft update of both target critics (:394-400) is one more launch
(`soft_update_from`).  Trained weights come in with `load_agent_state_dict` / `load_state_dict`; the losses, their
gradients and the optimiser steps stay with the learner.

    python examples/marl_next_actions.py [n_envs] [episodes]

Needs an MI355X and the built librisvec.so."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import (BatchedPolicy, BatchedTwinCritic, NomaGrouper, VecEnviron, VecReplayBuffer,  # noqa: E402
                              apply_yaml_config, reference_lanes)

E = int(sys.argv[1]) if len(sys.argv) > 1 else 256
EPISODES = int(sys.argv[2]) if len(sys.argv) > 2 else 2
V, M, N_STEP, GAMMA, TAU = 8, 40, 20, 0.99, 0.005        # Config defaults of the driver; a short episode
BATCH = 256
dev = torch.device("cuda:0")

L = reference_lanes()
env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3,
                 n_envs=E, device=dev, seed=0)
apply_yaml_config(env, None)
env.make_new_game()
policy = BatchedPolicy(V, 5, 512, 256, device=dev)
grouper = NomaGrouper(env)
memory = VecReplayBuffer(4 * N_STEP * E, 5, V + 2, V, device=dev)
critic = BatchedTwinCritic(5 * V, V * (V + 2), 1024, 512, 256, device=dev, seed=1)          # global_critic1 / 2 (:47-54)
target_critic = BatchedTwinCritic(5 * V, V * (V + 2), 1024, 512, 256, device=dev, seed=1)   # the targets start as copies
log_alpha, entropy_scale = torch.zeros(1, device=dev), 1.0
target, q_next = torch.empty(BATCH, device=dev), (torch.empty(BATCH, 1, device=dev), torch.empty(BATCH, 1, device=dev))
next_actions = torch.empty(BATCH, V * (V + 2), device=dev)                   # written by sample_normal, read by td_target
logp_power, logp_intent = torch.empty(BATCH, device=dev), torch.empty(BATCH, device=dev)

action_env = torch.zeros(E, 2, V, device=dev)
p_off01 = torch.zeros(E, V, device=dev)
action_store = torch.zeros(E, V * (V + 2), device=dev)
env.update_channel_gains()
grouper.begin_episode(0)
mask = grouper.refresh_mask()
partner, n_groups = grouper.group(p_off01, 0)
step = env.bind_step(action_env, partner, n_groups)
group = grouper.bind_group(p_off01)
store = memory.bind_store(None, action_store, env.tensors["metrics"], env.tensors["reward"], env.tensors["obs"], mask)

for ep in range(EPISODES):
    env.begin_episode(ep, env_refresh_every=5)
    grouper.begin_episode(ep)
    for st in range(N_STEP):
        refreshed = env.begin_step(st, ris_every=100)
        if refreshed:
            grouper.refresh_mask()
        policy.choose_action(env.tensors["obs"], mask, cpu_share_floor=env.cpu_share_floor, want_onehot=False,
                             out=(action_env, p_off01, action_store))
        group(st)
        step()
        store(done=(st == N_STEP - 1), use_mask=refreshed)
    states, actions, rewards_g, rewards_l, states_, dones, masks = memory.sample_buffer(BATCH)
    coef = (log_alpha.exp() * entropy_scale).expand(2).contiguous()                           # single alpha: the same value twice
    policy.sample_normal(states_.view(BATCH, V, 5), masks.view(BATCH, V, V), out=(next_actions, logp_power, logp_intent))
    target_critic.td_target(rewards_g, states_, next_actions, dones, GAMMA, logp_power, logp_intent, coef, out=target, q=q_next)
    target_critic.soft_update_from(critic, tau=TAU)
    print("episode %d  batch %d rows (%d terminal)  mean reward %.4f  mean logp power %.4f intent %.4f  mean min-q %.4f  mean target %.4f"
          % (ep, BATCH, int(dones.sum()), float(rewards_g.mean()), float(logp_power.mean()), float(logp_intent.mean()),
             float(torch.minimum(*q_next).mean()), float(target.mean())))
