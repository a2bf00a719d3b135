#!/usr/bin/env python3
"""Every agent's local TD target of the multi-agent learner (`Agent.local_learn`, Simulation-MARL-BCD/sac_agent.py:263-284,
called once per agent by `Global_SAC_Critic.global_learn`, global_sac_critic.py:373-392) in three launches from a sampled
batch, after a short rollout of E envs (examples/rollout.py and examples/marl_next_actions.py, whose loop this is):

    1  policy forward on the sampled next states                       (`risvec_policy_mlp`, inside `sample_normal`)
    2  `BatchedPolicy.sample_normal(states_)` without a mask, as `local_learn` calls it (:265-266): the powers and the
       per-agent log-probabilities                                     (`risvec_policy_sample_normal`)
    3  `BatchedLocalCritics.td_target(heads=..., power=...)`: per agent the one-hot from the raw logits with the agent's
       own entry masked (:269-274), both local target critics, the minimum, the entropy term and the product with
       (1 - done) gamma (:276-284), for all V agents at once           (`risvec_local_critics`)

`forward_heads` is called once more for the logits (`sample_normal` does not return them), so the script makes four
launches; a learner that keeps the logits saves one.  The target is compared with the same computation by library operators (gemm="library").  Trained
weights come in with `load_agent_state_dict(j, sd1, sd2)` or, by reference, `share_agent_state_dict`; the losses, their
gradients and the optimiser steps stay with the learner.

    python examples/marl_local_targets.py [n_envs] [episodes]

Needs an MI355X and the built librisvec.so."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import (BatchedLocalCritics, BatchedPolicy, NomaGrouper, VecEnviron, VecReplayBuffer,  # noqa: E402
                              apply_yaml_config, reference_lanes)
from ris_vec_marl_amd import _native as N  # noqa: E402

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
critics = BatchedLocalCritics(V, 5, V + 2, 1024, 512, 256, device=dev, seed=1)          # agents[j].q1 / q2 (sac_agent.py:171-176)
targets = BatchedLocalCritics(V, 5, V + 2, 1024, 512, 256, device=dev, seed=1)          # the targets start as copies (:184)
library = BatchedLocalCritics(V, 5, V + 2, 1024, 512, 256, device=dev, seed=1, gemm="library")
for j in range(V):
    library.share_agent_state_dict(j, *[{k: getattr(net, a) for k, a in net._SD.items()} for net in targets.nets[j]])
coef = torch.tensor([0.2, 0.05], device=dev)                                  # alpha_c, alpha_d times the entropy scale
target = torch.empty(V, BATCH, device=dev)
q_next = (torch.empty(V, BATCH, 1, device=dev), torch.empty(V, BATCH, 1, device=dev))

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
    obs_ = states_.view(BATCH, V, 5)
    power, _, logp_power, logp_intent = policy.sample_normal(obs_, sums=False)[:4]            # no mask: sac_agent.py:265-266
    heads = policy.forward_heads(obs_)                                                        # the raw logits of :269
    targets.td_target(rewards_l, obs_, dones, GAMMA, heads=heads, power=power, logp_power=logp_power, logp_intent=logp_intent,
                      coef=coef, out=target, q=q_next)
    kernel = N.last_kernel()
    want = library.td_target(rewards_l, obs_, dones, GAMMA, heads=heads, power=power, logp_power=logp_power,
                             logp_intent=logp_intent, coef=coef)
    agree = float((target - want).abs().max() / want.abs().max().clamp_min(1e-3))
    targets.soft_update_from(None, critics, TAU)                                              # sac_agent.py:305-312, 4 launches
    print("episode %d  batch %d rows x %d agents (%d terminal)  launches: 4 (policy forward x 2, sample_normal, %s)  "
          "mean local reward %.4f  mean min-q %.4f  mean target %.4f  fused vs library %.3g"
          % (ep, BATCH, V, int(dones.sum()), kernel, float(rewards_l.mean()),
             float(torch.minimum(*q_next).mean()), float(target.mean()), agree))
    assert agree < 2e-5
