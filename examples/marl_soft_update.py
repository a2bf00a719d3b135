#!/usr/bin/env python3
"""The target side of the multi-agent learner's step with the learner in the loop (`Global_SAC_Critic.global_learn`,
Simulation-MARL-BCD/global_sac_critic.py:287-353, and `update_global_network_parameters`, :394-400, which `global_learn`
calls on every learning step): after a short rollout of E envs (examples/rollout.py), every episode

    sample a batch -> [the optimiser step: stood in for by an in-place perturbation of the online critics' weights]
    -> target = tau online + (1 - tau) target for all 16 tensors of both target critics    (`soft_update_from`, 1 launch)
    -> q1', q2' = target_critic1(states_, next_actions), target_critic2(states_, next_actions)
       y = rewards_g + gamma (min(q1', q2') - coef[0] logp_power - coef[1] logp_intent);  y[done] = rewards_g[done]
                                                                                            (`td_target`, 1 launch)

With `target_critic.pack = "device"` the two weight streams that the blend made stale are rebuilt on the device in two
launches for both nets together, into the same buffers: four launches from "the optimiser stepped" to "the next TD target
is ready", nothing allocated, nothing synchronised.  The gradients, the losses and Adam stay with the learner.

    python examples/marl_soft_update.py [n_envs] [episodes] [batch]

Needs an MI355X and the built librisvec.so."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import (BatchedPolicy, BatchedTwinCritic, NomaGrouper, VecEnviron, VecReplayBuffer,  # noqa: E402
                              apply_yaml_config, reference_lanes)
from ris_vec_marl_amd import _native as N  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 256
EPISODES = int(sys.argv[2]) if len(sys.argv) > 2 else 2
BATCH = int(sys.argv[3]) if len(sys.argv) > 3 else 256
V, M, N_STEP, GAMMA, TAU = 8, 40, 20, 0.99, 0.005        # Config defaults of the driver; a short episode
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
target_critic = BatchedTwinCritic(5 * V, V * (V + 2), 1024, 512, 256, device=dev, seed=2)   # global_target_critic1 / 2
target_critic.pack = "device"
target_critic.soft_update_from(critic, tau=1.0)                                             # the targets start as copies
log_alpha, entropy_scale = torch.zeros(1, device=dev), 1.0
target, check = torch.empty(BATCH, device=dev), torch.empty(BATCH, device=dev)
gen = torch.Generator(device="cpu").manual_seed(7)

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
    # next actions as :326-333 build them, with library kernels (their construction on the device is not part of this)
    power, probs, _ = policy.choose_action(states_.view(BATCH, V, 5), masks.view(BATCH, V, V), want_onehot=False)
    onehot = torch.nn.functional.one_hot(probs.argmax(-1), V).float()
    next_actions = torch.cat([onehot, power], dim=-1).contiguous()                            # [B, V, V + 2]: read in place
    logp_intent = probs.amax(-1).clamp_min(1e-8).log().sum(-1)                                # [B]
    logp_power = torch.zeros(BATCH, device=dev)
    coef = (log_alpha.exp() * entropy_scale).expand(2).contiguous()                           # single alpha: the same value twice
    for net in critic.nets:                                   # the optimiser step's stand-in: every online tensor moves, in place
        for name in net._WEIGHTS:
            t = getattr(net, name)
            t.add_((torch.randn(t.shape, generator=gen) * 1e-2 * float(t.abs().max())).to(dev))
    launches = []
    target_critic.soft_update_from(critic, tau=TAU)
    launches.append(N.last_kernel())
    # both streams are stale now; td_target below would rebuild them on its own -- done here first only so that the
    # launcher's name can be read (the pack is two launches for both nets: its statistics kernel, then the kernel named)
    packs = target_critic.packs
    streams = [ws.data_ptr() for ws, _ in target_critic._fused_weights()]
    launches.append("2 x [%s]" % N.last_kernel())
    target_critic.td_target(rewards_g, states_, next_actions, dones, GAMMA, logp_power, logp_intent, coef, out=target)
    launches.append(N.last_kernel())
    assert target_critic.packs == packs + 2                   # one rebuild per net and blend, none by td_target
    # as the learner runs it, the rebuild happens inside td_target: the same streams, the same target
    target_critic.mark_stale()
    target_critic.td_target(rewards_g, states_, next_actions, dones, GAMMA, logp_power, logp_intent, coef, out=check)
    assert torch.equal(check, target)
    assert streams == [ws.data_ptr() for ws, _ in target_critic._fused_weights()]
    print("episode %d  batch %d rows (%d terminal)  mean reward %.4f  mean target %.4f  critic rebuilds %d"
          % (ep, BATCH, int(dones.sum()), float(rewards_g.mean()), float(target.mean()), target_critic.packs))
    print("  launches: " + " -> ".join(launches))
