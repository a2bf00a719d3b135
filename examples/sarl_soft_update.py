#!/usr/bin/env python3
"""The target side of the single-agent learner's step with the learner in the loop (Simulation-SARL/ddpg_torch.py:67-88
and 104-130): after a short rollout of E envs (examples/sarl_rollout.py), every episode

    sample a batch -> [the optimiser step: stood in for by an in-place perturbation of the online weights]
    -> target = tau online + (1 - tau) target for all 26 tensors of both target networks   (`ddpg_soft_update`, 1 launch)
    -> target_actions = target_actor(states_);  q' = target_critic(states_, target_actions);  q'[done] = 0
       y = rewards + gamma q'                                                              (`ddpg_td_target`, 2 launches)

With pack="device" the two weight streams that the blend made stale are rebuilt on the device in two launches each, into
the same buffers: seven launches from "the optimiser stepped" to "the next TD target is ready", nothing allocated,
nothing synchronised.  The gradients, the losses and Adam stay with the learner.

    python examples/sarl_soft_update.py [n_envs] [episodes]

Needs an MI355X and the built librisvec.so."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import (BatchedActor, BatchedCritic, OUNoise, SarlReplayBuffer, VecEnviron, ddpg_soft_update,  # noqa: E402
                              ddpg_td_target, reference_lanes)
from ris_vec_marl_amd import _native as N  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
EPISODES = int(sys.argv[2]) if len(sys.argv) > 2 else 2
V, M, N_STEP, GAMMA, TAU = 8, 40, 20, 0.99, 0.005        # ddpg_train.py:30-32; a short episode; ddpg_torch.py:13; ddpg_train.py:93
A, TN = 2 * V + M, M // V
IN, BATCH = V * (TN + 5), E
dev = torch.device("cuda:0")

L = reference_lanes()
env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3,
                 n_envs=E, device=dev, seed=0)
env.make_new_game()
actor = BatchedActor(IN, A, 512, 256, device=dev, seed=0, pack="device")            # ddpg_torch.py:17-19
critic = BatchedCritic(IN, A, 1024, 512, 256, device=dev, seed=1, pack="device")    # ddpg_torch.py:23-25 (the online one)
target_actor = BatchedActor(IN, A, 512, 256, device=dev, seed=2, pack="device")
target_critic = BatchedCritic(IN, A, 1024, 512, 256, device=dev, seed=3, pack="device")
ddpg_soft_update(actor, target_actor, critic, target_critic, 1.0)                   # ddpg_torch.py:35: the targets start as copies
noise = OUNoise(E, A, device=dev, seed=0)
memory = SarlReplayBuffer(4 * N_STEP * E, TN + 5, A, V, device=dev)
mu = torch.zeros(E, A, device=dev)
rollout = env.bind_sarl_rollout(mu, noise=noise, replay=memory)
target_actions, target = torch.empty(BATCH, A, device=dev), torch.empty(BATCH, device=dev)
gen = torch.Generator(device="cpu").manual_seed(7)

for ep in range(EPISODES):
    if ep % 100 == 0:
        env.renew_positions()
        env.compute_parms()
    obs = env.sarl_observation()
    for st in range(N_STEP):
        actor.forward(obs, out=mu)
        rollout(done=st == N_STEP - 1)
    states, actions, rewards, states_, dones = memory.sample_buffer(BATCH)
    for net in (actor, critic):                           # the optimiser step's stand-in: every online tensor moves, in place
        for name in net._WEIGHTS:
            t = getattr(net, name)
            t.add_((torch.randn(t.shape, generator=gen) * 1e-2 * float(t.abs().max())).to(dev))
    launches = []
    ddpg_soft_update(actor, target_actor, critic, target_critic, TAU)
    launches.append(N.last_kernel())
    # both streams are stale now; the two forwards below would rebuild them on their own -- done here one by one only so
    # that each launcher's name can be read (a pack is two launches: its statistics kernel, then the kernel named)
    streams = []
    for net in (target_actor, target_critic):
        streams.append(net._fused_weights()[0].data_ptr())
        launches.append("2 x " + N.last_kernel())
    target_actor.forward(states_, out=target_actions)
    launches.append(N.last_kernel())
    target_critic.td_target(rewards, states_, target_actions, dones, GAMMA, out=target)
    launches.append(N.last_kernel())
    assert streams == [target_actor._fused_weights()[0].data_ptr(), target_critic._fused_weights()[0].data_ptr()]
    check = torch.empty(BATCH, device=dev)
    ddpg_td_target(target_actor, target_critic, states_, rewards, dones, GAMMA, out=check)   # the same two launches in one call
    assert torch.equal(check, target)
    print("episode %d  batch %d rows (%d terminal)  mean reward %.4f  mean target %.4f  critic rebuilds %d"
          % (ep, BATCH, int(dones.sum()), float(rewards.mean()), float(target.mean()), target_critic.packs))
    print("  launches: " + " -> ".join(launches))
