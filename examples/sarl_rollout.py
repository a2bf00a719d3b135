#!/usr/bin/env python3
"""The single-agent driver's rollout loop (Simulation-SARL/ddpg_train.py:114-185, without the learner) for E envs:
actor -> ONE launch per step (OU exploration noise, clip, power / phase map, get_next_phase, RIS gains + step(), every
agent's observation, the transition store) -> a sampled training batch.  The actor is `BatchedActor`: the reference's
`ActorNetwork.forward` (networks.py:132-141) for every env in one launch, reading the observation the rollout launch
wrote and writing the `mu` it reads, both in place -- two launches per step.  A trained actor's weights come in with
`actor.load_state_dict(agent.actor.state_dict())`; `learn()` and the critics belong to the learner.

    python examples/sarl_rollout.py [n_envs] [episodes]

Needs an MI355X and the built librisvec.so."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import BatchedActor, OUNoise, SarlReplayBuffer, VecEnviron, reference_lanes  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
EPISODES = int(sys.argv[2]) if len(sys.argv) > 2 else 2
V, M, N_STEP, BATCH = 8, 40, 100, 64                     # ddpg_train.py:30-32, 45, 79
A, TN = 2 * V + M, M // V                                 # n_output (:76), theta_number (:46)
dev = torch.device("cuda:0")

L = reference_lanes()
env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3,
                 n_envs=E, device=dev, seed=0)
env.make_new_game()                                       # ddpg_train.py:42
actor = BatchedActor(V * (TN + 5), A, 512, 256, device=dev, seed=0)                            # ddpg_torch.py:17-19, ddpg_train.py:77-78
noise = OUNoise(E, A, device=dev, seed=0)                 # ddpg_torch.py:26
memory = SarlReplayBuffer(4 * N_STEP * E, TN + 5, A, V, device=dev)                            # ddpg_train.py:80 (per env: 400 steps)
mu = torch.zeros(E, A, device=dev)                        # the launch reads the actor's output in place
rollout = env.bind_sarl_rollout(mu, noise=noise, replay=memory)

torch.cuda.synchronize()
t0 = time.perf_counter()
for ep in range(EPISODES):
    if ep % 100 == 0:                                     # ddpg_train.py:120-123
        env.renew_positions()
        env.compute_parms()
    obs = env.sarl_observation()                          # state_old_all (:134-137): zero phase slice before the first step
    ep_reward = torch.zeros(E, device=dev)
    for st in range(N_STEP):
        actor.forward(obs, out=mu)                        # choose_action without the noise (:149), sigmoid head
        rollout(done=st == N_STEP - 1)                    # :151-179 in one launch; obs is the new observation afterwards
        ep_reward += env.tensors["metrics"][:, 0]
    states, actions, rewards, states_, dones = memory.sample_buffer(BATCH)                     # what learn() would start from
    print("episode %d  mean reward %.4f  buffer %d rows  batch %s" % (ep, float(ep_reward.mean()) / N_STEP,
                                                                     min(memory.mem_cntr, memory.mem_size), tuple(states.shape)))
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print("%d envs x %d steps x %d episodes: %.0f env-steps/s (actor included)" % (E, N_STEP, EPISODES, E * N_STEP * EPISODES / dt))
