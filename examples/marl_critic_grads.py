#!/usr/bin/env python3
"""The critic half of the multi-agent learner's step (`Global_SAC_Critic.global_learn`,
Simulation-MARL-BCD/global_sac_critic.py:287-370 and :394-400) with NO autograd graph: examples/marl_critic_update.py with
its stage 2 -- forward, `mse_loss`, `backward()` of the online critics -- replaced by `BatchedTwinCritic.loss_backward`.
Per episode, on a sampled batch:

    1  TD target in three launches (examples/marl_next_actions.py): policy forward, `sample_normal`, `td_target`
    2  the online critics' weight streams, rebuilt on the device after the last optimiser step      (2 launches)
       `loss_backward`: loss = mse(q1, y) + mse(q2, y) and its 16 gradient tensors                  (2 launches: rows, weights)
    3  `BatchedAdam.step(grads=, targets=target_critic, tau=0.005)`: `clip_grad_norm_(.., 1.0)` and `Adam.step()` of both
       critics (:364-370) and the blend of both targets (:394-400)                        (2 launches: sqsum, step)
    4  the two stale weight streams of the target critics, rebuilt on the device          (2 launches)
    5  the next `td_target`                                                              (1 launch)

The online critics are torch.nn modules whose parameters ARE the weights of a `BatchedTwinCritic` (`share_state_dict`), and
the gradient tensors are the parameters' `.grad`: a learner that still calls `backward()` elsewhere sees them where it
expects them.  In the first episode the gradients are compared with autograd's.

    python examples/marl_critic_grads.py [n_envs] [episodes] [batch]

Needs an MI355X and the built librisvec.so."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import (BatchedAdam, BatchedPolicy, BatchedTwinCritic, NomaGrouper, VecEnviron, VecReplayBuffer,  # noqa: E402
                              apply_yaml_config, reference_lanes)
from ris_vec_marl_amd import _native as N  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 256
EPISODES = int(sys.argv[2]) if len(sys.argv) > 2 else 2
BATCH = int(sys.argv[3]) if len(sys.argv) > 3 else 256
V, M, N_STEP, GAMMA, TAU, LR = 8, 40, 20, 0.99, 0.005, 3e-4   # Config defaults of the driver; a short episode
dev = torch.device("cuda:0")


class CriticNetwork(torch.nn.Module):
    """networks.py:7-49: a ReLU MLP on cat([state, action])."""

    def __init__(self, in_dims, fc1=1024, fc2=512, fc3=256):
        super().__init__()
        self.fc1, self.fc2 = torch.nn.Linear(in_dims, fc1), torch.nn.Linear(fc1, fc2)
        self.fc3, self.q = torch.nn.Linear(fc2, fc3), torch.nn.Linear(fc3, 1)

    def forward(self, state, action):
        x = torch.relu(self.fc1(torch.cat([state, action], dim=1)))
        return self.q(torch.relu(self.fc3(torch.relu(self.fc2(x)))))


L = reference_lanes()
env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3,
                 n_envs=E, device=dev, seed=0)
apply_yaml_config(env, None)
env.make_new_game()
policy = BatchedPolicy(V, 5, 512, 256, device=dev)
grouper = NomaGrouper(env)
memory = VecReplayBuffer(4 * N_STEP * E, 5, V + 2, V, device=dev)
torch.manual_seed(1)
online = [CriticNetwork(5 * V + V * (V + 2)).to(dev) for _ in range(2)]                     # global_critic1 / 2 (:47-54)
critic = BatchedTwinCritic(5 * V, V * (V + 2), 1024, 512, 256, device=dev, gemm="fused")    # the device path at every batch
critic.pack = "device"                                                                      # its weights change every step
critic.share_state_dict(*(m.state_dict() for m in online))                                  # the same storage, no copy
target_critic = BatchedTwinCritic(5 * V, V * (V + 2), 1024, 512, 256, device=dev, seed=2)   # global_target_critic1 / 2
target_critic.pack = "device"
target_critic.soft_update_from(critic, tau=1.0)                                             # the targets start as copies
optimizer = BatchedAdam([list(m.parameters()) for m in online], lr=LR, max_norm=1.0)        # :364-370, both critics
grads = critic.alloc_grads()                                  # nested like the optimiser's groups, state_dict() order
for m, gs in zip(online, grads):
    for p, g in zip(m.parameters(), gs):
        p.grad = g                                            # the same storage: what backward() would have filled
log_alpha, entropy_scale = torch.zeros(1, device=dev), 1.0
target, y_next = torch.empty(BATCH, device=dev), torch.empty(BATCH, device=dev)
q_online = (torch.empty(BATCH, 1, device=dev), torch.empty(BATCH, 1, device=dev))
loss = torch.empty(1, device=dev)
next_actions = torch.empty(BATCH, V * (V + 2), device=dev)
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
    coef = (log_alpha.exp() * entropy_scale).expand(2).contiguous()
    stages = []
    # 1: the TD target
    policy.sample_normal(states_.view(BATCH, V, 5), masks.view(BATCH, V, V), out=(next_actions, logp_power, logp_intent))
    target_critic.td_target(rewards_g, states_, next_actions, dones, GAMMA, logp_power, logp_intent, coef, out=target)
    stages.append(("td target", ["policy forward", "sample_normal", N.last_kernel()]))
    # 2: the critic losses and their gradients (:355-362), no graph.  loss_backward would rebuild the online critics' streams
    # on its own; done here so the name can be read
    s2, a2 = states.view(BATCH, -1), actions.view(BATCH, -1)
    online_packs = critic.packs
    critic._fused_weights()
    pack_name = N.last_kernel() if critic.packs != online_packs else None
    critic.loss_backward(s2, a2, target, grads=grads, q=q_online, loss=loss)
    stages.append(("loss + gradients", (["2 x [%s]" % pack_name] if pack_name else []) + [N.last_kernel()]))
    assert critic.packs in (online_packs, online_packs + 2)
    if ep == 0:                                               # against autograd, once
        want = torch.autograd.grad(sum(torch.nn.functional.mse_loss(m(s2, a2).view(-1), target) for m in online),
                                   [p for m in online for p in m.parameters()])
        worst = max(float((g - w).abs().max() / w.abs().max()) for g, w in zip((g for gs in grads for g in gs), want))
        print("gradients against autograd: largest relative difference %.2e" % worst)
        assert worst < 1e-4
    # 3: clip, Adam and the blend of both critics
    packs, versions = target_critic.packs, [p._version for m in online for p in m.parameters()]
    norms = optimizer.step(grads=grads, targets=target_critic, tau=TAU)
    stages.append(("optimiser + blend", [N.last_kernel()]))
    assert all(p._version == v + 1 for p, v in zip((p for m in online for p in m.parameters()), versions))
    # 4: the target critics' weight streams (td_target would rebuild them on its own; done here so the name can be read)
    target_critic._fused_weights()
    stages.append(("pack", ["2 x [%s]" % N.last_kernel()]))
    # 5: the next TD target
    target_critic.td_target(rewards_g, states_, next_actions, dones, GAMMA, logp_power, logp_intent, coef, out=y_next)
    stages.append(("next td target", [N.last_kernel()]))
    assert target_critic.packs == packs + 2                   # one rebuild per net, none by td_target
    print("episode %d  batch %d rows (%d terminal)  critic loss %.5f  grad norms %.4f %.4f  mean target %.4f -> %.4f  uploads %d"
          % (ep, BATCH, int(dones.sum()), float(loss), float(norms[0]), float(norms[1]), float(target.mean()),
             float(y_next.mean()), optimizer.table_uploads))
    for name, ks in stages:
        print("  %-18s %s" % (name + ":", " -> ".join(ks)))
    print("  launches after the td target: " + " -> ".join(k for _, ks in stages[1:] for k in ks))
