#!/usr/bin/env python3
"""The critic side of the multi-agent learner's actor update (`Global_SAC_Critic.centralized_actor_update`,
Simulation-MARL-BCD/global_sac_critic.py:117-250) with no autograd graph through the critics.  The reference evaluates both
online global critics on (states, actions_pi) (:174-176), takes `q_min = min(q1, q2)` into `actor_global_loss = (alpha *
sum_logp - q_min).mean()` (:224) and lets `backward()` (:246) walk both critics back to `actions_pi` -- forming, and throwing
away, all 16 critic weight gradients on the way.  The policies need ONE tensor from the critics, d q_min / d actions_pi, and
`BatchedTwinCritic.action_grad` gives it in two launches:

    actions_pi, sum_logp = the policies' differentiable sample of the batch           (torch, with a graph)
    dA = critic.action_grad(states, actions_pi.detach(), scale=-1.0 / B)              (2 launches, no graph)
    torch.autograd.backward([entropy_term, actions_pi], [None, dA])                   entropy_term = (alpha * sum_logp).mean()

The policy networks' own backward is OUT OF SCOPE here: `actions_pi` comes from a small differentiable torch stand-in for
the policies (one shared MLP per agent slot: Gumbel-softmax intents and tanh powers, both differentiable, so every action
column carries a gradient), and its backward stays with autograd.  The batch is drawn, not sampled from a replay buffer.  The
example prints the largest difference of the stand-in's parameter gradients against the all-autograd statements of :174-176,
:224 and :246, both measured against the same statements in float64.

    python examples/marl_actor_grads.py [batch]

Needs an MI355X and the built librisvec.so."""
import copy
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import BatchedTwinCritic  # noqa: E402
from ris_vec_marl_amd import _native as N  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
V, OBS = 8, 5                                                 # Config defaults of the driver
S, A = OBS * V, V * (V + 2)
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


class StandInPolicy(torch.nn.Module):
    """NOT the reference's policy: the smallest differentiable map obs -> (intent probabilities [V], two powers, log-probs)
    with the reference's two sampling forms, on noise that is drawn once so that every evaluation sees the same sample."""

    def __init__(self, hidden=64):
        super().__init__()
        self.body = torch.nn.Linear(OBS, hidden)
        self.heads = torch.nn.Linear(hidden, V + 4)           # V intent logits, mu [2], log_std [2]

    def forward(self, states, gumbel, eps):
        h = torch.tanh(self.body(states.view(-1, V, OBS)))
        out = self.heads(h)
        logits, mu, log_std = out[..., :V], out[..., V:V + 2], out[..., V + 2:].clamp(-5.0, 1.0)
        probs = torch.softmax(logits + gumbel, -1)            # Gumbel-softmax, tau = 1
        u = mu + log_std.exp() * eps
        power = torch.tanh(u)
        logp_power = (-0.5 * eps ** 2 - log_std - torch.log(1 - power ** 2 + 1e-6)).sum(-1)
        logp_intent = (probs.detach() * torch.log_softmax(logits, -1)).sum(-1)
        actions_pi = torch.cat([probs, power], -1).reshape(-1, A)                     # per agent [a_probs | a_pwr] (:164)
        return actions_pi, (logp_power + logp_intent).sum(-1, keepdim=True)           # sum over agents (:171-172, :222)


torch.manual_seed(1)
online = [CriticNetwork(S + A).to(dev) for _ in range(2)]     # global_critic1 / 2
policy = StandInPolicy().to(dev)
critic = BatchedTwinCritic(S, A, 1024, 512, 256, device=dev, gemm="fused")           # the device path at every batch
critic.pack = "device"
critic.share_state_dict(*(m.state_dict() for m in online))   # the same storage, no copy
alpha_pi = 0.2
g = torch.Generator().manual_seed(5)
states = (torch.rand(B, S, generator=g) * 1.2).to(dev)
gumbel = -torch.log(-torch.log(torch.rand(B, V, V, generator=g).clamp_min(1e-9))).to(dev)
eps = torch.randn(B, V, 2, generator=g).to(dev)
params = list(policy.parameters())


def all_autograd(critics, pol, st, gm, ep):
    """:174-176, :224, :246 as the reference has them -> the policy's parameter gradients"""
    for m in list(critics) + [pol]:
        m.zero_grad(set_to_none=True)
    actions_pi, sum_logp = pol(st, gm, ep)
    q_min = torch.min(critics[0](st, actions_pi), critics[1](st, actions_pi))
    (alpha_pi * sum_logp - q_min).mean().backward()
    return [p.grad.clone() for p in pol.parameters()]


# -- the device form: the graph ends at actions_pi
policy.zero_grad(set_to_none=True)
actions_pi, sum_logp = policy(states, gumbel, eps)
entropy_term = (alpha_pi * sum_logp).mean()
q_min = torch.empty(B, 1, device=dev)
dA = critic.action_grad(states, actions_pi.detach(), q_min=q_min, scale=-1.0 / B)
kernels = N.last_kernel()
torch.autograd.backward([entropy_term, actions_pi], [None, dA])
got = [p.grad.clone() for p in params]
assert all(p.grad is None for m in online for p in m.parameters())    # no critic weight gradient was formed

# -- the all-autograd form, in float32 and, as the yardstick of both, in float64
lib = all_autograd(online, policy, states, gumbel, eps)
assert all(p.grad is not None for m in online for p in m.parameters())       # ... which the reference forms and drops
want = all_autograd([copy.deepcopy(m).double() for m in online], copy.deepcopy(policy).double(), states.double(), gumbel.double(),
                    eps.double())


def worst(gs):
    return max(float((a.double() - w).abs().max() / w.abs().max()) for a, w in zip(gs, want))


print("batch %d rows  actor loss %.5f  mean q_min %.4f  |dA| max %.3e"
      % (B, float(entropy_term.detach() - q_min.mean()), float(q_min.mean()), float(dA.abs().max())))
print("  critic side: %s" % kernels)
print("policy gradients against float64 autograd: largest relative difference device %.3e  autograd float32 %.3e"
      % (worst(got), worst(lib)))
print("policy gradients against autograd: largest relative difference %.2e"
      % max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, lib)))
