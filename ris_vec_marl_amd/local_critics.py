"""The multi-agent (SAC) learner's second target computation on a sampled batch: every agent's LOCAL twin target critics
and local TD target (`Agent.local_learn`, `Simulation-MARL-BCD/sac_agent.py:263-284`, called once per agent by
`global_sac_critic.py:373-392`), for all agents and all rows in one launch on the GPU.

    x_j = [obs_[:, j] | action_j]                            per agent j; read in place, never concatenated in memory
    action_j = action_[:, j]                                 explicit form
             = [onehot(argmax masked logits_j) | power[:, j]]          from the policy: the logits of `forward_heads` with
                                                             the agent's own entry REPLACED by finfo.min / 2 (:269-274)
    q_jc = CriticNetwork_jc(x_j)                             c = 1 .. n_nets, each net a `marl_critic._Net`
    t_j  = min(q_j1, q_j2) - (coef[0] logp_power[:, j] + coef[1] logp_intent[:, j])
    y[j] = reward_l[:, j] + ((1 - done) * gamma) * t_j       a product, as :284 is -- not the select of the global target

`BatchedLocalCritics.forward` / `td_target` are one launch (`risvec_local_critics`, csrc/k_local_critics.hip): the net walk
of `risvec_marl_critic` on agent j's weight streams, one grid row of workgroups per agent.  Each net is a `WeightSet`, so
loading, sharing by reference, the Polyak blend and the staleness rules are those of `BatchedTwinCritic`, per agent.
Nothing here differentiates.  No CPU compute path.
"""
from __future__ import annotations

import ctypes as C
from itertools import chain
from typing import Mapping, Optional

import torch

from . import _native as N
from ._critic_nets import CriticNets, draw_net, entropy_args, minus_entropy, net_table, q_net, q_outs
from ._weights import (done_gamma_args, is_f32, load_weight_sets, out_f32, polyak_pairs, polyak_tau, share_weight_sets,
                       soft_update_tensors)


class BatchedLocalCritics(CriticNets):
    """`agents[j].target_q1` / `agents[j].target_q2` (`sac_agent.py:177-182`; `CriticNetwork`, networks.py:7-49) of all
    `n_agents` agents for n rows at once.  `obs_dims` is one agent's observation width, `action_dims` one agent's action
    width (default n_agents + 2: the intent one-hot and the two powers).  `nets[j][c]` is agent j's net c."""

    def __init__(self, n_agents: int, obs_dims: int = 5, action_dims: Optional[int] = None, fc1_dims: int = 1024,
                 fc2_dims: int = 512, fc3_dims: int = 256, n_nets: int = 2, device="cuda", seed: int = 0,
                 gemm: Optional[str] = None):
        """gemm: how `forward` / `td_target` run.  "fused": one hand-written MFMA launch for all agents
        (`risvec_local_critics`); built for 1 <= n_agents <= 16, obs_dims + action_dims <= 128, fc1 % 32 == 0 <= 1024,
        fc2 in {128, 256, 512}, fc3 in {128, 256}.  "library": the same computation with torch.nn.functional, agent by
        agent -- the fallback for every other shape and the comparator.  Default (None): fused where built, for batches
        of at least `AUTO_MIN_ROWS` rows; library otherwise."""
        lib = N.load()
        self.device = N.resolve_device(device)
        N.require_hip(self.device)
        self.n_agents, self.obs_dims = int(n_agents), int(obs_dims)
        self.action_dims = self.n_agents + 2 if action_dims is None else int(action_dims)
        self.fc1_dims, self.fc2_dims, self.fc3_dims = int(fc1_dims), int(fc2_dims), int(fc3_dims)
        self.n_nets = int(n_nets)
        self._dims = (self.obs_dims, self.action_dims, self.fc1_dims, self.fc2_dims, self.fc3_dims)
        if min((self.n_agents,) + self._dims) < 1:
            raise ValueError("BatchedLocalCritics: every dimension must be >= 1")
        if self.n_nets not in (1, 2):
            raise ValueError("BatchedLocalCritics: n_nets must be 1 or 2")
        self._init_modes(gemm, bool(lib.risvec_local_critics_supported(self.n_agents, *self._dims)),
                         "fused: n_agents <= 16, obs_dims + action_dims <= 128, fc1 % 32 == 0 <= 1024, fc2 in {128, 256, "
                         "512}, fc3 in {128, 256}")
        g = torch.Generator(device="cpu").manual_seed(seed)
        IN = self.obs_dims + self.action_dims
        self.nets = [[draw_net(g, IN, *self._dims[2:], self.device) for _ in range(self.n_nets)] for _ in range(self.n_agents)]
        self._flat = list(chain.from_iterable(self.nets))     # agent j's net c at [j n_nets + c], as the kernel's table

    def _shape(self) -> str:
        return "n_agents=%d obs_dims=%d action_dims=%d fc1=%d fc2=%d fc3=%d" % ((self.n_agents,) + self._dims)

    def _all_nets(self) -> list:
        return self._flat

    # ------------------------------------------------------------------ weights
    def _agent(self, j, what: str) -> int:
        if isinstance(j, bool) or not isinstance(j, int) or not 0 <= j < self.n_agents:
            raise ValueError("%s: agent %r is not in [0, %d)" % (what, j, self.n_agents))
        return j

    def _each(self, j: int, sds, what: str) -> list:
        if len(sds) != self.n_nets:
            raise ValueError("%s: %d weight sets given, an agent has %d nets" % (what, len(sds), self.n_nets))
        return [(net, sd, "%s: agent %d net %d" % (what, j, c + 1)) for c, (net, sd) in enumerate(zip(self.nets[j], sds))]

    def state_dict(self) -> list:
        """[agent][net] dicts under the reference's `CriticNetwork.state_dict()` keys (fc1.* fc2.* fc3.* q.*), CPU copies."""
        return [[net.state_dict() for net in pair] for pair in self.nets]

    def load_agent_state_dict(self, j: int, *sds: Mapping[str, object]) -> None:
        """Take `agents[j].target_q1.state_dict()`, `agents[j].target_q2.state_dict()` as they are (tensors or arrays; one
        mapping per net), by copy."""
        load_weight_sets(self._each(self._agent(j, "load_agent_state_dict"), sds, "load_agent_state_dict"))

    def share_agent_state_dict(self, j: int, *sds: Mapping[str, torch.Tensor]) -> None:
        """Use the learner's own tensors as agent j's weights, by reference (one mapping per net): nothing is copied, now
        or later.  An in-place update is seen through the tensors' version counters, and the next call rebuilds the
        weight streams of that agent's nets only.  Tensors must be float32, contiguous, on this object's device and of
        its shapes."""
        share_weight_sets(self._each(self._agent(j, "share_agent_state_dict"), sds, "share_agent_state_dict"))

    def soft_update_from(self, agents, online, tau: float) -> None:
        """`update_network_parameters` (`sac_agent.py:305-312`) of agent `agents` (an index), or of every agent (None):
        each of the 8 weight tensors per net becomes tau * online + (1 - tau) * own, in place, bit for bit what that
        statement gives on float32 tensors, in as few launches as the 32 tensors per launch of `soft_update_tensors`
        allow (an agent with two nets has 16: two agents per launch).  online: for one agent, one mapping per
        net under the reference's key names (contiguous float32 tensors of this object's shapes on its device, read in
        place); for every agent, a sequence of such sequences; either way also a `BatchedLocalCritics` of the same shape.
        The version counters are NOT advanced: the blended nets are marked stale here.  A refused argument changes
        nothing."""
        what = "soft_update_from"
        tau = polyak_tau(tau, what)
        js = list(range(self.n_agents)) if agents is None else [self._agent(agents, what)]
        if isinstance(online, BatchedLocalCritics):
            if (online.n_agents, online.n_nets) + online._dims != (self.n_agents, self.n_nets) + self._dims:
                raise ValueError("%s: online has another shape (%s)" % (what, online._shape()))
            per_agent = {j: tuple(online.nets[j]) for j in js}
        elif agents is None:
            online = list(online)
            if len(online) != self.n_agents:
                raise ValueError("%s: %d agents given, this object has %d" % (what, len(online), self.n_agents))
            per_agent = {j: tuple(online[j]) for j in js}
        else:
            per_agent = {js[0]: tuple(online)}
        pairs = [p for j in js for net, on, w in self._each(j, per_agent[j], what) for p in polyak_pairs(net, on, w)]
        soft_update_tensors(pairs, tau, self.device)
        for j in js:
            for net in self.nets[j]:
                net.mark_stale()

    def _fused_weights(self) -> list:
        """[agent][net] (wstream, scales); each agent's stale nets are rebuilt first, agent by agent
        (`CriticNets._rebuild_stale`: with pack="device" one two-launch pack per agent with stale nets)."""
        for pair in self.nets:
            self._rebuild_stale(pair)
        return [[net._packed[1] for net in pair] for pair in self.nets]

    # ------------------------------------------------------------------ forward
    def _rows(self, obs, action, heads, power, what: str) -> int:
        V, dev = self.n_agents, self.device
        if not is_f32(obs, dev) or obs.dim() != 3 or obs.shape[0] < 1 or tuple(obs.shape[1:]) != (V, self.obs_dims):
            raise ValueError("%s: obs must be a contiguous float32 tensor [n, %d, %d] on %s" % (what, V, self.obs_dims, dev))
        n = int(obs.shape[0])
        if (action is None) == (heads is None):
            raise ValueError("%s: give either the action or heads and power (exactly one of the two forms)" % what)
        if action is not None:
            if power is not None:
                raise ValueError("%s: power belongs to heads, not to an explicit action" % what)
            if not is_f32(action, dev) or action.dim() not in (2, 3) or action.shape[0] != n or action.numel() != n * V * self.action_dims:
                raise ValueError("%s: action must be a contiguous float32 tensor [%d, %d, %d] or [%d, %d] on %s"
                                 % (what, n, V, self.action_dims, n, V * self.action_dims, dev))
        else:
            if self.action_dims != V + 2:
                raise ValueError("%s: heads builds [onehot | power], which needs action_dims == n_agents + 2 (it is %d)"
                                 % (what, self.action_dims))
            if not is_f32(heads, dev, (V, n, 4 + V)):
                raise ValueError("%s: heads must be a contiguous float32 tensor [%d, %d, %d] on %s (what forward_heads returns)"
                                 % (what, V, n, 4 + V, dev))
            if not is_f32(power, dev, (n, V, 2)):
                raise ValueError("%s: heads needs power, a contiguous float32 tensor [%d, %d, 2] on %s" % (what, n, V, dev))
        return n

    def _q_outs(self, q, n: int, what: str):
        """The caller's q buffers as a tuple of n_nets tensors [V, n, 1] (or None)."""
        return q_outs(q, self.n_nets, (self.n_agents, n, 1), what, self.device)

    def _launch(self, n, obs, action, heads, power, reward, done, gamma, coef, lp, li, qs, y) -> None:
        nets = net_table(len(self._flat), self._flat, chain.from_iterable(self._fused_weights()))
        q1 = qs[0] if qs is not None else None
        q2 = qs[1] if qs is not None and self.n_nets == 2 else None
        N.check(N.load().risvec_local_critics(
            n, self.n_agents, *self._dims, self.n_nets, C.cast(nets, C.c_void_p), obs.data_ptr(), N.ptr(action), N.ptr(heads),
            N.ptr(power), N.ptr(reward), N.ptr(done), float(gamma), N.ptr(coef), N.ptr(lp), N.ptr(li), N.ptr(q1), N.ptr(q2),
            N.ptr(y), N.stream(self.device)))

    def next_action_torch(self, heads: torch.Tensor, power: torch.Tensor, j: int) -> torch.Tensor:
        """`sac_agent.py:270-274` for agent j with library operators: [onehot(argmax masked logits) | power_j], [n, V + 2]."""
        logits = heads[j, :, 4:].clone()
        logits[:, j] = torch.finfo(logits.dtype).min / 2
        onehot = torch.nn.functional.one_hot(torch.argmax(logits, dim=-1), num_classes=self.n_agents).float()
        return torch.cat([onehot, power[:, j]], dim=1)

    def q_torch(self, obs: torch.Tensor, action=None, heads=None, power=None) -> tuple:
        """The forward with library kernels only, agent by agent: what gemm="library" runs -> n_nets tensors [V, n, 1]."""
        n, V = obs.shape[0], self.n_agents
        act = None if action is None else action.view(n, V, self.action_dims)
        out = [[] for _ in range(self.n_nets)]
        for j, pair in enumerate(self.nets):
            a = act[:, j] if act is not None else self.next_action_torch(heads, power, j)
            x = torch.cat([obs[:, j], a], dim=1)
            for c, net in enumerate(pair):
                out[c].append(q_net(net, x))
        return tuple(torch.stack(qs, 0) for qs in out)

    def forward(self, obs: torch.Tensor, action: torch.Tensor, out=None):
        """`q1.forward` / `q2.forward` of every agent (`sac_agent.py:287-289`): obs [n, V, obs_dims], action [n, V,
        action_dims] (or [n, V * action_dims]), both read in place -> (q1, q2), each [V, n, 1]; one tensor when n_nets ==
        1.  `out`: caller-owned [V, n, 1] tensors written in place (a pair; one tensor when n_nets == 1)."""
        n, dev = self._rows(obs, action, None, None, "forward"), self.device
        qs = self._q_outs(out, n, "forward: out")
        if qs is None:
            qs = tuple(torch.empty(self.n_agents, n, 1, device=dev) for _ in range(self.n_nets))
        if not self._fused(n):
            for t, v in zip(qs, self.q_torch(obs, action)):
                t.copy_(v)
        else:
            self._launch(n, obs, action, None, None, None, None, 0.0, None, None, None, qs, None)
        return qs if self.n_nets == 2 else qs[0]

    __call__ = forward

    def td_target(self, reward_l: torch.Tensor, obs_: torch.Tensor, done: torch.Tensor, gamma: float = 0.99, *,
                  action_: Optional[torch.Tensor] = None, heads: Optional[torch.Tensor] = None,
                  power: Optional[torch.Tensor] = None, logp_power: Optional[torch.Tensor] = None,
                  logp_intent: Optional[torch.Tensor] = None, coef: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, q=None) -> torch.Tensor:
        """`sac_agent.py:269-284` for every agent in one launch: y [V, n], y[j] = reward_l[:, j] + ((1 - done) * gamma) *
        (min_c Q_jc(obs_[:, j], action_j) - (coef[0] logp_power[:, j] + coef[1] logp_intent[:, j])), a product as the
        reference's statement is.  reward_l [n, V] float32, obs_ [n, V, obs_dims], done [n] bool or uint8 (0 / 1).  The
        next action is either `action_` [n, V, action_dims] or built from `heads` [V, n, 4 + V] (`forward_heads(obs_)`)
        and `power` [n, V, 2] (`sample_normal`'s first output) as the reference does.  logp_power / logp_intent [n, V]
        float32 (`sample_normal`'s per-agent outputs; None: the term is absent), coef a float32 device tensor of 2
        values.  Everything is read in place, and what would have to be copied or converted is refused.  `out`: a
        caller-owned [V, n] tensor for y; `q`: caller-owned [V, n, 1] tensors (a pair; one when n_nets == 1) that receive
        the Q values."""
        what, V, dev = "td_target", self.n_agents, self.device
        n = self._rows(obs_, action_, heads, power, what)
        if not is_f32(reward_l, dev, (n, V)):
            raise ValueError("%s: reward_l must be a contiguous float32 tensor of shape (%d, %d) on %s" % (what, n, V, dev))
        done_gamma_args(done, gamma, n, dev)
        coef = entropy_args(logp_power, logp_intent, coef, ((n, V),), dev)
        out = out_f32(out, (V, n), "td_target: out", dev)
        qs = self._q_outs(q, n, "td_target: q")
        if not self._fused(n):
            qv = self.q_torch(obs_, action_, heads, power)
            if qs is not None:
                for t, v in zip(qs, qv):
                    t.copy_(v)
            t = (torch.minimum(qv[0], qv[1]) if self.n_nets == 2 else qv[0]).view(V, n)
            t = minus_entropy(t, coef, None if logp_power is None else logp_power.t(),
                              None if logp_intent is None else logp_intent.t())
            live = (1 - (done.view(torch.bool) if done.dtype == torch.uint8 else done).float()) * float(gamma)
            return out.copy_(reward_l.t() + live.view(1, n) * t)
        d8 = done.view(torch.uint8) if done.dtype == torch.bool else done
        self._launch(n, obs_, action_, heads, power, reward_l, d8, gamma, coef, logp_power, logp_intent, qs, out)
        return out
