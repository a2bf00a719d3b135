"""f1: the single-agent environment variant, `Simulation-SARL/Environment.py`
(SENV below) - the env `ddpg_torch.py` drives.  Its geometry, mobility, reset and RIS cascade are the
MARL ones; only `step(action_power, action_phase)` differs (SENV:321-359): the phases come from
the agent, the rate is a natural log against sigma^2, local processing follows the cube-root CPU
model, the reward is power + buffer length with two penalties.

`SarlEnviron` is the E=1 facade with the reference's constructor and 6-tuple `step`; batched use
goes through `VecEnviron.sarl_step`, or -- the whole rollout step of `ddpg_train.py:114-185` in one
launch -- `VecEnviron.bind_sarl_rollout` with an `OUNoise` and a `SarlReplayBuffer`.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native as N
from .compat import Environ, Staging
from .params import poisson_cdf_table


class SarlParams:
    """SENV:66-83 class defaults under the reference's attribute names."""

    def __init__(self):
        self.time_fast = 0.001      # SENV:67
        self.bandwidth = 1          # SENV:69 (MHz)
        self.k = 1e-28              # SENV:70
        self.L = 500                # SENV:71
        self.rate = 3               # SENV:78
        self.t_factor1 = 1          # SENV:80
        self.t_factor2 = 0.6        # SENV:81
        self.penalty1 = 2           # SENV:82
        self.penalty2 = 2           # SENV:83

    def to_c(self) -> N.RisVecSarlParams:
        p = N.RisVecSarlParams()
        p.abi_version = N.ABI_VERSION
        p.struct_bytes = N.C.sizeof(N.RisVecSarlParams)
        p.time_fast, p.bandwidth_mhz, p.k_cpu, p.cycles_l = float(self.time_fast), float(self.bandwidth), float(self.k), float(self.L)
        p.t_factor1, p.t_factor2 = float(self.t_factor1), float(self.t_factor2)
        p.penalty1, p.penalty2 = float(self.penalty1), float(self.penalty2)
        p.arrival_rate = float(self.rate)
        p.poisson_cdf[:] = poisson_cdf_table(float(self.rate)).tolist()
        return p


def sarl_action_map(action: torch.Tensor, n_veh: int, M: int):
    """ddpg_train.py:149-158: agent output [E, 2V+M] in [-1,1] -> (action_power [E,2,V],
    action_phase [E,M] in [0, 2 pi)).  Pure data marshalling of the policy output."""
    a = action.clamp(-0.999, 0.999)
    power = torch.stack([(a[:, :n_veh] + 1) / 2, (a[:, n_veh:2 * n_veh] + 1) / 2], dim=1)
    phase = ((a[:, 2 * n_veh:2 * n_veh + M] + 1) / 2) * (math.pi * 2)
    return power.contiguous(), phase.contiguous()


def sarl_observe(env, action_phase: torch.Tensor) -> torch.Tensor:
    """ddpg_train.py:47-73 for all agents: [E, V, M//V + 5] = each agent's slice of the phase
    action followed by the 5-float tail the step kernel wrote into `obs`."""
    E, V = env.n_envs, env.n_veh
    tn = env.M // V
    th = action_phase[:, :tn * V].reshape(E, V, tn)
    return torch.cat([th, env.tensors["obs"]], dim=2)


class OUNoise:
    """`noise.py:OUActionNoise` for E envs: the state `x` [E, n_actions] float32 lives on the device and is advanced in
    place by the rollout launch (`VecEnviron.bind_sarl_rollout(mu, noise=...)`):
    x' = x + theta (mu - x) dt + sigma sqrt(dt) z,  z ~ N(0, 1).
    z is drawn by Philox4x32-10 at (env_offset + e, pair j, step counter, site 11; seed), Box-Muller of the block's
    first two words giving elements 2j and 2j + 1 -- so a batch sharded over devices draws what the whole batch would
    (give every shard the env's `env_offset`)."""

    def __init__(self, n_envs: int, n_actions: int, sigma: float = 0.15, theta: float = 0.2, dt: float = 1e-2,
                 mu: float = 0.0, device="cuda", seed: int = 0, env_offset: int = 0):
        self.device = N.resolve_device(device)
        self.n_envs, self.n_actions = int(n_envs), int(n_actions)
        self.sigma, self.theta, self.dt, self.mu = float(sigma), float(theta), float(dt), float(mu)
        self.seed, self.env_offset = int(seed), int(env_offset)
        self.x = torch.zeros(self.n_envs, self.n_actions, dtype=torch.float32, device=self.device)

    def reset(self) -> None:
        """noise.py:19-20 with x0 = None."""
        self.x.zero_()

    def state_dict(self) -> dict:
        return dict(x=self.x.detach().cpu().clone(),
                    scalars=dict(sigma=self.sigma, theta=self.theta, dt=self.dt, mu=self.mu, seed=self.seed,
                                 env_offset=self.env_offset))

    def load_state_dict(self, sd: dict) -> None:
        self.x.copy_(sd["x"].to(self.device))
        for k, v in sd["scalars"].items():
            setattr(self, k, type(getattr(self, k))(v))


class SarlReplayBuffer:
    """`Simulation-SARL/buffer.py:ReplayBuffer(max_size, input_shape, n_actions, n_agents)` kept in HBM: one row per
    transition, state rows of input_shape * n_agents floats, action rows of n_actions.  The rollout launch appends the
    E transitions of a step itself (`VecEnviron.bind_sarl_rollout(..., replay=...)`); `store_batch` /
    `store_transition` append from tensors.  Storage is float32: the reference keeps float16 states and actions and
    float64 rewards, so bit parity with buffer.py's arrays is not claimed -- rows hold what the env computed."""

    _ARRAYS = ("state_memory", "action_memory", "reward_memory", "new_state_memory", "terminal_memory")

    def __init__(self, max_size: int, input_shape: int, n_actions: int, n_agents: int, device="cuda", seed: int = 0):
        N.load()
        self.device = N.resolve_device(device)
        N.require_hip(self.device)
        self.mem_size, self.mem_cntr = int(max_size), 0
        self.input_shape, self.n_actions, self.n_agents = int(input_shape), int(n_actions), int(n_agents)
        self.seed, self._samples = int(seed), 0
        S = self.input_shape * self.n_agents
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=self.device)   # noqa: E731
        self.state_memory = z(self.mem_size, S)
        self.action_memory = z(self.mem_size, self.n_actions)
        self.reward_memory = z(self.mem_size)
        self.new_state_memory = z(self.mem_size, S)
        self.terminal_memory = z(self.mem_size, dt=torch.bool)
        c = N.RisVecSarlRollout()
        c.struct_bytes, c.mem_size = C.sizeof(N.RisVecSarlRollout), self.mem_size
        for k in self._ARRAYS:
            setattr(c, k, getattr(self, k).data_ptr())
        self._c = c

    def store_batch(self, state: torch.Tensor, action: torch.Tensor, reward: torch.Tensor, state_: torch.Tensor,
                    done=False) -> None:
        """n consecutive store_transition calls (buffer.py:13-21), row 0 first: state / state_ [n, ...] with
        input_shape * n_agents elements per row, action [n, n_actions], reward [n], done a bool or [n]."""
        n = int(action.shape[0])
        if n > self.mem_size:
            raise ValueError("%d transitions do not fit mem_size = %d" % (n, self.mem_size))
        rows = (torch.arange(n, device=self.device) + self.mem_cntr) % self.mem_size
        f = lambda x: torch.as_tensor(x).to(self.device, torch.float32).reshape(n, -1)   # noqa: E731
        self.state_memory.index_copy_(0, rows, f(state))
        self.action_memory.index_copy_(0, rows, f(action))
        self.reward_memory.index_copy_(0, rows, f(reward).reshape(n))
        self.new_state_memory.index_copy_(0, rows, f(state_))
        d = torch.as_tensor(done, device=self.device).to(torch.bool)
        self.terminal_memory.index_copy_(0, rows, d.expand(n) if d.dim() == 0 else d.reshape(n))
        self.mem_cntr += n

    def store_transition(self, state, action, reward, state_, done) -> None:
        """buffer.py:13-21 with the reference's signature (one transition; NumPy arrays or tensors)."""
        row = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32) if not isinstance(x, torch.Tensor) else x).reshape(1, -1)  # noqa: E731
        self.store_batch(row(state), row(action), torch.tensor([float(reward)]), row(state_), bool(done))

    def sample_buffer(self, batch_size: int, idx: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, ...]:
        """buffer.py:23-34 -> (states, actions, rewards, states_, dones), device tensors.  `idx` [batch] int64 injects
        the rows; otherwise they are drawn by Philox on the device from (seed, number of this sample call), uniformly
        in [0, min(mem_cntr, mem_size)) (`last_batch` holds them afterwards)."""
        B = int(batch_size)
        max_mem = min(self.mem_cntr, self.mem_size)
        if max_mem < 1:
            raise ValueError("sample_buffer on an empty buffer")
        S, dev = self.input_shape * self.n_agents, self.device
        out = (torch.empty(B, S, device=dev), torch.empty(B, self.n_actions, device=dev), torch.empty(B, device=dev),
               torch.empty(B, S, device=dev), torch.empty(B, dtype=torch.bool, device=dev))
        ix = None
        if idx is not None:
            ix = idx.to(dev, torch.int64).contiguous()
            if ix.numel() != B:
                raise ValueError("idx must hold batch_size rows")
            if int(ix.min()) < 0 or int(ix.max()) >= max_mem:
                raise ValueError("idx outside [0, %d)" % max_mem)
        self.last_batch = torch.empty(B, dtype=torch.int64, device=dev)
        self._samples += 1
        N.check(N.load().risvec_sarl_replay_sample(C.byref(self._c), S, self.n_actions, max_mem, B, N.ptr(ix), self.seed,
                                                   self._samples, *(t.data_ptr() for t in out),
                                                   self.last_batch.data_ptr(), N.stream(dev)))
        return out

    def state_dict(self) -> dict:
        """The filled part of the ring + its counters (host tensors)."""
        n = min(self.mem_cntr, self.mem_size)
        sd = {k: getattr(self, k)[:n].detach().cpu().clone() for k in self._ARRAYS}
        sd["scalars"] = dict(mem_cntr=self.mem_cntr, mem_size=self.mem_size, samples=self._samples, seed=self.seed)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        s = sd["scalars"]
        if int(s["mem_size"]) != self.mem_size:
            raise ValueError("replay checkpoint has mem_size %d, this buffer %d" % (s["mem_size"], self.mem_size))
        n = min(int(s["mem_cntr"]), self.mem_size)
        for k in self._ARRAYS:
            getattr(self, k)[:n].copy_(sd[k].to(self.device))
        self.mem_cntr, self._samples, self.seed = int(s["mem_cntr"]), int(s["samples"]), int(s["seed"])


class SarlEnviron(Environ):
    """`Simulation-SARL/Environment.py:Environ` surface over one device-resident env."""

    def __init__(self, down_lane, up_lane, left_lane, right_lane, width, height, n_veh, M, control_bit,
                 device: str = "cuda", seed: int = 0):
        super().__init__(down_lane, up_lane, left_lane, right_lane, width, height, n_veh, M, control_bit,
                         device=device, seed=seed)
        object.__setattr__(self, "sarl", SarlParams())
        self.Reward = 0.0

    # the SARL attribute names that differ from / shadow the MARL parameter bag
    def __getattr__(self, name):
        sp = self.__dict__.get("sarl")
        if sp is not None and name in ("t_factor1", "t_factor2", "penalty1", "penalty2"):
            return getattr(sp, name)
        return super().__getattr__(name)

    def __setattr__(self, name, value):
        sp = self.__dict__.get("sarl")
        if sp is not None and name in ("t_factor1", "t_factor2", "penalty1", "penalty2", "rate", "k", "L",
                                       "bandwidth", "time_fast"):
            setattr(sp, name, value)
            if name in ("t_factor1", "t_factor2", "penalty1", "penalty2"):
                return
        super().__setattr__(name, value)

    def _sarl_launch(self, a: np.ndarray, ph: np.ndarray, arrivals) -> None:
        """One env, one step: power | phase | arrivals go to the device in ONE copy (`Staging`) and the launch is
        pre-bound (re-bound when a parameter of `self.sarl` changed), as in `Environ._step_launch`."""
        V, M, vec = self.n_veh, self.M, self._vec
        key = tuple(sorted(vars(self.sarl).items()))
        if self.__dict__.get("_sarl_stage", (None,))[0] != key:
            vec._ensure_device()
            st = Staging(vec.device, (("a", 2 * V, torch.float32, (1, 2, V)), ("ph", M, torch.float32, (1, M)),
                                      ("ar", V, torch.int32, (1, V))))
            d = st.dev
            plain = vec.bind_sarl_step(d["a"], d["ph"], None, sarl_params=self.sarl)
            injected = vec.bind_sarl_step(d["a"], d["ph"], d["ar"], sarl_params=self.sarl)
            object.__setattr__(self, "_sarl_stage", (key, st, plain, injected))
        _, st, plain, injected = self._sarl_stage
        st.host["a"][:] = a.reshape(-1)
        st.host["ph"][:] = ph
        if arrivals is not None:
            st.host["ar"][:] = self._arrivals(arrivals)
        st.upload()
        (plain if arrivals is None else injected)()

    def step(self, action_power, action_phase, arrivals=None):   # noqa: D102  (signature of SENV:321)
        a = np.asarray(action_power, dtype=np.float64)
        ph = np.asarray(action_phase, dtype=np.float64)
        if a.shape != (2, self.n_veh) or ph.shape != (self.M,):
            raise ValueError("step(action_power [2,n_veh], action_phase [M])")
        self.elements_phase_shift_real = action_phase
        self._sarl_launch(a, ph, arrivals)
        self._dirty()
        self.Reward = float(self._host("metrics")[0])
        return (self.Reward, self.DataBuf, self.data_t, self.data_p, self._host("over_power"), self.over_data)
