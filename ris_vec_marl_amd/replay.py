"""f3: the reference's replay buffer (`Simulation-MARL-BCD/buffer.py`, BUF below) kept in
HBM, and the marshalling its driver does around `env.step()` (`marl_train_bcd.py`, TRAIN).

`VecReplayBuffer` has buffer.py's constructor, attribute names and two methods
(`store_transition`, `sample_buffer`, BUF:16-37); `store_batch` appends the E transitions of one
vectorised step in a single launch, reading the step kernel's outputs in place (obs, reward,
metrics[:,0], the NOMA mask).  `marshal_actions` is TRAIN:1386-1396, 1601-1608, 1776-1784 for all
envs.  No CPU path: every method launches HIP kernels through the C ABI (`risvec_replay_*`,
`risvec_marshal_actions`).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native as N


class VecReplayBuffer:
    """ReplayBuffer(max_size, input_shape, n_actions, n_agents) of BUF:3-14, arrays on `device`."""

    def __init__(self, max_size: int, input_shape: int, n_actions: int, n_agents: int, device="cuda", seed: int = 0):
        N.load()
        self.device = N.resolve_device(device)
        N.require_hip(self.device)
        self.mem_size = int(max_size)
        self.mem_cntr = 0
        self.input_shape, self.n_actions, self.n_agents = int(input_shape), int(n_actions), int(n_agents)
        self.seed = int(seed)
        self._samples = 0
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=self.device)   # noqa: E731
        S, A, L = self.input_shape * self.n_agents, self.n_actions * self.n_agents, self.n_agents
        self.state_memory = z(self.mem_size, S)
        self.action_memory = z(self.mem_size, A)
        self.reward_global_memory = z(self.mem_size)
        self.reward_local_memory = z(self.mem_size, L)
        self.new_state_memory = z(self.mem_size, S)
        self.terminal_memory = z(self.mem_size, dt=torch.bool)
        self.mask_memory = z(self.mem_size, L * L)
        rb = N.RisVecReplay()
        rb.n_agents, rb.input_shape, rb.n_actions, rb.mem_size = L, self.input_shape, self.n_actions, self.mem_size
        for k in ("state_memory", "action_memory", "reward_global_memory", "reward_local_memory", "new_state_memory",
                  "terminal_memory", "mask_memory"):
            setattr(rb, k, getattr(self, k).data_ptr())
        self._c = rb

    # ------------------------------------------------------------------ stores
    # Both stores have ONE implementation, `_bind_store(conv, ...)`: validate, marshal once, return the launcher.  `conv`
    # is the whole difference between the twins: `bind_store` passes `N.in_place` (inputs read in place on every call, so
    # used as they are or refused), `store_batch` passes `N.converted` (copied if needed) and calls the launcher once.
    def store_batch(self, state: torch.Tensor, action: Optional[torch.Tensor], reward_g: torch.Tensor, reward_l: torch.Tensor,
                    state_: torch.Tensor, done=False, mask: Optional[torch.Tensor] = None,
                    policy_out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> None:
        """n consecutive store_transition calls (BUF:16-25), env 0 first.  state / state_ [n, ...]
        (any trailing shape with input_shape*n_agents elements, e.g. the env's obs [E,V,5]); action
        [n, n_actions*n_agents]; reward_g [n] or an [n, k] tensor whose column 0 is used
        (the env's metrics); reward_l [n, n_agents]; done: bool or [n] bool/uint8; mask [n, A, A]
        uint8/bool (the NOMA mask) or None = all ones (TRAIN:1786-1787).
        `action=None, policy_out=(power_raw [n,A,2], probs [n,A,A])`: the action row is built in the store kernel
        from the policy outputs (what `marshal_actions` would have written, TRAIN:1386-1390, 1776-1784)."""
        per_row = None if isinstance(done, (bool, np.bool_, int)) else done
        self._bind_store(N.converted, state, action, reward_g, reward_l, state_, N.mask_u8(mask), policy_out,
                         per_row)(done=per_row is None and bool(done))

    def bind_store(self, state: Optional[torch.Tensor], action: Optional[torch.Tensor], reward_g: torch.Tensor,
                   reward_l: torch.Tensor, state_: torch.Tensor, mask: Optional[torch.Tensor] = None,
                   policy_out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """`store_batch` with the arguments validated and marshalled once: returns `launch(done=False,
        use_mask=True)`, one pre-built C-ABI call that appends the CURRENT contents of the given
        tensors (they are read in place every call: the env's obs / reward / metrics, the marshalled
        action rows, the NOMA mask).  All tensors must be contiguous float32 (mask uint8) on the device;
        reward_g may be the env's [E, k] metrics tensor (column 0 is read).
        `state=None`: the buffer carries the previous step's `state_` forward itself (the store kernel
        drops a copy of `state_` into a ping-pong buffer while it has it in registers), i.e. the
        driver's `marl_state_old_all = marl_state_new_all` (TRAIN:1277, 1774) without a copy kernel;
        the first call then stores the CURRENT `state_` as `state`.
        `action=None, policy_out=(power_raw, probs)`: the action row is built in the store kernel from the policy
        outputs, read in place (no marshalling launch; see `store_batch`)."""
        return self._bind_store(N.in_place, state, action, reward_g, reward_l, state_, mask, policy_out)

    def _bind_store(self, conv, state, action, reward_g, reward_l, state_, mask, policy_out, done_rows=None):
        n = int(state_.shape[0])
        S, A, L = self.input_shape * self.n_agents, self.n_actions * self.n_agents, self.n_agents

        def rows(x, width, name, dtype=torch.float32):
            """x [n, ...] of `width` elements per row, whatever its trailing shape (only its memory is handed on)."""
            if x is None:
                return None
            t = x if isinstance(x, torch.Tensor) else torch.as_tensor(x)
            if t.numel() != n * width:
                raise ValueError("%s must hold n = %d rows of %d elements, got shape %s" % (name, n, width, tuple(t.shape)))
            return conv(t, dtype, t.shape, name, self.device)
        st2, rl = rows(state_, S, "state_"), rows(reward_l, L, "reward_l")
        carry, st = None, rows(state, S, "state")
        if st is None:
            carry = [st2.detach().clone(), torch.empty_like(st2)]
        if action is not None:
            fn, act = N.load().risvec_replay_store, (rows(action, A, "action"),)
        elif policy_out is None:
            raise ValueError("give action or policy_out=(power_raw [n,A,2], probs [n,A,A])")
        elif self.n_actions != L + 2:
            raise ValueError("the policy-output form needs n_actions = n_agents + 2")
        else:
            fn = N.load().risvec_replay_store_policy
            act = (rows(policy_out[0], L * 2, "power_raw"), rows(policy_out[1], L * L, "probs"))
        rg = reward_g if isinstance(reward_g, torch.Tensor) else torch.as_tensor(reward_g)
        if rg.dim() < 1 or rg.shape[0] != n:
            raise ValueError("reward_g must have n = %d rows, got shape %s" % (n, tuple(rg.shape)))
        rg = conv(rg, torch.float32, rg.shape, "reward_g", self.device)     # [n], or [n, k] whose column 0 is read
        mk, dn = rows(mask, L * L, "mask", torch.uint8), rows(done_rows, 1, "done", torch.uint8)
        check, rb, stream = N.check, C.byref(self._c), N.stream(self.device)
        p_st, p_act, p_mk = N.ptr(st), tuple(t.data_ptr() for t in act), N.ptr(mk)
        tail = (rg.data_ptr(), int(rg.stride(0)), rl.data_ptr(), st2.data_ptr(), N.ptr(dn))
        flip = [0]

        def launch(done: bool = False, use_mask: bool = True) -> None:
            if carry is None:
                src, dst = p_st, None
            else:
                src, dst = carry[flip[0]].data_ptr(), carry[flip[0] ^ 1].data_ptr()
                flip[0] ^= 1
            check(fn(rb, self.mem_cntr, n, src, *p_act, *tail, 1 if done else 0, p_mk if use_mask else None, dst, stream))
            self.mem_cntr += n

        launch.keepalive = (st, act, rg, rl, st2, mk, dn, carry)
        return launch

    def store_transition(self, state, action, reward_g, reward_l, state_, done, mask_flat) -> None:
        """BUF:16-25 with the reference's signature (one transition; NumPy arrays or tensors)."""
        def row(x):
            t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32))
            return t.reshape(1, -1)
        L = self.n_agents
        mask = mask_flat if isinstance(mask_flat, torch.Tensor) else torch.as_tensor(np.asarray(mask_flat))
        self.store_batch(row(state), row(action), torch.tensor([float(reward_g)], dtype=torch.float32), row(reward_l),
                         row(state_), bool(done), (mask != 0).reshape(1, L, L))

    # ------------------------------------------------------------------ checkpoint
    _ARRAYS = ("state_memory", "action_memory", "reward_global_memory", "reward_local_memory", "new_state_memory",
               "terminal_memory", "mask_memory")

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

    # ------------------------------------------------------------------ sampling
    def sample_buffer(self, batch_size: int, idx: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, ...]:
        """BUF:27-37 -> (states, actions, rewards_g, rewards_l, states_, dones, masks), device tensors.
        `idx` [batch] int64 injects the rows (parity with the reference's np.random.choice draw);
        otherwise rows are drawn by Philox on the device (`last_batch` holds them afterwards)."""
        B = int(batch_size)
        max_mem = min(self.mem_cntr, self.mem_size)
        if max_mem < 1:
            raise ValueError("sample_buffer on an empty buffer")
        S, A, L = self.input_shape * self.n_agents, self.n_actions * self.n_agents, self.n_agents
        dev = self.device
        out = (torch.empty(B, S, device=dev), torch.empty(B, A, device=dev), torch.empty(B, device=dev),
               torch.empty(B, L, device=dev), torch.empty(B, S, device=dev),
               torch.empty(B, dtype=torch.bool, device=dev), torch.empty(B, L * L, device=dev))
        ix = None
        if idx is not None:
            ix = idx.to(dev, torch.int64).contiguous()
            if ix.numel() != B:
                raise ValueError("idx must hold batch_size rows")
            if int(ix.min()) < 0 or int(ix.max()) >= max_mem:
                raise ValueError("idx outside [0, %d)" % max_mem)
        self.last_batch = torch.empty(B, dtype=torch.int64, device=dev)
        self._samples += 1
        N.check(N.load().risvec_replay_sample(C.byref(self._c), max_mem, B, N.ptr(ix), self.seed, self._samples,
                                              *(t.data_ptr() for t in out), self.last_batch.data_ptr(), N.stream(dev)))
        return out


def marshal_actions(power_raw: torch.Tensor, probs: Optional[torch.Tensor], cpu_share_floor: float = 0.10,
                    want_store: bool = True, out: Optional[tuple] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Policy outputs of all agents of all envs -> (action_env [E,2,V], p_off01 [E,V], action_store
    [E, V*(V+2)] or None): TRAIN:1601-1608 (env action), TRAIN:1391-1396 (pairing power) and
    TRAIN:1386-1390 + 1776-1784 (replay action row = per agent [probs_i with zero diagonal, raw
    power_i]).  power_raw [E,V,2] float32 in [-1,1]; probs [E,V,V] float32.  `out` = preallocated
    (action_env, p_off01, action_store) to write into."""
    N.load()
    N.require_hip(power_raw.device)
    E, V = int(power_raw.shape[0]), int(power_raw.shape[1])
    pr = power_raw.to(torch.float32).contiguous()
    if tuple(pr.shape) != (E, V, 2):
        raise ValueError("power_raw must have shape [E, V, 2]")
    pb = None
    if want_store:
        if probs is None or tuple(probs.shape) != (E, V, V):
            raise ValueError("probs must have shape [E, V, V]")
        pb = probs.to(pr.device, torch.float32).contiguous()
    dev = pr.device
    if out is not None:             # preallocated (action_env, p_off01, action_store): stable pointers for bound launches
        action_env, p01, store = out
        N.in_place(action_env, torch.float32, (E, 2, V), "out[0] (action_env)", dev)
        N.in_place(p01, torch.float32, (E, V), "out[1] (p_off01)", dev)
        N.in_place(store if want_store else None, torch.float32, (E, V * (V + 2)), "out[2] (action_store)", dev)
    else:
        action_env = torch.empty(E, 2, V, device=dev)
        p01 = torch.empty(E, V, device=dev)
        store = torch.empty(E, V * (V + 2), device=dev) if want_store else None
    N.check(N.load().risvec_marshal_actions(E, V, pr.data_ptr(), N.ptr(pb), float(cpu_share_floor), action_env.data_ptr(),
                                            p01.data_ptr(), N.ptr(store), N.stream(dev)))
    return action_env, p01, store
