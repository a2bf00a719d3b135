"""The single-agent (DDPG) learner's first step on a sampled batch (`Simulation-SARL/ddpg_torch.py:80-88`): the target
critic's forward, `CriticNetwork.forward` (`Simulation-SARL/networks.py:66-79`, NET below), and the TD target, for all
rows at once on the GPU.

    s = relu(LN1(fc1 x));  s = LN2(fc2 s);  h = relu(s + action_value(a));  h = relu(LN3(fc3 h));  q = q_w . h + q_b
    y = done ? reward : reward + gamma q

One weight set shared by all rows.  `BatchedCritic.forward` / `td_target` are one launch (`risvec_sarl_critic`);
`ddpg_td_target` is `target_actor.forward` + `target_critic.td_target`, two launches, the sampled tensors read in
place.  `ddpg_soft_update` is the learner's last step, `update_network_parameters` (`ddpg_torch.py:104-130`), for both
target networks in one launch; with pack="device" the next `ddpg_td_target` rebuilds both weight streams in two
launches each.  Nothing here differentiates: the gradient half of `learn()` stays with the learner.  No CPU compute path.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

from . import _native as N
from ._weights import (PACK_RULE, WeightSet, choose_mode, is_f32, out_f32, pack_out, pack_workspace, polyak_pairs, polyak_tau,
                       rows_of, soft_update_tensors, stream_pair, td_args, td_select)
from ._wstream import _WAVES, _by_wave, _frags, _from_wave, _split_scaled, _unfrags, centre_fc1


class CriticGeom(NamedTuple):
    """Layout of the weight stream of `risvec_sarl_critic` (include/risvec.h): fragment rows of 1 KiB in four blocks that
    start at rows `av`, `fc1`, `fc2`, `fc3`; `rows` in all."""
    ks: int
    ksa: int
    ng: int
    mt2: int
    mt3: int
    av: int
    fc1: int
    fc2: int
    fc3: int
    rows: int


def critic_geom(input_dims: int, fc1_dims: int, fc2_dims: int, fc3_dims: int, n_actions: int) -> CriticGeom:
    ks, ksa, ng = (input_dims + 1 + 15) // 16, (n_actions + 15) // 16, fc1_dims // 32
    mt2, mt3 = fc2_dims // (32 * _WAVES), fc3_dims // (32 * _WAVES)
    av = 0
    fc1 = av + _WAVES * ksa * mt2 * 2
    fc2 = fc1 + ng * ks * 2
    fc3 = fc2 + _WAVES * 2 * ng * mt2 * 2
    rows = fc3 + _WAVES * 8 * mt2 * mt3 * 2
    return CriticGeom(ks, ksa, ng, mt2, mt3, av, fc1, fc2, fc3, rows)


def _supported(input_dims: int, fc1_dims: int, fc2_dims: int, fc3_dims: int, n_actions: int) -> bool:
    """The rule of `risvec_sarl_critic_supported`, restated for the pure packing function (the library is the authority:
    tests compare the two)."""
    return (1 <= input_dims <= 128 and fc1_dims >= 32 and fc1_dims % 32 == 0 and fc1_dims <= 1024
            and fc2_dims in (128, 256, 512) and fc3_dims in (128, 256) and 1 <= n_actions <= 96)


def pack_critic_weights(W1, b1, W2, Wav, W3) -> Tuple[torch.Tensor, torch.Tensor]:
    """(wstream [rows, 64, 8] float16, scales [4] float32) of `risvec_sarl_critic` from the float32 Linear weights
    ([out, in]: fc1 and its bias, fc2, action_value, fc3).  A pure function of its arguments; runs on any device, CPU
    included.  The LayerNorm parameters, the other biases and the q layer are read by the kernel as they are."""
    F1, IN = W1.shape
    F2, A, F3 = W2.shape[0], Wav.shape[1], W3.shape[0]
    if not _supported(IN, F1, F2, F3, A):
        raise ValueError("no fused critic kernel for input_dims=%d fc1=%d fc2=%d fc3=%d n_actions=%d" % (IN, F1, F2, F3, A))
    if tuple(b1.shape) != (F1,) or tuple(W2.shape) != (F2, F1) or tuple(Wav.shape) != (F2, A) or tuple(W3.shape) != (F3, F2):
        raise ValueError("pack_critic_weights: the weights' shapes do not chain")
    g = critic_geom(IN, F1, F2, F3, A)
    dev = W1.device
    # fc1 operand [F1, 16 KS]: column k < IN the centred weight, column IN the centred bias
    x1 = torch.zeros(F1, 16 * g.ks, dtype=torch.float64, device=dev)
    x1[:, :IN + 1] = centre_fc1(W1, b1).T
    h1, l1, u1 = _split_scaled(x1)
    # (t, g, r, s, h, j) -> (g, s, t, h, r, j): row (g KS + s) 2 + t, lane = 32 h + r
    f1 = torch.stack([h1, l1], 0).reshape(2, g.ng, 32, g.ks, 2, 8).permute(1, 3, 0, 4, 2, 5).reshape(-1, 64, 8)
    wa = torch.zeros(16 * g.ksa, F2, dtype=torch.float32, device=dev)
    wa[:A] = Wav.T
    ha, la, ua = _split_scaled(wa)
    h2, l2, u2 = _split_scaled(W2.T)
    h3, l3, u3 = _split_scaled(W3.T)
    stream = torch.cat([_by_wave(_frags(ha, la, "nat"), g.mt2), f1, _by_wave(_frags(h2, l2, "cd"), g.mt2),
                        _by_wave(_frags(h3, l3, "cd"), g.mt3)], 0).contiguous()
    assert stream.shape[0] == g.rows
    return stream, torch.stack([u1, u2, ua, u3]).float().contiguous()


def pack_critic_weights_device(W1, b1, W2, Wav, W3, out=None, workspace=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`pack_critic_weights` computed on the device by `risvec_sarl_critic_pack` (csrc/k_sarl_critic_pack.hip): two launches
    on the current stream, the float32 weights read in place, no copy and no synchronisation.  out: (wstream, scales)
    to write into, every byte of them (default: new tensors); workspace: a uint8 tensor of
    `risvec_sarl_critic_pack_workspace` bytes (default: a new one).  The same function of its arguments as the host
    one, except that the float64 row means of the centred fc1 weight are summed in another order."""
    lib = N.load()
    ws = (W1, b1, W2, Wav, W3)
    if not (isinstance(W1, torch.Tensor) and all(is_f32(t, W1.device) for t in ws)):
        raise ValueError("pack_critic_weights_device: the weights must be contiguous float32 tensors on one device")
    dev = W1.device
    N.require_hip(dev)
    if W1.dim() != 2 or W2.dim() != 2 or Wav.dim() != 2 or W3.dim() != 2:
        raise ValueError("pack_critic_weights_device: W1, W2, Wav and W3 are Linear weights [out, in]")
    (F1, IN), F2, A, F3 = W1.shape, W2.shape[0], Wav.shape[1], W3.shape[0]
    want = dict(b1=(F1,), W2=(F2, F1), Wav=(F2, A), W3=(F3, F2))
    for name, t in zip(("b1", "W2", "Wav", "W3"), ws[1:]):
        if tuple(t.shape) != want[name]:
            raise ValueError("pack_critic_weights_device: %s has shape %s, W1 %s and W2 %s ask for %s"
                             % (name, tuple(t.shape), tuple(W1.shape), tuple(W2.shape), want[name]))
    need = int(lib.risvec_sarl_critic_pack_workspace(IN, F1, F2, F3, A))
    if need == 0:
        raise ValueError("no fused critic kernel for input_dims=%d fc1=%d fc2=%d fc3=%d n_actions=%d" % (IN, F1, F2, F3, A))
    g = critic_geom(IN, F1, F2, F3, A)
    stream, scales = pack_out(out, (g.rows, 64, 8), 4, "pack_critic_weights_device: out", dev)
    workspace = pack_workspace(workspace, need, "pack_critic_weights_device", dev)
    N.check(lib.risvec_sarl_critic_pack(IN, F1, F2, F3, A, *(t.data_ptr() for t in ws), stream.data_ptr(),
                                        stream.numel() * stream.element_size(), scales.data_ptr(), workspace.data_ptr(),
                                        workspace.numel(), N.stream(dev)))
    return stream, scales


def unpack_critic_weights(stream: torch.Tensor, scales: torch.Tensor, input_dims: int, fc1_dims: int, fc2_dims: int,
                          fc3_dims: int, n_actions: int) -> dict:
    """What the kernel multiplies by, as float64: {"fc1" [input_dims + 1, fc1] (centred, the bias last), "fc2" [fc1, fc2],
    "action_value" [n_actions, fc2], "fc3" [fc2, fc3]} -- hi + lo with the recorded scale undone.  The inverse of
    `pack_critic_weights` up to the split's rounding."""
    g = critic_geom(input_dims, fc1_dims, fc2_dims, fc3_dims, n_actions)
    s, sc = stream.cpu(), scales.cpu().double()
    f = s[g.fc1:g.fc2].double().reshape(g.ng, g.ks, 2, 2, 32, 8)      # (g, s, t, h, r, j)
    x1 = (f[:, :, 0] + f[:, :, 1]).permute(0, 3, 1, 2, 4).reshape(32 * g.ng, 16 * g.ks)   # (g, r, s, h, j)
    return {"fc1": (x1 * sc[0]).T[:input_dims + 1].contiguous(),
            "fc2": _unfrags(_from_wave(s[g.fc2:g.fc3], g.mt2, 2 * g.ng), "cd") * sc[1],
            "action_value": (_unfrags(_from_wave(s[g.av:g.fc1], g.mt2, g.ksa), "nat") * sc[2])[:n_actions].contiguous(),
            "fc3": _unfrags(_from_wave(s[g.fc3:g.rows], g.mt3, 8 * g.mt2), "cd") * sc[3]}


class BatchedCritic(WeightSet):
    """`CriticNetwork` (NET:9-79) for n rows at once.  `input_dims` is the flattened state width, n_agents x per-agent
    width (NET:19); the output is q [n, 1]."""

    GEMM_MODES = ("fused", "library")
    PACK_MODES = ("host", "device")
    #: with gemm=None, batches of fewer rows than this run the library path even where the fused kernel is built
    #: (the measured crossover, profiles/sarl_critic.json; 1 = fused at every row count)
    AUTO_MIN_ROWS = 1
    _WEIGHTS = ("W1", "b1", "ln1_w", "ln1_b", "W2", "b2", "ln2_w", "ln2_b", "W3", "b3", "ln3_w", "ln3_b", "Wav", "bav", "Wq", "bq")
    _SD = {"fc1.weight": "W1", "fc1.bias": "b1", "fc2.weight": "W2", "fc2.bias": "b2", "fc3.weight": "W3", "fc3.bias": "b3",
           "bn1.weight": "ln1_w", "bn1.bias": "ln1_b", "bn2.weight": "ln2_w", "bn2.bias": "ln2_b", "bn3.weight": "ln3_w",
           "bn3.bias": "ln3_b", "action_value.weight": "Wav", "action_value.bias": "bav", "q.weight": "Wq", "q.bias": "bq"}
    _PACKED = ("W1", "b1", "W2", "Wav", "W3")                 # what the weight stream is built from
    _NOUN = "critic"
    _pack_host, _pack_device = staticmethod(pack_critic_weights), staticmethod(pack_critic_weights_device)

    def __init__(self, input_dims: int, n_actions: int, fc1_dims: int = 1024, fc2_dims: int = 512, fc3_dims: int = 256,
                 device="cuda", seed: int = 0, gemm: Optional[str] = None, pack: Optional[str] = None):
        """gemm: how `forward` / `td_target` run.  "fused": one hand-written MFMA launch (`risvec_sarl_critic`: float16
        hi + lo split products at float32 accuracy, the hidden layers never leaving the chip); built for input_dims <=
        128, fc1 % 32 == 0 <= 1024, fc2 in {128, 256, 512}, fc3 in {128, 256}, n_actions <= 96.  "library": `q_torch`,
        the same forward with library kernels only -- the fallback for every other shape and the comparator.
        Default (None): fused where built, for batches of at least `AUTO_MIN_ROWS` rows; library otherwise.
        pack: how the fused kernel's weight stream is rebuilt after a weight update.  "host": `pack_critic_weights`,
        library kernels into new tensors (the default).  "device": `pack_critic_weights_device`, two launches into
        buffers allocated once -- for a target critic that is blended every step (see `soft_update_from`); only where
        the fused kernel covers the shape."""
        lib = N.load()
        self.device = N.resolve_device(device)
        N.require_hip(self.device)
        self.input_dims, self.n_actions = int(input_dims), int(n_actions)
        self.fc1_dims, self.fc2_dims, self.fc3_dims = int(fc1_dims), int(fc2_dims), int(fc3_dims)
        dims = (self.input_dims, self.fc1_dims, self.fc2_dims, self.fc3_dims, self.n_actions)
        if min(dims) < 1:
            raise ValueError("BatchedCritic: every dimension must be >= 1")
        fused_ok = bool(lib.risvec_sarl_critic_supported(*dims))
        shape = "input_dims=%d fc1=%d fc2=%d fc3=%d n_actions=%d" % dims
        self.gemm = choose_mode("gemm", gemm, "fused" if fused_ok else "library", self.GEMM_MODES, fused_ok, shape,
                                "fused: input_dims <= 128, fc1 % 32 == 0 <= 1024, fc2 in {128, 256, 512}, fc3 in {128, 256}, "
                                "n_actions <= 96")
        self.fused_min_rows = self.AUTO_MIN_ROWS if gemm is None else 1
        self.pack = choose_mode("pack", pack, "host", self.PACK_MODES, fused_ok, shape, PACK_RULE)
        self._packed = (None, None)                           # (key, (wstream, scales))
        self._pack_buffers = None                             # pack="device": ((wstream, scales), workspace), at first use
        self.packs = 0                                        # how often the weight stream was rebuilt
        dev = self.device
        g = torch.Generator(device="cpu").manual_seed(seed)

        def uni(*shape, r):
            return ((torch.rand(*shape, generator=g) * 2 - 1) * r).to(dev)
        f1, f2, f3 = 1.0 / math.sqrt(self.fc1_dims), 1.0 / math.sqrt(self.fc2_dims), 1.0 / math.sqrt(self.fc3_dims)   # NET:40-58
        self.W1, self.b1 = uni(self.fc1_dims, self.input_dims, r=f1), uni(self.fc1_dims, r=f1)
        self.W2, self.b2 = uni(self.fc2_dims, self.fc1_dims, r=f2), uni(self.fc2_dims, r=f2)
        self.W3, self.b3 = uni(self.fc3_dims, self.fc2_dims, r=f3), uni(self.fc3_dims, r=f3)
        self.Wq, self.bq = uni(1, self.fc3_dims, r=0.003), uni(1, r=0.003)
        self.Wav, self.bav = uni(self.fc2_dims, self.n_actions, r=f2), uni(self.fc2_dims, r=f2)
        for i, f in ((1, self.fc1_dims), (2, self.fc2_dims), (3, self.fc3_dims)):
            setattr(self, "ln%d_w" % i, torch.ones(f, device=dev))
            setattr(self, "ln%d_b" % i, torch.zeros(f, device=dev))

    def _new_pack_buffers(self):
        dims = (self.input_dims, self.fc1_dims, self.fc2_dims, self.fc3_dims, self.n_actions)
        return (stream_pair((critic_geom(*dims).rows, 64, 8), 4, self.device, torch.zeros),
                torch.zeros(int(N.load().risvec_sarl_critic_pack_workspace(*dims)), dtype=torch.uint8, device=self.device))

    # ------------------------------------------------------------------ forward
    def _rows(self, state, action) -> int:
        n = rows_of(state, self.input_dims, "state", self.device)
        if action is None:
            raise ValueError("action must be a contiguous float32 tensor [n, %d] on %s" % (self.n_actions, self.device))
        N.in_place(action, torch.float32, (n, self.n_actions), "action", self.device)
        return n

    def _fused(self, n: int) -> bool:
        return self.gemm == "fused" and n >= self.fused_min_rows

    def _launch(self, n, state, action, reward, done, gamma, q, y) -> None:
        ws, scales = self._fused_weights()
        p = lambda t: t.data_ptr()   # noqa: E731
        N.check(N.load().risvec_sarl_critic(
            n, self.input_dims, self.fc1_dims, self.fc2_dims, self.fc3_dims, self.n_actions, p(state), p(action), p(ws),
            ws.numel() * ws.element_size(), p(scales), p(self.ln1_w), p(self.ln1_b), p(self.b2), p(self.ln2_w), p(self.ln2_b),
            p(self.bav), p(self.b3), p(self.ln3_w), p(self.ln3_b), p(self.Wq), p(self.bq), N.ptr(reward), N.ptr(done),
            float(gamma), N.ptr(q), N.ptr(y), N.stream(self.device)))

    def forward(self, state: torch.Tensor, action: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """NET:66-79 for every row: state [n, input_dims] or [n, V, input_dims / V], action [n, n_actions], both read in
        place -> q [n, 1].  `out`: a caller-owned [n, 1] tensor written in place."""
        n, dev = self._rows(state, action), self.device
        out = out_f32(out, (n, 1), "forward: out", dev)
        if not self._fused(n):
            return out.copy_(self.q_torch(state.view(n, self.input_dims), action))
        self._launch(n, state, action, None, None, 0.0, out, None)
        return out

    __call__ = forward

    def td_target(self, reward: torch.Tensor, state_: torch.Tensor, action_: torch.Tensor, done: torch.Tensor,
                  gamma: float = 0.99, out: Optional[torch.Tensor] = None, q: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ddpg_torch.py:81, 84-87 in the same launch as the forward: y [n] = reward where done, reward + gamma Q(state_,
        action_) elsewhere (a select, as `critic_value_[done] = 0.0` is).  reward [n] float32, done [n] bool or uint8 (0 / 1),
        all read in place; `out`: a caller-owned [n] tensor for y; `q`: a caller-owned [n, 1] tensor that receives
        Q(state_, action_)."""
        n, dev = self._rows(state_, action_), self.device
        td_args(reward, done, gamma, n, dev)
        out = out_f32(out, (n,), "td_target: out", dev)
        N.in_place(q, torch.float32, (n, 1), "td_target: q", dev)
        if not self._fused(n):
            qv = self.q_torch(state_.view(n, self.input_dims), action_)
            if q is not None:
                q.copy_(qv)
            return td_select(out, reward, done, gamma, qv.view(n))
        d8 = done.view(torch.uint8) if done.dtype == torch.bool else done
        self._launch(n, state_, action_, reward, d8, gamma, q, out)
        return out

    def q_torch(self, x: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
        F = torch.nn.functional
        s = torch.relu(F.layer_norm(F.linear(x, self.W1, self.b1), (self.fc1_dims,), self.ln1_w, self.ln1_b, 1e-5))
        s = F.layer_norm(F.linear(s, self.W2, self.b2), (self.fc2_dims,), self.ln2_w, self.ln2_b, 1e-5)
        h = torch.relu(torch.add(s, F.linear(a, self.Wav, self.bav)))
        h = torch.relu(F.layer_norm(F.linear(h, self.W3, self.b3), (self.fc3_dims,), self.ln3_w, self.ln3_b, 1e-5))
        return F.linear(h, self.Wq, self.bq)

    def forward_torch(self, state: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
        """The same forward with library kernels only (torch.nn.functional.linear / layer_norm): what gemm="library" runs."""
        return self.q_torch(state.reshape(state.shape[0], self.input_dims), action)


def ddpg_td_target(target_actor, target_critic: BatchedCritic, states_: torch.Tensor, rewards: torch.Tensor, dones: torch.Tensor,
                   gamma: float, out: Optional[torch.Tensor] = None, actions_: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ddpg_torch.py:80-81, 84-87 as two launches: `target_actor.forward(states_, out=actions_)` (a `BatchedActor`), then
    `target_critic.td_target(rewards, states_, target_actions, dones, gamma, out=out)`.  The tensors
    `SarlReplayBuffer.sample_buffer` returned are read in place; `actions_` [n, n_actions] and `out` [n] are optional
    caller-owned buffers.  Returns y [n]; `target.view(batch, 1)` (:88) is a view of it."""
    target_actions = target_actor.forward(states_, out=actions_)
    return target_critic.td_target(rewards, states_, target_actions, dones, gamma, out=out)


def ddpg_soft_update(actor, target_actor, critic, target_critic: BatchedCritic, tau: float) -> None:
    """`update_network_parameters` (`ddpg_torch.py:104-130`) for both target networks in ONE launch: all 10 actor and all
    16 critic tensors become tau * online + (1 - tau) * target, in place, bit for bit what the reference's statements
    give on float32 tensors.  `actor` / `critic`: the online networks, each a `BatchedActor` / `BatchedCritic` of the
    target's shape or a mapping under the reference's key names (the learner's `state_dict()`, read in place);
    `target_actor` / `target_critic`: the `Batched*` objects `ddpg_td_target` runs.  tau in [0, 1].  The targets'
    version counters are not advanced; both weight streams are marked stale, so the next `ddpg_td_target` rebuilds them first
    (pack="device": two launches each, into the same buffers).  A refused argument changes nothing."""
    tau = polyak_tau(tau, "ddpg_soft_update")
    if target_actor.device != target_critic.device:
        raise ValueError("ddpg_soft_update: the two target networks must be on one device")
    pairs = polyak_pairs(target_actor, actor, "ddpg_soft_update: actor") + polyak_pairs(target_critic, critic, "ddpg_soft_update: critic")
    soft_update_tensors(pairs, tau, target_critic.device)
    target_actor.mark_stale()
    target_critic.mark_stale()
