"""The multi-agent (SAC) learner's first step on a sampled batch (`Simulation-MARL-BCD/global_sac_critic.py:338-352`): the
two target critics' forward -- each a `CriticNetwork.forward` (`Simulation-MARL-BCD/networks.py:38-49`, NET below), a plain
ReLU MLP on `cat([state, action])` -- the minimum, the entropy term and the TD target, for all rows at once on the GPU.

    x   = [state | action]                                   two tensors, read in place; never concatenated in memory
    h1  = relu(fc1 x);  h2 = relu(fc2 h1);  h3 = relu(fc3 h2);  q_c = q(h3)                       c = 1 .. n_nets
    m   = min(q_1, q_2)                                      (n_nets == 1: q_1)
    ent = coef[0] logp_power + coef[1] logp_intent           an absent logp is an absent term
    y   = done ? reward : reward + gamma (m - ent)

`BatchedTwinCritic.forward` / `td_target` are one launch (`risvec_marl_critic`); the log-probability sums arrive as
tensors the learner already has.  `soft_update_from` is `update_global_network_parameters` (:394-400) for both nets in
one launch; with pack="device" the next `td_target` rebuilds both weight streams in two launches in all
(`risvec_marl_critic_pack`).  Nothing here differentiates: the gradient half of `global_learn` stays with the learner.  No CPU compute
path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Mapping, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _native as N
from ._weights import (PACK_RULE, WeightSet, choose_mode, is_f32, load_weight_sets, out_f32, pack_out, pack_workspace, polyak_pairs,
                       polyak_tau, rows_of, share_weight_sets, soft_update_tensors, stream_pair, td_args, td_select)
from ._wstream import _WAVES, _by_wave, _frags, _from_wave, _split_scaled, _unfrags


class MarlCriticGeom(NamedTuple):
    """Layout of one net's weight stream of `risvec_marl_critic` (include/risvec.h): fragment rows of 1 KiB in three
    blocks that start at rows `fc1`, `fc2`, `fc3`; `rows` in all."""
    ks: int
    ng: int
    mt2: int
    mt3: int
    fc1: int
    fc2: int
    fc3: int
    rows: int


def marl_critic_geom(state_dims: int, action_dims: int, fc1_dims: int, fc2_dims: int, fc3_dims: int) -> MarlCriticGeom:
    ks, ng = (state_dims + action_dims + 15) // 16, fc1_dims // 32
    mt2, mt3 = fc2_dims // (32 * _WAVES), fc3_dims // (32 * _WAVES)
    fc1 = 0
    fc2 = fc1 + ng * ks * 2
    fc3 = fc2 + _WAVES * 2 * ng * mt2 * 2
    rows = fc3 + _WAVES * 8 * mt2 * mt3 * 2
    return MarlCriticGeom(ks, ng, mt2, mt3, fc1, fc2, fc3, rows)


def _supported(state_dims: int, action_dims: int, fc1_dims: int, fc2_dims: int, fc3_dims: int) -> bool:
    """The rule of `risvec_marl_critic_supported`, restated for the pure packing function (the library is the authority:
    tests compare the two)."""
    return (state_dims >= 1 and action_dims >= 1 and state_dims + action_dims <= 128 and fc1_dims >= 32
            and fc1_dims % 32 == 0 and fc1_dims <= 1024 and fc2_dims in (128, 256, 512) and fc3_dims in (128, 256))


def pack_marl_critic_weights(W1, W2, W3) -> Tuple[torch.Tensor, torch.Tensor]:
    """(wstream [rows, 64, 8] float16, scales [3] float32) of one net of `risvec_marl_critic` from its float32 Linear
    weights ([out, in]: fc1 over [state | action], fc2, fc3).  A pure function of its arguments; runs on any device, CPU
    included.  The biases and the q layer are read by the kernel as float32, as they are."""
    if W1.dim() != 2 or W2.dim() != 2 or W3.dim() != 2:
        raise ValueError("pack_marl_critic_weights: W1, W2 and W3 are Linear weights [out, in]")
    (F1, IN), F2, F3 = W1.shape, W2.shape[0], W3.shape[0]
    # the rule depends on the two widths through their sum only
    if IN < 2 or not _supported(IN - 1, 1, F1, F2, F3):
        raise ValueError("no fused twin-critic kernel for state_dims + action_dims=%d fc1=%d fc2=%d fc3=%d" % (IN, F1, F2, F3))
    if tuple(W2.shape) != (F2, F1) or tuple(W3.shape) != (F3, F2):
        raise ValueError("pack_marl_critic_weights: the weights' shapes do not chain")
    g = marl_critic_geom(IN - 1, 1, F1, F2, F3)
    x1 = torch.zeros(16 * g.ks, F1, dtype=torch.float32, device=W1.device)
    x1[:IN] = W1.T
    h1, l1, u1 = _split_scaled(x1)
    h2, l2, u2 = _split_scaled(W2.T)
    h3, l3, u3 = _split_scaled(W3.T)
    # fc1: row (g KS + s) 2 + t -- the "nat" fragments in tile order
    stream = torch.cat([_frags(h1, l1, "nat").reshape(-1, 64, 8), _by_wave(_frags(h2, l2, "cd"), g.mt2),
                        _by_wave(_frags(h3, l3, "cd"), g.mt3)], 0).contiguous()
    assert stream.shape[0] == g.rows
    return stream, torch.stack([u1, u2, u3]).float().contiguous()


def pack_marl_critic_weights_device(weights: Sequence, out: Optional[Sequence] = None,
                                    workspace: Optional[torch.Tensor] = None) -> list:
    """`pack_marl_critic_weights` of 1 or 2 nets of one shape, computed on the device by `risvec_marl_critic_pack`
    (csrc/k_marl_critic_pack.hip): two launches in all on the current stream, the float32 weights read in place, no copy
    and no synchronisation.  weights: a sequence of 1 or 2 triples (W1, W2, W3), contiguous float32 tensors on one HIP
    device; out: a matching sequence of (wstream [rows, 64, 8] float16, scales [3] float32) to write into, every byte of
    them (default: new tensors); workspace: a uint8 tensor of at least `risvec_marl_critic_pack_workspace` bytes (default:
    a new one).  -> the list of (wstream, scales) pairs, bit for bit what the host function gives net by net.  What would
    have to be copied or converted is refused with ValueError."""
    what = "pack_marl_critic_weights_device"
    lib = N.load()
    try:
        weights = [tuple(ws) for ws in weights]
    except TypeError:
        raise ValueError("%s: weights is a sequence of 1 or 2 triples (W1, W2, W3)" % what) from None
    n_nets = len(weights)
    if n_nets not in (1, 2) or any(len(ws) != 3 for ws in weights):
        raise ValueError("%s: weights is a sequence of 1 or 2 triples (W1, W2, W3), got %d nets" % (what, n_nets))
    flat = [t for ws in weights for t in ws]
    dev = getattr(flat[0], "device", None)
    if not all(is_f32(t, dev) for t in flat):
        raise ValueError("%s: the weights must be contiguous float32 tensors on one device" % what)
    if dev.type != "cuda":
        raise ValueError("%s: the weights must be on a HIP device (they are read in place; pack_marl_critic_weights runs "
                         "anywhere)" % what)
    N.require_hip(dev)
    if any(t.dim() != 2 for t in flat):
        raise ValueError("%s: W1, W2 and W3 are Linear weights [out, in]" % what)
    (F1, IN), F2, F3 = weights[0][0].shape, weights[0][1].shape[0], weights[0][2].shape[0]
    want = ((F1, IN), (F2, F1), (F3, F2))
    for c, ws in enumerate(weights):
        for name, t, shape in zip(("W1", "W2", "W3"), ws, want):
            if tuple(t.shape) != shape:
                raise ValueError("%s: %s of net %d has shape %s, the shapes of net 1 ask for %s"
                                 % (what, name, c + 1, tuple(t.shape), shape))
    # the rule depends on the two widths through their sum only
    dims = (IN - 1, 1, F1, F2, F3)
    need = int(lib.risvec_marl_critic_pack_workspace(*dims, n_nets)) if IN >= 2 else 0
    if need == 0:
        raise ValueError("no fused twin-critic kernel for state_dims + action_dims=%d fc1=%d fc2=%d fc3=%d" % (IN, F1, F2, F3))
    g = marl_critic_geom(*dims)
    try:
        out = [None] * n_nets if out is None else [tuple(o) for o in out]
    except TypeError:
        raise ValueError("%s: out is a sequence of %d pairs (wstream, scales)" % (what, n_nets)) from None
    if len(out) != n_nets or any(o is not None and len(o) != 2 for o in out):
        raise ValueError("%s: out is a sequence of %d pairs (wstream, scales)" % (what, n_nets))
    out = [pack_out(o, (g.rows, 64, 8), 3, "%s: out[%d]" % (what, c), dev) for c, o in enumerate(out)]
    workspace = pack_workspace(workspace, need, what, dev)
    nets = (N.RisVecMarlCriticPackNet * n_nets)()
    for c, (ws, (stream, scales)) in enumerate(zip(weights, out)):
        nets[c] = N.RisVecMarlCriticPackNet(ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr(), stream.data_ptr(),
                                            stream.numel() * stream.element_size(), scales.data_ptr())
    N.check(lib.risvec_marl_critic_pack(*dims, n_nets, C.cast(nets, C.c_void_p), workspace.data_ptr(), workspace.numel(),
                                        N.stream(dev)))
    return out


def _unpack(stream: torch.Tensor, scales: torch.Tensor, state_dims: int, action_dims: int, fc1_dims: int, fc2_dims: int,
            fc3_dims: int) -> dict:
    """What the kernel multiplies by, as float64: {"fc1" [state_dims + action_dims, fc1], "fc2" [fc1, fc2], "fc3" [fc2,
    fc3]} -- hi + lo with the recorded scale undone.  The inverse of `pack_marl_critic_weights` up to the split's
    rounding."""
    g = marl_critic_geom(state_dims, action_dims, fc1_dims, fc2_dims, fc3_dims)
    s, sc = stream.cpu(), scales.cpu().double()
    return {"fc1": (_unfrags(s[g.fc1:g.fc2].reshape(g.ng, g.ks, 2, 64, 8), "nat") * sc[0])[:state_dims + action_dims].contiguous(),
            "fc2": _unfrags(_from_wave(s[g.fc2:g.fc3], g.mt2, 2 * g.ng), "cd") * sc[1],
            "fc3": _unfrags(_from_wave(s[g.fc3:g.rows], g.mt3, 8 * g.mt2), "cd") * sc[2]}


class _Net(WeightSet):
    """One `CriticNetwork`'s weights (NET:29-32) and weight stream; `BatchedTwinCritic` rebuilds the stale streams of its
    nets together."""
    _WEIGHTS = ("W1", "b1", "W2", "b2", "W3", "b3", "Wq", "bq")
    _SD = {"fc1.weight": "W1", "fc1.bias": "b1", "fc2.weight": "W2", "fc2.bias": "b2", "fc3.weight": "W3", "fc3.bias": "b3",
           "q.weight": "Wq", "q.bias": "bq"}
    _PACKED = ("W1", "W2", "W3")                              # what the weight stream is built from
    _NOUN = "critic"

    def __init__(self, device):
        self.device = device
        self._packed = (None, None)                           # (key, (wstream, scales))
        self._pack_buffers = None                             # pack="device": (wstream, scales), at first use

    packed = property(lambda self: self._packed)              # the cache slot under the name it had before `WeightSet`


class BatchedTwinCritic:
    """`global_target_critic1` / `global_target_critic2` (`global_sac_critic.py:55-62`; `CriticNetwork`, NET:7-49) for n
    rows at once.  `state_dims` is the flattened state width (n_agents x per-agent width), `action_dims` the flattened
    action width (n_agents x per-agent action); the outputs are q [n, 1] per net.  n_nets=1 is one `CriticNetwork`: the
    local critics of `sac_agent.py:276-284` have the same class and the same target form, one call per agent."""

    GEMM_MODES = ("fused", "library")
    PACK_MODES = ("host", "device")
    #: with gemm=None, batches of fewer rows than this run the library path even where the fused kernel is built
    #: (the measured crossover, profiles/marl_critic.json; 1 = fused at every row count)
    AUTO_MIN_ROWS = 1
    _SD = _Net._SD

    def __init__(self, state_dims: int, action_dims: int, fc1_dims: int = 1024, fc2_dims: int = 512, fc3_dims: int = 256,
                 n_nets: int = 2, device="cuda", seed: int = 0, gemm: Optional[str] = None):
        """gemm: how `forward` / `td_target` run.  "fused": one hand-written MFMA launch (`risvec_marl_critic`: float16
        hi + lo split products at float32 accuracy, neither the hidden layers nor the concatenated input ever in memory);
        built for state_dims + action_dims <= 128, fc1 % 32 == 0 <= 1024, fc2 in {128, 256, 512}, fc3 in {128, 256}.
        "library": `forward_torch` and the same epilogue with torch.nn.functional only -- the fallback for every other
        shape (16 vehicles: 80 + 288 inputs) and the comparator.  Default (None): fused where built, for batches of at
        least `AUTO_MIN_ROWS` rows; library otherwise."""
        lib = N.load()
        self.device = N.resolve_device(device)
        N.require_hip(self.device)
        self.state_dims, self.action_dims = int(state_dims), int(action_dims)
        self.fc1_dims, self.fc2_dims, self.fc3_dims = int(fc1_dims), int(fc2_dims), int(fc3_dims)
        self.n_nets = int(n_nets)
        dims = (self.state_dims, self.action_dims, self.fc1_dims, self.fc2_dims, self.fc3_dims)
        if min(dims) < 1:
            raise ValueError("BatchedTwinCritic: every dimension must be >= 1")
        if self.n_nets not in (1, 2):
            raise ValueError("BatchedTwinCritic: n_nets must be 1 or 2")
        fused_ok = bool(lib.risvec_marl_critic_supported(*dims))
        self.gemm = choose_mode("gemm", gemm, "fused" if fused_ok else "library", self.GEMM_MODES, fused_ok, self._shape(),
                                "fused: state_dims + action_dims <= 128, fc1 % 32 == 0 <= 1024, fc2 in {128, 256, 512}, fc3 in "
                                "{128, 256}")
        self.fused_min_rows = self.AUTO_MIN_ROWS if gemm is None else 1
        self._fused_ok = fused_ok
        self._pack = "host"                                   # see `pack`
        self._pack_workspace = None                           # pack="device": one workspace for both nets, at first use
        self.packs = 0                                        # how often a net's weight stream was rebuilt
        dev = self.device
        g = torch.Generator(device="cpu").manual_seed(seed)

        def uni(*shape, r):
            return ((torch.rand(*shape, generator=g) * 2 - 1) * r).to(dev)
        IN = self.state_dims + self.action_dims
        self.nets = []
        for _ in range(self.n_nets):                          # nn.Linear's default ranges (NET:29-32): 1 / sqrt(fan_in)
            net = _Net(dev)
            for w, b, fan_out, fan_in in (("W1", "b1", self.fc1_dims, IN), ("W2", "b2", self.fc2_dims, self.fc1_dims),
                                          ("W3", "b3", self.fc3_dims, self.fc2_dims), ("Wq", "bq", 1, self.fc3_dims)):
                r = 1.0 / math.sqrt(fan_in)
                setattr(net, w, uni(fan_out, fan_in, r=r))
                setattr(net, b, uni(fan_out, r=r))
            self.nets.append(net)

    def _shape(self) -> str:
        return "state_dims=%d action_dims=%d fc1=%d fc2=%d fc3=%d" % (self.state_dims, self.action_dims, self.fc1_dims,
                                                                      self.fc2_dims, self.fc3_dims)

    @property
    def pack(self) -> str:
        """How the fused kernel's weight streams are rebuilt after a weight update.  "host" (the default):
        `pack_marl_critic_weights` once per stale net, library kernels into new tensors.  "device":
        `pack_marl_critic_weights_device`, two launches for all stale nets together into buffers allocated once -- for
        target critics that are blended every learning step (see `soft_update_from`); only where the fused kernel covers
        the shape.  Setting it marks the streams stale; a refused value changes nothing."""
        return self._pack

    @pack.setter
    def pack(self, mode) -> None:
        if choose_mode("pack", mode, None, self.PACK_MODES, self._fused_ok, self._shape(), PACK_RULE) != self._pack:
            self._pack = mode
            self.mark_stale()

    # ------------------------------------------------------------------ weights
    def state_dict(self) -> list:
        """One dict per net under the reference's `CriticNetwork.state_dict()` keys (fc1.* fc2.* fc3.* q.*), CPU copies."""
        return [net.state_dict() for net in self.nets]

    def _each(self, sds, what: str) -> list:
        if len(sds) != self.n_nets:
            raise ValueError("%s: %d weight sets given, this critic has %d nets" % (what, len(sds), self.n_nets))
        return [(net, sd, "%s: net %d" % (what, c + 1)) for c, (net, sd) in enumerate(zip(self.nets, sds))]

    def load_state_dict(self, *sds: Mapping[str, object]) -> None:
        """Take the weights of `global_target_critic1.state_dict()`, `global_target_critic2.state_dict()` as they are
        (tensors or arrays; one mapping per net).  Load checkpoints with `torch.load(..., weights_only=True)`."""
        load_weight_sets(self._each(sds, "load_state_dict"))

    def share_state_dict(self, *sds: Mapping[str, torch.Tensor]) -> None:
        """Use the learner's own tensors as the weights, by reference (one mapping per net under the reference's key
        names): nothing is copied, now or later.  An in-place update of them is seen through their version counters, and
        the next call rebuilds that net's weight stream first.  Tensors must be float32, contiguous, on this critic's
        device and of this critic's shapes."""
        share_weight_sets(self._each(sds, "share_state_dict"))

    def soft_update_from(self, *online, tau: float) -> None:
        """`update_global_network_parameters` (`global_sac_critic.py:394-400`) for every net in ONE launch: each of the 8
        weight tensors per net becomes tau * online + (1 - tau) * own, in place, bit for bit what that statement gives on
        float32 tensors.  online: one mapping per net under the reference's key names (`global_critic1.state_dict()`,
        `global_critic2.state_dict()`; contiguous float32 tensors of this critic's shapes on this critic's device, read in
        place), or one `BatchedTwinCritic` of the same shape.  tau in [0, 1].  The write goes through raw pointers, so the
        tensors' version counters are NOT advanced: the weight streams are marked stale here and the next `forward` /
        `td_target` rebuilds them.  A refused argument changes nothing."""
        tau = polyak_tau(tau, "soft_update_from")
        if len(online) == 1 and isinstance(online[0], BatchedTwinCritic):
            online = tuple(online[0].nets)
        pairs = [p for net, on, what in self._each(online, "soft_update_from") for p in polyak_pairs(net, on, what)]
        soft_update_tensors(pairs, tau, self.device)
        self.mark_stale()

    def mark_stale(self) -> None:
        """Have the next `forward` / `td_target` rebuild the weight streams: for writers that do not advance the weights'
        version counters."""
        for net in self.nets:
            net.mark_stale()

    def _fused_weights(self) -> list:
        """(wstream, scales) of every net; a net's are rebuilt when one of its packed weight tensors is replaced or updated
        in place, or after `mark_stale` (pack="host": library kernels into new tensors, net by net; pack="device": the
        stale nets together in two launches, into the buffers of their first rebuild)."""
        stale = []
        for net in self.nets:
            s = net._stale()
            if s is not None:
                stale.append((net,) + s)
        if stale and self._pack == "device":
            dev = self.device
            if self._pack_workspace is None:
                need = int(N.load().risvec_marl_critic_pack_workspace(self.state_dims, self.action_dims, self.fc1_dims,
                                                                      self.fc2_dims, self.fc3_dims, self.n_nets))
                self._pack_workspace = torch.zeros(need, dtype=torch.uint8, device=dev)
            rows = marl_critic_geom(self.state_dims, self.action_dims, self.fc1_dims, self.fc2_dims, self.fc3_dims).rows
            for net, _, _ in stale:
                if net._pack_buffers is None:
                    net._pack_buffers = stream_pair((rows, 64, 8), 3, dev, torch.zeros)
            pack_marl_critic_weights_device([ws for _, _, ws in stale], out=[net._pack_buffers for net, _, _ in stale],
                                            workspace=self._pack_workspace)
            for net, key, _ in stale:
                net._packed = (key, net._pack_buffers)
        else:
            for net, key, ws in stale:
                net._packed = (key, pack_marl_critic_weights(*ws))
        self.packs += len(stale)
        return [net._packed[1] for net in self.nets]

    # ------------------------------------------------------------------ forward
    def _rows(self, state, action) -> int:
        n = rows_of(state, self.state_dims, "state", self.device)
        return rows_of(action, self.action_dims, "action", self.device, n)

    def _q_outs(self, q, n: int, what: str):
        """The caller's q buffers as a tuple of n_nets tensors [n, 1] (or None)."""
        if q is None:
            return None
        if isinstance(q, torch.Tensor):
            q = (q,)
        q = tuple(q)
        if len(q) != self.n_nets:
            raise ValueError("%s must hold %d tensors of shape (%d, 1)" % (what, self.n_nets, n))
        for t in q:
            if t is None:
                raise ValueError("%s must hold %d tensors of shape (%d, 1)" % (what, self.n_nets, n))
            N.in_place(t, torch.float32, (n, 1), what, self.device)
        if self.n_nets == 2 and q[0].data_ptr() == q[1].data_ptr():
            raise ValueError("%s: the two tensors are the same" % what)
        return q

    def _fused(self, n: int) -> bool:
        return self.gemm == "fused" and n >= self.fused_min_rows

    def _launch(self, n, state, action, reward, done, gamma, coef, lp, li, qs, y) -> None:
        nets = (N.RisVecMarlCriticNet * self.n_nets)()
        for c, (net, (ws, scales)) in enumerate(zip(self.nets, self._fused_weights())):
            nets[c] = N.RisVecMarlCriticNet(ws.data_ptr(), ws.numel() * ws.element_size(), scales.data_ptr(), net.b1.data_ptr(),
                                            net.b2.data_ptr(), net.b3.data_ptr(), net.Wq.data_ptr(), net.bq.data_ptr())
        q1 = qs[0] if qs is not None else None
        q2 = qs[1] if qs is not None and self.n_nets == 2 else None
        N.check(N.load().risvec_marl_critic(
            n, self.state_dims, self.action_dims, self.fc1_dims, self.fc2_dims, self.fc3_dims, self.n_nets,
            C.cast(nets, C.c_void_p), state.data_ptr(), action.data_ptr(), N.ptr(reward), N.ptr(done), float(gamma),
            N.ptr(coef), N.ptr(lp), N.ptr(li), N.ptr(q1), N.ptr(q2), N.ptr(y), N.stream(self.device)))

    def forward(self, state: torch.Tensor, action: torch.Tensor, out=None):
        """NET:38-49 of every net for every row: state [n, state_dims] or [n, V, state_dims / V], action [n, action_dims] or
        [n, V, action_dims / V], both read in place -> (q1, q2), each [n, 1]; one tensor when n_nets == 1.  `out`: caller-
        owned [n, 1] tensors written in place (a pair; one tensor when n_nets == 1)."""
        n, dev = self._rows(state, action), self.device
        qs = self._q_outs(out, n, "forward: out")
        if qs is None:
            qs = tuple(torch.empty(n, 1, device=dev) for _ in range(self.n_nets))
        if not self._fused(n):
            for t, v in zip(qs, self.q_torch(state.view(n, self.state_dims), action.view(n, self.action_dims))):
                t.copy_(v)
        else:
            self._launch(n, state, action, None, None, 0.0, None, None, None, qs, None)
        return qs if self.n_nets == 2 else qs[0]

    __call__ = forward

    def td_target(self, reward: torch.Tensor, state_: torch.Tensor, action_: torch.Tensor, done: torch.Tensor,
                  gamma: float = 0.99, logp_power: Optional[torch.Tensor] = None, logp_intent: Optional[torch.Tensor] = None,
                  coef: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, q=None) -> torch.Tensor:
        """`global_sac_critic.py:339-352` in the same launch as the forward: y [n] = reward where done, reward + gamma
        (min_c Q_c(state_, action_) - coef[0] logp_power - coef[1] logp_intent) elsewhere (a select, as `target[done] =
        rewards_g[done]` is).  reward [n] float32, done [n] bool or uint8 (0 / 1), logp_power / logp_intent [n] or [n, 1]
        float32 (`next_logp_power_sum`, `next_logp_int_sum`; None: the term is absent), coef a float32 device tensor of 2
        values (`log_alpha.exp() * entropy_scale` twice on the single-alpha path :341-344, `alpha_c`, `alpha_d` on the
        separate-alpha path :346-349; built on the device, no host synchronisation).  Everything is read in place, and
        what would have to be copied is refused.  `out`: a caller-owned [n] tensor for y; `q`: caller-owned [n, 1]
        tensors (a pair; one when n_nets == 1) that receive Q_c(state_, action_)."""
        n, dev = self._rows(state_, action_), self.device
        td_args(reward, done, gamma, n, dev)
        for name, t in (("logp_power", logp_power), ("logp_intent", logp_intent)):
            if t is not None and not (is_f32(t, dev, (n,)) or is_f32(t, dev, (n, 1))):
                raise ValueError("td_target: %s must be a contiguous float32 tensor of shape (%d,) or (%d, 1) on %s"
                                 % (name, n, n, dev))
        if logp_power is not None or logp_intent is not None:
            if coef is None:
                raise ValueError("td_target: logp_power / logp_intent need coef, a float32 tensor of 2 values on %s" % dev)
            if not is_f32(coef, dev) or coef.numel() != 2:
                raise ValueError("td_target: coef must be a contiguous float32 tensor of 2 values on %s" % dev)
        else:
            coef = None
        out = out_f32(out, (n,), "td_target: out", dev)
        qs = self._q_outs(q, n, "td_target: q")
        if not self._fused(n):
            qv = self.q_torch(state_.view(n, self.state_dims), action_.view(n, self.action_dims))
            if qs is not None:
                for t, v in zip(qs, qv):
                    t.copy_(v)
            m = (torch.minimum(qv[0], qv[1]) if self.n_nets == 2 else qv[0]).view(n)
            if logp_power is not None and logp_intent is not None:
                m = m - (coef.view(2)[0] * logp_power.view(n) + coef.view(2)[1] * logp_intent.view(n))
            elif logp_power is not None:
                m = m - coef.view(2)[0] * logp_power.view(n)
            elif logp_intent is not None:
                m = m - coef.view(2)[1] * logp_intent.view(n)
            return td_select(out, reward, done, gamma, m)
        d8 = done.view(torch.uint8) if done.dtype == torch.bool else done
        self._launch(n, state_, action_, reward, d8, gamma, coef, logp_power, logp_intent, qs, out)
        return out

    def q_torch(self, state: torch.Tensor, action: torch.Tensor) -> tuple:
        F = torch.nn.functional
        x = torch.cat([state, action], dim=1)
        out = []
        for net in self.nets:
            h = torch.relu(F.linear(x, net.W1, net.b1))
            h = torch.relu(F.linear(h, net.W2, net.b2))
            h = torch.relu(F.linear(h, net.W3, net.b3))
            out.append(F.linear(h, net.Wq, net.bq))
        return tuple(out)

    def forward_torch(self, state: torch.Tensor, action: torch.Tensor):
        """The same forward with library kernels only (torch.cat, torch.nn.functional.linear, relu): what gemm="library"
        runs.  -> (q1, q2), or one tensor when n_nets == 1."""
        n = state.shape[0]
        qs = self.q_torch(state.reshape(n, self.state_dims), action.reshape(n, self.action_dims))
        return qs if self.n_nets == 2 else qs[0]
