"""The multi-agent (SAC) learner's first step on a sampled batch (`Simulation-MARL-BCD/global_sac_critic.py:338-352`): the
two target critics' forward -- each a `CriticNetwork.forward` (`Simulation-MARL-BCD/networks.py:38-49`, NET below), a plain
ReLU MLP on `cat([state, action])` -- the minimum, the entropy term and the TD target, for all rows at once on the GPU.

    x   = [state | action]                                   two tensors, read in place; never concatenated in memory
    h1  = relu(fc1 x);  h2 = relu(fc2 h1);  h3 = relu(fc3 h2);  q_c = q(h3)                       c = 1 .. n_nets
    m   = min(q_1, q_2)                                      (n_nets == 1: q_1)
    ent = coef[0] logp_power + coef[1] logp_intent           an absent logp is an absent term
    y   = done ? reward : reward + gamma (m - ent)

`BatchedTwinCritic.forward` / `td_target` are one launch (`risvec_marl_critic`; gemm="wide": `risvec_marl_critic_wide`,
which covers 16 vehicles); the log-probability sums arrive as
tensors the learner already has.  `soft_update_from` is `update_global_network_parameters` (:394-400) for both nets in
one launch; with pack="device" the next `td_target` rebuilds both weight streams in two launches in all
(`risvec_marl_critic_pack`).  For the ONLINE critics `loss_backward` is the loss of `global_learn` (:355-363) and its
gradient with respect to every weight in two launches (`risvec_marl_critic_grad`), without an autograd graph, and
`action_grad` the critic side of `centralized_actor_update` (:174-176 and the `backward()` at :246): d min(q_1, q_2) / d action
in two launches (`risvec_marl_critic_action_grad`), no weight gradient formed.  The policies' own backward and the local
critics' gradients stay with the learner.  No CPU compute path.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _native as N
from ._critic_nets import (CriticNets, _Net, action_grad_table, check_grads, draw_net, entropy_args, grad_tables, minus_entropy,
                           net_table, q_net, q_outs)
from ._weights import (is_f32, load_weight_sets, out_f32, pack_out, pack_workspace, polyak_pairs, polyak_tau, rows_of,
                       share_weight_sets, soft_update_tensors, td_args, td_select)
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


def _supported_wide(state_dims: int, action_dims: int, fc1_dims: int, fc2_dims: int, fc3_dims: int) -> bool:
    """The rule of `risvec_marl_critic_wide_supported`, restated likewise: up to 512 inputs, the same fc sizes.  It
    overlaps `_supported` on purpose."""
    return (state_dims >= 1 and action_dims >= 1 and state_dims + action_dims <= 512 and fc1_dims >= 32
            and fc1_dims % 32 == 0 and fc1_dims <= 1024 and fc2_dims in (128, 256, 512) and fc3_dims in (128, 256))


def grad_workspace_bytes(n_rows: int, state_dims: int, action_dims: int, fc1_dims: int, fc2_dims: int, fc3_dims: int,
                         n_nets: int) -> int:
    """`risvec_marl_critic_grad_workspace`, restated (the library is the authority: tests compare the two).  float32, with
    npad = n_rows rounded up to 32: the input [S + A rounded up to 32][npad] once; per net the three activations and the
    three deltas feature-major [F][npad], e and q - target [npad], and the tiles' largest deltas [3][npad / 32] rounded
    up to 4 floats.  0: n_rows < 1, n_nets outside {1, 2} or a shape `risvec_marl_critic_grad` is not built for (its rule
    is `risvec_marl_critic`'s)."""
    if n_rows < 1 or n_nets not in (1, 2) or not _supported(state_dims, action_dims, fc1_dims, fc2_dims, fc3_dims):
        return 0
    r32 = lambda v: (v + 31) // 32 * 32                       # noqa: E731
    npad = r32(n_rows)
    per_net = 2 * (fc1_dims + fc2_dims + fc3_dims) * npad + 2 * npad + (3 * (npad // 32) + 3) // 4 * 4
    return 4 * (r32(state_dims + action_dims) * npad + n_nets * per_net)


def pack_marl_critic_weights(W1, W2, W3, wide: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(wstream [rows, 64, 8] float16, scales [3] float32) of one net of `risvec_marl_critic` from its float32 Linear
    weights ([out, in]: fc1 over [state | action], fc2, fc3).  A pure function of its arguments; runs on any device, CPU
    included.  The biases and the q layer are read by the kernel as float32, as they are.  wide=True: the shapes of
    `risvec_marl_critic_wide` (up to 512 inputs) -- the same layout at that shape's number of k-steps, and the same
    bits where both rules hold."""
    if W1.dim() != 2 or W2.dim() != 2 or W3.dim() != 2:
        raise ValueError("pack_marl_critic_weights: W1, W2 and W3 are Linear weights [out, in]")
    (F1, IN), F2, F3 = W1.shape, W2.shape[0], W3.shape[0]
    # the rule depends on the two widths through their sum only
    if IN < 2 or not (_supported_wide if wide else _supported)(IN - 1, 1, F1, F2, F3):
        raise ValueError("no %s twin-critic kernel for state_dims + action_dims=%d fc1=%d fc2=%d fc3=%d"
                         % ("wide" if wide else "fused", IN, F1, F2, F3))
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
    return _pack_device(weights, out, workspace, False, "pack_marl_critic_weights_device")


def pack_marl_critic_weights_wide_device(weights: Sequence, out: Optional[Sequence] = None,
                                         workspace: Optional[torch.Tensor] = None) -> list:
    """`pack_marl_critic_weights_device` for the shapes of `risvec_marl_critic_wide` (up to 512 inputs), through
    `risvec_marl_critic_wide_pack`: the same two kernels, the workspace of `risvec_marl_critic_wide_pack_workspace`, bit
    for bit what `pack_marl_critic_weights(..., wide=True)` gives net by net."""
    return _pack_device(weights, out, workspace, True, "pack_marl_critic_weights_wide_device")


def _pack_device(weights, out, workspace, wide: bool, what: str) -> list:
    lib = N.load()
    pack_workspace_fn = lib.risvec_marl_critic_wide_pack_workspace if wide else lib.risvec_marl_critic_pack_workspace
    pack_fn = lib.risvec_marl_critic_wide_pack if wide else lib.risvec_marl_critic_pack
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
    need = int(pack_workspace_fn(*dims, n_nets)) if IN >= 2 else 0
    if need == 0:
        raise ValueError("no %s twin-critic kernel for state_dims + action_dims=%d fc1=%d fc2=%d fc3=%d"
                         % ("wide" if wide else "fused", IN, F1, F2, F3))
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
    N.check(pack_fn(*dims, n_nets, C.cast(nets, C.c_void_p), workspace.data_ptr(), workspace.numel(), N.stream(dev)))
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


class BatchedTwinCritic(CriticNets):
    """`global_target_critic1` / `global_target_critic2` (`global_sac_critic.py:55-62`; `CriticNetwork`, NET:7-49) for n
    rows at once.  `state_dims` is the flattened state width (n_agents x per-agent width), `action_dims` the flattened
    action width (n_agents x per-agent action); the outputs are q [n, 1] per net.  n_nets=1 is one `CriticNetwork`: the
    local critics of `sac_agent.py:276-284` have the same class and the same target form, one call per agent.  With
    pack="device" both nets' stale weight streams are rebuilt together, in two launches (see `CriticNets.pack`)."""

    GEMM_MODES = ("fused", "library", "wide")

    def __init__(self, state_dims: int, action_dims: int, fc1_dims: int = 1024, fc2_dims: int = 512, fc3_dims: int = 256,
                 n_nets: int = 2, device="cuda", seed: int = 0, gemm: Optional[str] = None):
        """gemm: how `forward` / `td_target` run.  "fused": one hand-written MFMA launch (`risvec_marl_critic`: float16
        hi + lo split products at float32 accuracy, neither the hidden layers nor the concatenated input ever in memory);
        built for state_dims + action_dims <= 128, fc1 % 32 == 0 <= 1024, fc2 in {128, 256, 512}, fc3 in {128, 256}.
        "library": `forward_torch` and the same epilogue with torch.nn.functional only -- the fallback for every other
        shape (16 vehicles: 80 + 288 inputs) and the comparator.  "wide": one launch of `risvec_marl_critic_wide`, the
        fused kernel with fc1 walking the input in chunks of 128; built for state_dims + action_dims <= 512 and the same
        fc sizes, so for 16 vehicles too; opt-in, and `pack = "device"` is available with it.  Default (None): fused
        where built, for batches of at least `AUTO_MIN_ROWS` rows; library otherwise -- never wide."""
        lib = N.load()
        self.device = N.resolve_device(device)
        N.require_hip(self.device)
        self.state_dims, self.action_dims = int(state_dims), int(action_dims)
        self.fc1_dims, self.fc2_dims, self.fc3_dims = int(fc1_dims), int(fc2_dims), int(fc3_dims)
        self.n_nets = int(n_nets)
        self._dims = (self.state_dims, self.action_dims, self.fc1_dims, self.fc2_dims, self.fc3_dims)
        if min(self._dims) < 1:
            raise ValueError("BatchedTwinCritic: every dimension must be >= 1")
        if self.n_nets not in (1, 2):
            raise ValueError("BatchedTwinCritic: n_nets must be 1 or 2")
        self._init_modes(gemm, bool(lib.risvec_marl_critic_supported(*self._dims)),
                         "fused: state_dims + action_dims <= 128 (wide: <= 512), fc1 % 32 == 0 <= 1024, fc2 in {128, 256, 512}, "
                         "fc3 in {128, 256}", bool(lib.risvec_marl_critic_wide_supported(*self._dims)))
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.nets = [draw_net(g, self.state_dims + self.action_dims, *self._dims[2:], self.device) for _ in range(self.n_nets)]

    def _shape(self) -> str:
        return "state_dims=%d action_dims=%d fc1=%d fc2=%d fc3=%d" % self._dims

    def _all_nets(self) -> list:
        return self.nets

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

    def _fused_weights(self) -> list:
        """(wstream, scales) of every net, the stale ones rebuilt first (`CriticNets._rebuild_stale`)."""
        self._rebuild_stale(self.nets)
        return [net._packed[1] for net in self.nets]

    # ------------------------------------------------------------------ forward
    def _rows(self, state, action) -> int:
        n = rows_of(state, self.state_dims, "state", self.device)
        return rows_of(action, self.action_dims, "action", self.device, n)

    def _q_outs(self, q, n: int, what: str):
        """The caller's q buffers as a tuple of n_nets tensors [n, 1] (or None)."""
        return q_outs(q, self.n_nets, (n, 1), what, self.device)

    def _launch(self, n, state, action, reward, done, gamma, coef, lp, li, qs, y) -> None:
        nets = net_table(self.n_nets, self.nets, self._fused_weights())
        q1 = qs[0] if qs is not None else None
        q2 = qs[1] if qs is not None and self.n_nets == 2 else None
        lib = N.load()
        N.check((lib.risvec_marl_critic_wide if self.gemm == "wide" else lib.risvec_marl_critic)(
            n, *self._dims, self.n_nets, C.cast(nets, C.c_void_p), state.data_ptr(), action.data_ptr(), N.ptr(reward), N.ptr(done), float(gamma),
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
        coef = entropy_args(logp_power, logp_intent, coef, ((n,), (n, 1)), dev)
        out = out_f32(out, (n,), "td_target: out", dev)
        qs = self._q_outs(q, n, "td_target: q")
        if not self._fused(n):
            qv = self.q_torch(state_.view(n, self.state_dims), action_.view(n, self.action_dims))
            if qs is not None:
                for t, v in zip(qs, qv):
                    t.copy_(v)
            m = (torch.minimum(qv[0], qv[1]) if self.n_nets == 2 else qv[0]).view(n)
            m = minus_entropy(m, coef, None if logp_power is None else logp_power.view(n),
                              None if logp_intent is None else logp_intent.view(n))
            return td_select(out, reward, done, gamma, m)
        d8 = done.view(torch.uint8) if done.dtype == torch.bool else done
        self._launch(n, state_, action_, reward, d8, gamma, coef, logp_power, logp_intent, qs, out)
        return out

    # ------------------------------------------------------------------ loss and gradients
    #: with gemm=None, `loss_backward` runs the two device launches for row counts in this closed range and the library
    #: path elsewhere; gemm="fused" runs them at every row count.  Measured at 64 / 256 / 4 096 rows, (40, 80) and (20, 24)
    #: inputs (profiles/marl_critic_grad.json): faster than autograd in every round at each -- 6.5x / 6.1x / 2.9x at
    #: (40, 80) with both weight streams rebuilt first.  The device time grows with the rows and nothing beyond 4 096 was
    #: measured, so the default ends there.
    GRAD_AUTO_ROWS = (1, 4096)

    def alloc_grads(self) -> list:
        """Per net, 8 zeroed float32 tensors shaped like the weights, in `state_dict()` order (fc1.weight, fc1.bias, ..,
        q.weight, q.bias): nested like `BatchedAdam`'s groups, so `optimizer.step(grads=grads)` takes them as they are."""
        return [[torch.zeros_like(getattr(net, a)) for a in _Net._WEIGHTS] for net in self.nets]

    def _grad_device(self, n: int) -> bool:
        if self.gemm != "fused":
            return False
        return not getattr(self, "_gemm_auto", False) or self.GRAD_AUTO_ROWS[0] <= n <= self.GRAD_AUTO_ROWS[1]

    def _loss_args(self, state, action, target, grads, q, loss, what: str):
        n, dev = self._rows(state, action), self.device
        if not (is_f32(target, dev, (n,)) or is_f32(target, dev, (n, 1))):
            raise ValueError("%s: target must be a contiguous float32 tensor of shape (%d,) or (%d, 1) on %s (it is read in "
                             "place)" % (what, n, n, dev))
        if target.requires_grad:
            raise ValueError("%s: target is a constant; detach it" % what)
        grads = self.alloc_grads() if grads is None else check_grads(grads, self.nets, what, dev)
        qs = self._q_outs(q, n, what + ": q")
        if qs is None:
            qs = tuple(torch.empty(n, 1, device=dev) for _ in range(self.n_nets))
        return n, grads, qs, out_f32(loss, (1,), what + ": loss", dev)

    def loss_backward(self, state: torch.Tensor, action: torch.Tensor, target: torch.Tensor, grads=None, q=None, loss=None,
                      workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`global_sac_critic.py:355-363` for these (online) critics without an autograd graph: loss = sum_c
        mse_loss(Q_c(state, action), target) and its gradient with respect to every weight, in two launches
        (`risvec_marl_critic_grad`) after the stale weight streams were rebuilt.  -> loss [1] on the device, no
        synchronisation.  `grads` (default: new tensors from `alloc_grads`, kept as `last_grads`) are
        OVERWRITTEN, the state after `zero_grad(set_to_none=True)` and one `backward()`; `q`: caller-owned [n, 1]
        tensors that receive Q_c; `loss`: a caller-owned [1] tensor; `workspace`: a uint8 tensor of at least
        `risvec_marl_critic_grad_workspace` bytes (default: one cached on this object and grown on demand).  target [n] or
        [n, 1] float32 is a constant.  Everything is read in place, and what would have to be copied is refused.
        gemm="library", gemm="wide" and -- with gemm=None -- row counts outside `GRAD_AUTO_ROWS` run
        `loss_backward_torch` into the same buffers."""
        what = "loss_backward"
        n, grads, qs, loss = self._loss_args(state, action, target, grads, q, loss, what)
        if not self._grad_device(n):
            return self._loss_backward_torch(n, state, action, target, grads, qs, loss)
        lib, dev = N.load(), self.device
        need = int(lib.risvec_marl_critic_grad_workspace(n, *self._dims, self.n_nets))
        if workspace is None:
            cached = getattr(self, "_grad_workspace", None)
            if cached is None or cached.numel() < need:
                cached = self._grad_workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            workspace = cached
        else:
            workspace = pack_workspace(workspace, need, what, dev)
        nets, outs = grad_tables(self.n_nets, self.nets, self._fused_weights(), grads)
        N.check(lib.risvec_marl_critic_grad(
            n, *self._dims, self.n_nets, C.cast(nets, C.c_void_p), C.cast(outs, C.c_void_p), state.data_ptr(), action.data_ptr(),
            target.data_ptr(), qs[0].data_ptr(), qs[1].data_ptr() if self.n_nets == 2 else None, loss.data_ptr(),
            workspace.data_ptr(), workspace.numel(), N.stream(dev)))
        self.last_grads = grads
        return loss

    def loss_backward_torch(self, state: torch.Tensor, action: torch.Tensor, target: torch.Tensor, grads=None, q=None,
                            loss=None) -> torch.Tensor:
        """`loss_backward` through autograd and library kernels (torch.cat, linear, relu, mse_loss, backward): the fallback
        and the comparator.  The same arguments, checks and outputs."""
        n, grads, qs, loss = self._loss_args(state, action, target, grads, q, loss, "loss_backward_torch")
        return self._loss_backward_torch(n, state, action, target, grads, qs, loss)

    def _loss_backward_torch(self, n, state, action, target, grads, qs, loss) -> torch.Tensor:
        F = torch.nn.functional
        x = torch.cat([state.view(n, self.state_dims), action.view(n, self.action_dims)], dim=1)
        y = target.view(n)
        leaves, total = [], None
        with torch.enable_grad():
            for net, qo in zip(self.nets, qs):
                w = [getattr(net, a).detach().requires_grad_(True) for a in _Net._WEIGHTS]       # the same storage
                h = torch.relu(F.linear(x, w[0], w[1]))
                h = torch.relu(F.linear(h, w[2], w[3]))
                h = torch.relu(F.linear(h, w[4], w[5]))
                qv = F.linear(h, w[6], w[7])
                qo.copy_(qv.detach())
                term = F.mse_loss(qv.view(n), y)
                total = term if total is None else total + term
                leaves += w
            got = torch.autograd.grad(total, leaves)
        for t, g in zip((t for gs in grads for t in gs), got):
            t.copy_(g)
        loss.copy_(total.detach().view(1))
        self.last_grads = grads
        return loss

    # ------------------------------------------------------------------ d min(q1, q2) / d action
    #: with gemm=None, `action_grad` runs the two device launches for row counts in this closed range and
    #: `action_grad_torch` elsewhere; gemm="fused" runs them at every row count.  The range is the measured row counts (64 /
    #: 256 / 4 096; (40, 80) and (20, 24) inputs; profiles/marl_action_grad.json) at which the device form beat
    #: `action_grad_torch` in every round at both shapes by more than the spread between rounds -- all three, 3.4x to 4.1x
    #: with both weight streams rebuilt first; nothing below 64 or beyond 4 096 rows was measured, so the range ends there.
    #: (): the device path is opt-in.
    ACTION_GRAD_AUTO_ROWS = (64, 4096)

    def _action_grad_device(self, n: int) -> bool:
        if self.gemm != "fused":
            return False
        if not getattr(self, "_gemm_auto", False):
            return True
        rng = self.ACTION_GRAD_AUTO_ROWS
        return len(rng) == 2 and rng[0] <= n <= rng[1]

    def _action_grad_args(self, state, action, out, q_min, q, scale, what: str):
        n, dev = self._rows(state, action), self.device
        if action.requires_grad or state.requires_grad:
            raise ValueError("%s: state and action are read as constants and the result is returned, not recorded; detach it"
                             % what)
        scale = float(scale)
        if not scale == scale or scale in (float("inf"), float("-inf")):
            raise ValueError("%s: scale must be finite" % what)
        out = out_f32(out, (n, self.action_dims), what + ": out", dev)
        if q_min is not None and not (is_f32(q_min, dev, (n,)) or is_f32(q_min, dev, (n, 1))):
            raise ValueError("%s: q_min must be a contiguous float32 tensor of shape (%d,) or (%d, 1) on %s (it is written in "
                             "place)" % (what, n, n, dev))
        return n, out, self._q_outs(q, n, what + ": q"), scale

    def action_grad(self, state: torch.Tensor, action: torch.Tensor, out: Optional[torch.Tensor] = None,
                    q_min: Optional[torch.Tensor] = None, q=None, scale: float = 1.0,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The critic side of `centralized_actor_update` (`global_sac_critic.py:174-176` and the `backward()` at :246) for
        these (online) critics without an autograd graph: out [n, action_dims] = scale * d min(Q_1, Q_2)(state, action) / d
        action, row by row, in two launches (`risvec_marl_critic_action_grad`) after the stale weight streams were rebuilt;
        where Q_1 == Q_2 each net counts half, as `torch.min`'s backward has it; n_nets == 1: scale * dQ / d action.  No
        weight gradient is formed.  No synchronisation.  `out`: a caller-owned [n, action_dims] tensor; `q_min`: a
        caller-owned [n] or [n, 1] tensor that receives min(Q_1, Q_2); `q`: caller-owned [n, 1] tensors (a pair; one when
        n_nets == 1) that receive Q_c, with the bits of `forward`; `workspace`: a uint8 tensor of at least
        `risvec_marl_critic_action_grad_workspace` bytes (default: one cached on this object and grown on demand).
        Everything is read in place, and what would have to be copied is refused; an action that requires grad is refused
        too -- detach it, and hand `out` to `torch.autograd.backward([actions_pi], [out])`.  gemm="library", gemm="wide" and
        -- with gemm=None -- row counts outside `ACTION_GRAD_AUTO_ROWS` run `action_grad_torch` into the same buffers."""
        what = "action_grad"
        n, out, qs, scale = self._action_grad_args(state, action, out, q_min, q, scale, what)
        if not self._action_grad_device(n):
            return self._action_grad_torch(n, state, action, out, q_min, qs, scale)
        lib, dev = N.load(), self.device
        need = int(lib.risvec_marl_critic_action_grad_workspace(n, *self._dims, self.n_nets))
        if workspace is None:
            cached = getattr(self, "_action_grad_workspace", None)
            if cached is None or cached.numel() < need:
                cached = self._action_grad_workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            workspace = cached
        else:
            workspace = pack_workspace(workspace, need, what, dev)
        nets = action_grad_table(self.n_nets, self.nets, self._fused_weights())
        N.check(lib.risvec_marl_critic_action_grad(
            n, *self._dims, self.n_nets, C.cast(nets, C.c_void_p), state.data_ptr(), action.data_ptr(), scale,
            N.ptr(qs[0]) if qs is not None else None, N.ptr(qs[1]) if qs is not None and self.n_nets == 2 else None,
            N.ptr(q_min), out.data_ptr(), workspace.data_ptr(), workspace.numel(), N.stream(dev)))
        return out

    def action_grad_torch(self, state: torch.Tensor, action: torch.Tensor, out: Optional[torch.Tensor] = None,
                          q_min: Optional[torch.Tensor] = None, q=None, scale: float = 1.0) -> torch.Tensor:
        """`action_grad` through autograd and library kernels (torch.cat, linear, relu, torch.min, autograd.grad with respect
        to the action only, the weights detached): the fallback and the comparator.  The same arguments, checks and
        outputs."""
        n, out, qs, scale = self._action_grad_args(state, action, out, q_min, q, scale, "action_grad_torch")
        return self._action_grad_torch(n, state, action, out, q_min, qs, scale)

    def _action_grad_torch(self, n, state, action, out, q_min, qs, scale) -> torch.Tensor:
        F = torch.nn.functional
        with torch.enable_grad():
            a = action.detach().view(n, self.action_dims).requires_grad_(True)
            x = torch.cat([state.detach().view(n, self.state_dims), a], dim=1)
            qv = []
            for net in self.nets:
                w = [getattr(net, k).detach() for k in _Net._WEIGHTS]
                h = torch.relu(F.linear(x, w[0], w[1]))
                h = torch.relu(F.linear(h, w[2], w[3]))
                h = torch.relu(F.linear(h, w[4], w[5]))
                qv.append(F.linear(h, w[6], w[7]))
            m = torch.min(qv[0], qv[1]) if self.n_nets == 2 else qv[0]
            g, = torch.autograd.grad(m.sum(), a)
        if qs is not None:
            for t, v in zip(qs, qv):
                t.copy_(v.detach())
        if q_min is not None:
            q_min.copy_(m.detach().view(q_min.shape))
        torch.mul(g, scale, out=out)
        return out

    def q_torch(self, state: torch.Tensor, action: torch.Tensor) -> tuple:
        x = torch.cat([state, action], dim=1)
        return tuple(q_net(net, x) for net in self.nets)

    def forward_torch(self, state: torch.Tensor, action: torch.Tensor):
        """The same forward with library kernels only (torch.cat, torch.nn.functional.linear, relu): what gemm="library"
        runs.  -> (q1, q2), or one tensor when n_nets == 1."""
        n = state.shape[0]
        qs = self.q_torch(state.reshape(n, self.state_dims), action.reshape(n, self.action_dims))
        return qs if self.n_nets == 2 else qs[0]
