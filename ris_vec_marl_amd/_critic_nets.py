"""What a group of plain ReLU `CriticNetwork` nets (`Simulation-MARL-BCD/networks.py:7-49`) needs on the host, written once
for `BatchedTwinCritic` (one group of n_nets nets) and `BatchedLocalCritics` (one such group per agent): the net itself
and its seeded construction, the rebuild of a group's stale weight streams, the `RisVecMarlCriticNet` table of a launch,
the library path of one net, and the checks of the q buffers and of the entropy term.  The helpers take the device as an
argument and run on CPU tensors too.  How a stream is laid out and packed is `marl_critic`'s subject.
"""
from __future__ import annotations

import math

import torch

from . import _native as N
from ._weights import PACK_RULE, WeightSet, choose_mode, is_f32, stream_pair


class _Net(WeightSet):
    """One `CriticNetwork`'s weights (NET:29-32) and weight stream; the stale streams of a group are rebuilt together."""
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


def draw_net(g: torch.Generator, in_dims: int, fc1_dims: int, fc2_dims: int, fc3_dims: int, device) -> _Net:
    """The next net from the CPU generator `g`: nn.Linear's default ranges (NET:29-32), 1 / sqrt(fan_in), drawn in the
    order W1, b1, W2, b2, W3, b3, Wq, bq."""
    def uni(*shape, r):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * r).to(device)
    net = _Net(device)
    for w, b, fan_out, fan_in in (("W1", "b1", fc1_dims, in_dims), ("W2", "b2", fc2_dims, fc1_dims),
                                  ("W3", "b3", fc3_dims, fc2_dims), ("Wq", "bq", 1, fc3_dims)):
        r = 1.0 / math.sqrt(fan_in)
        setattr(net, w, uni(fan_out, fan_in, r=r))
        setattr(net, b, uni(fan_out, r=r))
    return net


def net_table(count: int, nets, packed):
    """The `RisVecMarlCriticNet` array of a launch: `count` nets and their (wstream, scales), in order (any iterables)."""
    table = (N.RisVecMarlCriticNet * count)()
    for k, (net, (ws, scales)) in enumerate(zip(nets, packed)):
        table[k] = N.RisVecMarlCriticNet(ws.data_ptr(), ws.numel() * ws.element_size(), scales.data_ptr(), net.b1.data_ptr(),
                                         net.b2.data_ptr(), net.b3.data_ptr(), net.Wq.data_ptr(), net.bq.data_ptr())
    return table


def grad_tables(count: int, nets, packed, grads):
    """The `RisVecMarlCriticGradNet` and `RisVecMarlCriticGrads` arrays of a `risvec_marl_critic_grad` launch: `count` nets,
    their (wstream, scales) and their 8 gradient tensors in `_Net._WEIGHTS` order."""
    fwd = net_table(count, nets, packed)
    table, out = (N.RisVecMarlCriticGradNet * count)(), (N.RisVecMarlCriticGrads * count)()
    for k, (net, g) in enumerate(zip(nets, grads)):
        table[k] = N.RisVecMarlCriticGradNet(fwd[k], net.W2.data_ptr(), net.W3.data_ptr())
        out[k] = N.RisVecMarlCriticGrads(*(t.data_ptr() for t in g))
    return table, out


def action_grad_table(count: int, nets, packed):
    """The `RisVecMarlCriticActionGradNet` array of a `risvec_marl_critic_action_grad` launch: `count` nets and their
    (wstream, scales)."""
    fwd = net_table(count, nets, packed)
    table = (N.RisVecMarlCriticActionGradNet * count)()
    for k, net in enumerate(nets):
        table[k] = N.RisVecMarlCriticActionGradNet(fwd[k], net.W1.data_ptr(), net.W2.data_ptr(), net.W3.data_ptr())
    return table


def check_grads(grads, nets, what: str, device) -> list:
    """The caller's gradient tensors, nested like `BatchedAdam`'s groups: per net 8 contiguous float32 tensors shaped like
    the weights in `state_dict()` order, written in place.  -> a list of lists."""
    try:
        nested = [list(g) for g in grads]
    except TypeError:
        raise ValueError("%s: grads is a nested sequence, 8 tensors per net" % what) from None
    if len(nested) != len(nets) or any(len(g) != len(_Net._WEIGHTS) for g in nested):
        raise ValueError("%s: grads holds %d lists of %d tensors" % (what, len(nets), len(_Net._WEIGHTS)))
    names = {a: k for k, a in _Net._SD.items()}
    for c, (net, g) in enumerate(zip(nets, nested)):
        for a, t in zip(_Net._WEIGHTS, g):
            shape = getattr(net, a).shape
            if not is_f32(t, device, shape):
                raise ValueError("%s: the gradient of %s of net %d must be a contiguous float32 tensor of shape %s on %s "
                                 "(it is written in place)" % (what, names[a], c + 1, tuple(shape), device))
    flat = [t.data_ptr() for g in nested for t in g]
    if len(set(flat)) != len(flat):
        raise ValueError("%s: two gradient tensors are the same" % what)
    return nested


def q_net(net: _Net, x: torch.Tensor) -> torch.Tensor:
    """NET:38-49 of one net on the ready input x = [state | action], with library kernels."""
    F = torch.nn.functional
    h = torch.relu(F.linear(x, net.W1, net.b1))
    h = torch.relu(F.linear(h, net.W2, net.b2))
    h = torch.relu(F.linear(h, net.W3, net.b3))
    return F.linear(h, net.Wq, net.bq)


def q_outs(q, n_nets: int, shape: tuple, what: str, device):
    """The caller's q buffers as a tuple of n_nets tensors of `shape` (or None)."""
    if q is None:
        return None
    if isinstance(q, torch.Tensor):
        q = (q,)
    q = tuple(q)
    if len(q) != n_nets or any(t is None for t in q):
        raise ValueError("%s must hold %d tensors of shape %s" % (what, n_nets, shape))
    for t in q:
        N.in_place(t, torch.float32, shape, what, device)
    if n_nets == 2 and q[0].data_ptr() == q[1].data_ptr():
        raise ValueError("%s: the two tensors are the same" % what)
    return q


def entropy_args(logp_power, logp_intent, coef, shapes: tuple, device):
    """The checks of `td_target`'s entropy term: each logp a float32 tensor of one of `shapes`, read in place, and coef 2
    float32 values on the device.  -> coef, None when both logps are absent (the term is)."""
    for name, t in (("logp_power", logp_power), ("logp_intent", logp_intent)):
        if t is not None and not any(is_f32(t, device, s) for s in shapes):
            raise ValueError("td_target: %s must be a contiguous float32 tensor of shape %s on %s"
                             % (name, " or ".join(str(s) for s in shapes), device))
    if logp_power is None and logp_intent is None:
        return None
    if coef is None:
        raise ValueError("td_target: logp_power / logp_intent need coef, a float32 tensor of 2 values on %s" % device)
    if not is_f32(coef, device) or coef.numel() != 2:
        raise ValueError("td_target: coef must be a contiguous float32 tensor of 2 values on %s" % device)
    return coef


def minus_entropy(m: torch.Tensor, coef, lp, li) -> torch.Tensor:
    """The library path's m - (coef[0] lp + coef[1] li), an absent logp an absent term; lp and li arrive in m's shape."""
    if lp is not None and li is not None:
        return m - (coef.view(2)[0] * lp + coef.view(2)[1] * li)
    if lp is not None:
        return m - coef.view(2)[0] * lp
    if li is not None:
        return m - coef.view(2)[1] * li
    return m


class CriticNets:
    """What `BatchedTwinCritic` and `BatchedLocalCritics` share around their nets: the gemm / pack modes and the rebuild of
    stale weight streams.  A subclass sets `device`, `_dims` = (state, action, fc1, fc2, fc3) of one net and `n_nets` (the
    nets of one group), then calls `_init_modes`, and gives `_shape()` for messages and `_all_nets()`."""

    GEMM_MODES = ("fused", "library")
    PACK_MODES = ("host", "device")
    #: with gemm=None, batches of fewer rows than this run the library path even where the fused kernel is built
    #: (the measured crossovers: profiles/marl_critic.json, profiles/local_critics.json; 1 = fused at every row count)
    AUTO_MIN_ROWS = 1
    _SD = _Net._SD

    def _init_modes(self, gemm, fused_ok: bool, rule: str, wide_ok: bool = False) -> None:
        """wide_ok: the chunked kernel (`BatchedTwinCritic`'s gemm="wide") is built for the shape.  It is opt-in: gemm=None
        chooses between "fused" and "library" as before."""
        self.gemm = choose_mode("gemm", gemm, "fused" if fused_ok else "library", self.GEMM_MODES, fused_ok, self._shape(), rule,
                                wide_ok)
        self.fused_min_rows = self.AUTO_MIN_ROWS if gemm is None else 1
        self._gemm_auto = gemm is None                        # the mode was chosen by default: measured row rules apply
        self._fused_ok = fused_ok
        self._wide = self.gemm == "wide"                      # built as gemm="wide": the streams are packed under the wide rule
        self._pack = "host"                                   # see `pack`
        self._pack_workspace = None                           # pack="device": one workspace for every group, at first use
        self.packs = 0                                        # how often a net's weight stream was rebuilt

    @property
    def pack(self) -> str:
        """How the fused kernel's weight streams are rebuilt after a weight update.  "host" (the default):
        `pack_marl_critic_weights` once per stale net, library kernels into new tensors.  "device":
        `pack_marl_critic_weights_device`, two launches for the stale nets of a group together (the twin critic's nets;
        one agent's local nets) into buffers allocated once -- for target critics that are blended every learning step
        (see `soft_update_from`); only where the fused kernel covers the shape, or on a gemm="wide" object.  Setting it marks the streams stale; a
        refused value changes nothing."""
        return self._pack

    @pack.setter
    def pack(self, mode) -> None:
        if choose_mode("pack", mode, None, self.PACK_MODES, self._fused_ok or self._wide, self._shape(), PACK_RULE) != self._pack:
            self._pack = mode
            self.mark_stale()

    def mark_stale(self) -> None:
        """Have the next `forward` / `td_target` rebuild every weight stream: for writers that do not advance the
        weights' version counters."""
        for net in self._all_nets():
            net.mark_stale()

    def _fused(self, n: int) -> bool:
        return self.gemm in ("fused", "wide") and n >= self.fused_min_rows

    def _rebuild_stale(self, nets) -> None:
        """Rebuild the stale weight streams among `nets`, one group: a net's is stale when one of its packed weight tensors
        was replaced or updated in place, or after `mark_stale` (pack="host": library kernels into new tensors, net by
        net; pack="device": the stale nets together in two launches, into the buffers of their first rebuild)."""
        stale = []
        for net in nets:
            s = net._stale()
            if s is not None:
                stale.append((net,) + s)
        if not stale:
            return
        from . import marl_critic as MC                       # it builds on this module: resolved here, off the launch path
        if self._pack == "device":
            dev = self.device
            if self._pack_workspace is None:
                lib = N.load()
                workspace = lib.risvec_marl_critic_wide_pack_workspace if self._wide else lib.risvec_marl_critic_pack_workspace
                need = int(workspace(*self._dims, self.n_nets))
                self._pack_workspace = torch.zeros(need, dtype=torch.uint8, device=dev)
            rows = MC.marl_critic_geom(*self._dims).rows
            for net, _, _ in stale:
                if net._pack_buffers is None:
                    net._pack_buffers = stream_pair((rows, 64, 8), 3, dev, torch.zeros)
            pack = MC.pack_marl_critic_weights_wide_device if self._wide else MC.pack_marl_critic_weights_device
            pack([ws for _, _, ws in stale], out=[net._pack_buffers for net, _, _ in stale], workspace=self._pack_workspace)
            for net, key, _ in stale:
                net._packed = (key, net._pack_buffers)
        else:
            for net, key, ws in stale:
                net._packed = (key, MC.pack_marl_critic_weights(*ws, wide=self._wide))
        self.packs += len(stale)
