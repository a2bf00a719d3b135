"""The single-agent (DDPG) driver's `agent.choose_action(state)` without the noise (`Simulation-SARL/ddpg_torch.py:37-45`):
`ActorNetwork.forward` (`Simulation-SARL/networks.py:132-141`, NET below) for all rows at once, on the GPU.

    fc1 -> LayerNorm -> ReLU -> fc2 -> LayerNorm -> ReLU -> mu -> sigmoid

One weight set, shared by all rows (unlike `BatchedPolicy`, which stacks one network per agent).  The input is the
rollout launch's observation `[E, V, M//V + 5]` read in place as `[E, V (M//V + 5)]` (`ddpg_train.py:149` flattens it
agent-major), the output is the `mu [E, 2V + M]` tensor bound to `bind_sarl_rollout`: the driver's rollout step is two
launches, actor and everything else.  No CPU compute path.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

from . import _native as N
from ._weights import (PACK_RULE, WeightSet, choose_mode, is_f32, out_f32, pack_out, pack_workspace, rows_of,
                       soft_update_tensors, stream_pair)  # noqa: F401 (soft_update_tensors stays importable from here)
from ._wstream import _split_scaled, centre_fc1

_KS_BUILT = (3, 6, 7, 9)          # fc1 k-steps of 16 the kernel is instantiated for (csrc/k_sarl_actor.hip)


class ActorGeom(NamedTuple):
    """Layout of the weight stream of `risvec_sarl_actor` (include/risvec.h): `items` items of `rows` fragment rows."""
    ks: int
    mt: int
    ht: int
    ng: int
    rows: int
    p1: int
    t1: int
    hs: int
    th: int
    items: int


def actor_geom(input_dims: int, fc1_dims: int, fc2_dims: int, n_actions: int) -> ActorGeom:
    ks = next(k for k in _KS_BUILT if 16 * k >= input_dims + 1)
    mt, ht, ng = fc2_dims // 32, (n_actions + 31) // 32, fc1_dims // 32
    rows = (2 * ks + 1 + 4 * mt + 3) // 4 * 4
    p1, hs = rows // (2 * ks), rows // (2 * ht)
    t1, th = -(-ng // p1), -(-2 * mt // hs)
    return ActorGeom(ks, mt, ht, ng, rows, p1, t1, hs, th, t1 + ng + th)


def _supported(input_dims: int, fc1_dims: int, fc2_dims: int, n_actions: int) -> bool:
    """The rule of `risvec_sarl_actor_supported`, restated for the pure packing function (the library is the authority:
    tests compare the two)."""
    return (1 <= input_dims <= 128 and fc1_dims >= 32 and fc1_dims % 32 == 0 and fc1_dims <= 1024 and fc2_dims in (128, 256)
            and 1 <= n_actions <= 96)


def pack_actor_weights(W1, b1, ln1_w, ln1_b, W2, Wmu) -> Tuple[torch.Tensor, torch.Tensor]:
    """(wstream [items, rows, 64, 8] float16, scales [3] float32) of `risvec_sarl_actor` from the float32 weights
    (Linear weights [out, in]).  A pure function of its arguments; runs on any device, CPU included."""
    F1, IN = W1.shape
    F2, A = W2.shape[0], Wmu.shape[0]
    if not _supported(IN, F1, F2, A):
        raise ValueError("no fused actor kernel for input_dims=%d fc1=%d fc2=%d n_actions=%d" % (IN, F1, F2, A))
    g = actor_geom(IN, F1, F2, A)
    KS, MT, HT, NG = g.ks, g.mt, g.ht, g.ng
    dev = W1.device
    stream = torch.zeros(g.items, g.rows, 64, 8, dtype=torch.float16, device=dev)
    # fc1 operand [F1, 16 KS]: column k < IN the centred weight, column IN the centred bias
    x1 = torch.zeros(F1, 16 * KS, dtype=torch.float64, device=dev)
    x1[:, :IN + 1] = centre_fc1(W1, b1).T
    h1, l1, u1 = _split_scaled(x1)
    # (t, g, r, s, h, j) -> (g, s, t, h, r, j): row = 2 s + t, lane = 32 h + r
    f1 = torch.stack([h1, l1], 0).reshape(2, NG, 32, KS, 2, 8).permute(1, 3, 0, 4, 2, 5).reshape(NG, 2 * KS, 64, 8)
    # fc2 weight as [F1, F2]; hidden feature f = 32 g + 16 u + 8 jh + 4 h + jl:
    # (t, g, u, jh, h, jl, m, r) -> (g, u, t, m, h, r, jh, jl): row = (2 u + t) MT + m
    h2, l2, u2 = _split_scaled(W2.T)
    f2 = torch.stack([h2, l2], 0).reshape(2, NG, 2, 2, 2, 4, MT, 32).permute(1, 2, 0, 6, 4, 7, 3, 5).reshape(NG, 4 * MT, 64, 8)
    # mu weight as [F2, 32 HT], zero padded; f = 32 m + 16 u + 8 jh + 4 h + jl:
    # (t, m, u, jh, h, jl, ht, r) -> (m, u, ht, t, h, r, jh, jl): k-step 2 m + u, row = 2 ht + t
    wp = torch.zeros(F2, 32 * HT, dtype=Wmu.dtype, device=dev)
    wp[:, :A] = Wmu.T
    hh, hl, uh = _split_scaled(wp)
    fh = torch.stack([hh, hl], 0).reshape(2, MT, 2, 2, 2, 4, HT, 32).permute(1, 2, 6, 0, 4, 7, 3, 5).reshape(2 * MT, 2 * HT, 64, 8)
    ln = torch.zeros(NG, 256, dtype=torch.float32, device=dev)        # one fragment row as float32
    ln[:, :32] = ln1_w.float().reshape(NG, 32)
    ln[:, 32:64] = ln1_b.float().reshape(NG, 32)
    s32 = stream.view(torch.float32).view(g.items, g.rows, 256)
    for grp in range(NG):
        it, at = divmod(grp, g.p1)
        stream[it, 2 * KS * at:2 * KS * (at + 1)] = f1[grp]
    p2 = stream[g.t1:g.t1 + NG]
    p2[:, :2 * KS] = f1
    s32[g.t1:g.t1 + NG, 2 * KS] = ln
    p2[:, 2 * KS + 1:2 * KS + 1 + 4 * MT] = f2
    for st in range(2 * MT):
        it, at = divmod(st, g.hs)
        stream[g.t1 + NG + it, 2 * HT * at:2 * HT * (at + 1)] = fh[st]
    return stream, torch.stack([u1, u2, uh]).float().contiguous()


def pack_actor_weights_device(W1, b1, ln1_w, ln1_b, W2, Wmu, out=None, workspace=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`pack_actor_weights` computed on the device by `risvec_sarl_actor_pack` (csrc/k_sarl_actor_pack.hip): two launches
    on the current stream, the float32 weights read in place, no copy and no synchronisation.  out: (wstream, scales)
    to write into, every byte of them (default: new tensors); workspace: a uint8 tensor of
    `risvec_sarl_actor_pack_workspace` bytes (default: a new one).  The same function of its arguments as the host
    one, except that the float64 row means of the centred fc1 weight are summed in another order."""
    lib = N.load()
    ws = (W1, b1, ln1_w, ln1_b, W2, Wmu)
    if not (isinstance(W1, torch.Tensor) and all(is_f32(t, W1.device) for t in ws)):
        raise ValueError("pack_actor_weights_device: the weights must be contiguous float32 tensors on one device")
    dev = W1.device
    N.require_hip(dev)
    if W1.dim() != 2 or W2.dim() != 2 or Wmu.dim() != 2:
        raise ValueError("pack_actor_weights_device: W1, W2 and Wmu are Linear weights [out, in]")
    (F1, IN), F2, A = W1.shape, W2.shape[0], Wmu.shape[0]
    want = dict(b1=(F1,), ln1_w=(F1,), ln1_b=(F1,), W2=(F2, F1), Wmu=(A, F2))
    for name, t in zip(("b1", "ln1_w", "ln1_b", "W2", "Wmu"), ws[1:]):
        if tuple(t.shape) != want[name]:
            raise ValueError("pack_actor_weights_device: %s has shape %s, W1 %s asks for %s" % (name, tuple(t.shape), tuple(W1.shape), want[name]))
    need = int(lib.risvec_sarl_actor_pack_workspace(IN, F1, F2, A))
    if need == 0:
        raise ValueError("no fused actor kernel for input_dims=%d fc1=%d fc2=%d n_actions=%d" % (IN, F1, F2, A))
    g = actor_geom(IN, F1, F2, A)
    stream, scales = pack_out(out, (g.items, g.rows, 64, 8), 3, "pack_actor_weights_device: out", dev)
    workspace = pack_workspace(workspace, need, "pack_actor_weights_device", dev)
    N.check(lib.risvec_sarl_actor_pack(IN, F1, F2, A, *(t.data_ptr() for t in ws), stream.data_ptr(),
                                       stream.numel() * stream.element_size(), scales.data_ptr(), workspace.data_ptr(),
                                       workspace.numel(), N.stream(dev)))
    return stream, scales


def unpack_actor_weights(stream: torch.Tensor, scales: torch.Tensor, input_dims: int, fc1_dims: int, fc2_dims: int,
                         n_actions: int) -> dict:
    """What the kernel multiplies by, as float64: {"fc1" [input_dims + 1, fc1] (centred, the bias last), "fc1_pass1" (the
    same, read from the pass-1 items), "fc2" [fc1, fc2], "mu" [fc2, n_actions], "ln1_w", "ln1_b" [fc1]} -- hi + lo with
    the recorded scale undone.  The inverse of `pack_actor_weights` up to the split's rounding."""
    g = actor_geom(input_dims, fc1_dims, fc2_dims, n_actions)
    KS, MT, HT, NG = g.ks, g.mt, g.ht, g.ng
    s = stream.cpu()
    sc = scales.cpu().double()
    p2 = s[g.t1:g.t1 + NG]

    def fc1_of(frag):                                                 # [NG, 2 KS, 64, 8] -> [IN + 1, F1]
        f = frag.double().reshape(NG, KS, 2, 2, 32, 8)                # (g, s, t, h, r, j)
        x = (f[:, :, 0] + f[:, :, 1]).permute(0, 3, 1, 2, 4).reshape(32 * NG, 16 * KS)    # (g, r, s, h, j)
        return (x * sc[0]).T[:input_dims + 1].contiguous()
    p1 = torch.stack([s[grp // g.p1, 2 * KS * (grp % g.p1):2 * KS * (grp % g.p1 + 1)] for grp in range(NG)])
    f2 = p2[:, 2 * KS + 1:2 * KS + 1 + 4 * MT].double().reshape(NG, 2, 2, MT, 2, 32, 2, 4)     # (g, u, t, m, h, r, jh, jl)
    w2 = (f2[:, :, 0] + f2[:, :, 1]).permute(0, 1, 5, 3, 6, 2, 4).reshape(32 * NG, 32 * MT) * sc[1]   # (g, u, jh, h, jl, m, r)
    fh = torch.stack([s[g.t1 + NG + st // g.hs, 2 * HT * (st % g.hs):2 * HT * (st % g.hs + 1)] for st in range(2 * MT)])
    fh = fh.double().reshape(MT, 2, HT, 2, 2, 32, 2, 4)               # (m, u, ht, t, h, r, jh, jl)
    wm = (fh[:, :, :, 0] + fh[:, :, :, 1]).permute(0, 1, 5, 3, 6, 2, 4).reshape(32 * MT, 32 * HT) * sc[2]  # (m, u, jh, h, jl, ht, r)
    ln = s.view(torch.float32).view(g.items, g.rows, 256)[g.t1:g.t1 + NG, 2 * KS]
    return {"fc1": fc1_of(p2[:, :2 * KS]), "fc1_pass1": fc1_of(p1), "fc2": w2, "mu": wm[:, :n_actions].contiguous(),
            "ln1_w": ln[:, :32].reshape(-1).double(), "ln1_b": ln[:, 32:64].reshape(-1).double()}


class BatchedActor(WeightSet):
    """`ActorNetwork` (NET:95-141) for n rows at once: input_dims -> fc1 -> LayerNorm -> ReLU -> fc2 -> LayerNorm -> ReLU
    -> mu[n_actions] -> sigmoid.  `input_dims` is the flattened width, n_agents x per-agent width (NET:99)."""

    GEMM_MODES = ("fused", "library")
    PACK_MODES = ("host", "device")
    _WEIGHTS = ("W1", "b1", "ln1_w", "ln1_b", "W2", "b2", "ln2_w", "ln2_b", "Wmu", "bmu")
    _SD = {"fc1.weight": "W1", "fc1.bias": "b1", "bn1.weight": "ln1_w", "bn1.bias": "ln1_b", "fc2.weight": "W2",
           "fc2.bias": "b2", "bn2.weight": "ln2_w", "bn2.bias": "ln2_b", "mu.weight": "Wmu", "mu.bias": "bmu"}
    _PACKED = ("W1", "b1", "ln1_w", "ln1_b", "W2", "Wmu")     # what the weight stream is built from
    _NOUN = "actor"
    _pack_host, _pack_device = staticmethod(pack_actor_weights), staticmethod(pack_actor_weights_device)

    def __init__(self, input_dims: int, n_actions: int, fc1_dims: int = 512, fc2_dims: int = 256, device="cuda", seed: int = 0,
                 gemm: Optional[str] = None, pack: Optional[str] = None):
        """gemm: how `forward` runs.  "fused": the whole forward in one hand-written MFMA launch (`risvec_sarl_actor`:
        float16 hi + lo split products at float32 accuracy, the hidden layers never leaving the chip); built for
        input_dims <= 128, fc1 % 32 == 0 <= 1024, fc2 in {128, 256}, n_actions <= 96.  "library": `forward_torch`,
        the same forward with library kernels only -- the fallback for every other shape and the comparator.
        Default: fused where supported.
        pack: how the fused kernel's weight stream is rebuilt after a weight update.  "host": `pack_actor_weights`,
        library kernels into new tensors (the default).  "device": `pack_actor_weights_device`, two launches into
        buffers allocated once -- for a learner that updates the weights every step (see `share_state_dict`); only where
        the fused kernel covers the shape."""
        lib = N.load()
        self.device = N.resolve_device(device)
        N.require_hip(self.device)
        self.input_dims, self.n_actions, self.fc1_dims, self.fc2_dims = int(input_dims), int(n_actions), int(fc1_dims), int(fc2_dims)
        if min(self.input_dims, self.n_actions, self.fc1_dims, self.fc2_dims) < 1:
            raise ValueError("BatchedActor: every dimension must be >= 1")
        dims = (self.input_dims, self.fc1_dims, self.fc2_dims, self.n_actions)
        fused_ok = bool(lib.risvec_sarl_actor_supported(*dims))
        shape = "input_dims=%d fc1=%d fc2=%d n_actions=%d" % dims
        self.gemm = choose_mode("gemm", gemm, "fused" if fused_ok else "library", self.GEMM_MODES, fused_ok, shape,
                                "fused: input_dims <= 128, fc1 % 32 == 0 <= 1024, fc2 in {128, 256}, n_actions <= 96")
        self.pack = choose_mode("pack", pack, "host", self.PACK_MODES, fused_ok, shape, PACK_RULE)
        self._packed = (None, None)                           # (key, (wstream, scales))
        self._pack_buffers = None                             # pack="device": ((wstream, scales), workspace), at first use
        self.packs = 0                                        # how often the weight stream was rebuilt
        dev = self.device
        g = torch.Generator(device="cpu").manual_seed(seed)

        def uni(*shape, r):
            return ((torch.rand(*shape, generator=g) * 2 - 1) * r).to(dev)
        f1, f2, f3 = 1.0 / math.sqrt(self.fc1_dims), 1.0 / math.sqrt(self.fc2_dims), 0.003      # NET:115-125
        self.W1, self.b1 = uni(self.fc1_dims, self.input_dims, r=f1), uni(self.fc1_dims, r=f1)
        self.W2, self.b2 = uni(self.fc2_dims, self.fc1_dims, r=f2), uni(self.fc2_dims, r=f2)
        self.Wmu, self.bmu = uni(self.n_actions, self.fc2_dims, r=f3), uni(self.n_actions, r=f3)
        self.ln1_w, self.ln1_b = torch.ones(self.fc1_dims, device=dev), torch.zeros(self.fc1_dims, device=dev)
        self.ln2_w, self.ln2_b = torch.ones(self.fc2_dims, device=dev), torch.zeros(self.fc2_dims, device=dev)

    def _new_pack_buffers(self):
        dims = (self.input_dims, self.fc1_dims, self.fc2_dims, self.n_actions)
        g = actor_geom(*dims)
        return (stream_pair((g.items, g.rows, 64, 8), 3, self.device, torch.zeros),
                torch.zeros(int(N.load().risvec_sarl_actor_pack_workspace(*dims)), dtype=torch.uint8, device=self.device))

    # ------------------------------------------------------------------ forward
    def forward(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None, logits: Optional[torch.Tensor] = None) -> torch.Tensor:
        """NET:132-141 for every row: obs [n, input_dims] or [n, V, input_dims / V] (the rollout launch's observation, read in
        place) -> mu [n, n_actions] = sigmoid(logits).  `out`: a caller-owned [n, n_actions] tensor written in place
        (the one bound to `bind_sarl_rollout`); `logits`: receives the pre-sigmoid values."""
        n, dev = rows_of(obs, self.input_dims, "obs", self.device), self.device
        out = out_f32(out, (n, self.n_actions), "forward: out", dev)
        N.in_place(logits, torch.float32, (n, self.n_actions), "forward: logits", dev)
        if self.gemm == "library":
            lg = self.logits_torch(obs.view(n, self.input_dims))
            if logits is not None:
                logits.copy_(lg)
            return torch.sigmoid(lg, out=out)
        ws, scales = self._fused_weights()
        N.check(N.load().risvec_sarl_actor(n, self.input_dims, self.fc1_dims, self.fc2_dims, self.n_actions, obs.data_ptr(),
                                           ws.data_ptr(), ws.numel() * ws.element_size(), scales.data_ptr(), self.b2.data_ptr(),
                                           self.ln2_w.data_ptr(), self.ln2_b.data_ptr(), self.bmu.data_ptr(), N.ptr(logits),
                                           out.data_ptr(), N.stream(dev)))
        return out

    __call__ = forward

    def logits_torch(self, x: torch.Tensor) -> torch.Tensor:
        F = torch.nn.functional
        h = torch.relu(F.layer_norm(F.linear(x, self.W1, self.b1), (self.fc1_dims,), self.ln1_w, self.ln1_b, 1e-5))
        h = torch.relu(F.layer_norm(F.linear(h, self.W2, self.b2), (self.fc2_dims,), self.ln2_w, self.ln2_b, 1e-5))
        return F.linear(h, self.Wmu, self.bmu)

    def forward_torch(self, obs: torch.Tensor) -> torch.Tensor:
        """The same forward with library kernels only (torch.nn.functional.linear / layer_norm): what gemm="library" runs."""
        return torch.sigmoid(self.logits_torch(obs.reshape(obs.shape[0], self.input_dims)))
