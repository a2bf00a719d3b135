"""Who owns the weights of the hand-written MLP kernels on the host: `WeightSet`, the named float32 tensors of one network
under the reference's `state_dict` keys -- taken by copy or by reference, blended, and watched for changes so that no
kernel reads a stale weight stream -- and the argument checks `actor`, `critic` and `marl_critic` share in front of their
raw-pointer launches.  How a stream is laid out is `_wstream`'s subject, not this module's.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Mapping, Sequence, Tuple

import torch

from . import _native as N


def is_f32(t, device, shape=None) -> bool:
    """A contiguous float32 tensor on `device` (of `shape`, a tuple or torch.Size, where one is given): what a kernel can
    read in place."""
    return (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == device and t.is_contiguous()
            and (shape is None or t.shape == shape))


_NOT_F32 = "%s: %s must be a contiguous float32 tensor of shape %s on %s (%s)"


def choose_mode(name: str, mode, default, modes, fused_ok: bool, shape: str, rule: str, wide_ok: bool = False):
    """The value of a `gemm=` / `pack=` argument (None: `default`), refused unless it is one of `modes` and, for the modes
    that need the fused kernel ("wide": the chunked one, `wide_ok`), the kernel is built for the shape."""
    chosen = mode if mode is not None else default
    if chosen not in modes or (chosen in ("fused", "device") and not fused_ok) or (chosen == "wide" and not wide_ok):
        raise ValueError("%s=%r is not available for %s (modes: %s; %s)" % (name, mode, shape, ", ".join(modes), rule))
    return chosen


PACK_RULE = "device: where the fused kernel is built, see gemm"


def rows_of(t, width: int, name: str, device, n=None) -> int:
    """The row count of a kernel input [n, width] or [n, V, width / V] that is read in place (`n`: the count it must have)."""
    if (not is_f32(t, device) or t.dim() not in (2, 3) or t.shape[0] < 1 or (n is not None and t.shape[0] != n)
            or t.numel() != t.shape[0] * width):
        rows = "n" if n is None else "%d" % n
        raise ValueError("%s must be a contiguous float32 tensor [%s, %d] or [%s, V, %d / V] on %s"
                         % (name, rows, width, rows, width, device))
    return int(t.shape[0])


def out_f32(out, shape, name: str, device) -> torch.Tensor:
    """The caller's output tensor, used as it is or refused, or a new one."""
    return torch.empty(shape, device=device) if out is None else N.in_place(out, torch.float32, shape, name, device)


def stream_pair(stream_shape, n_scales: int, device, new=torch.empty):
    return new(stream_shape, dtype=torch.float16, device=device), new(n_scales, device=device)


def pack_out(out, stream_shape, n_scales: int, what: str, device):
    """(wstream, scales) a device pack writes into: the caller's pair, checked, or new tensors."""
    if out is None:
        return stream_pair(stream_shape, n_scales, device)
    stream, scales = out
    if stream is None or scales is None:
        raise ValueError("%s is a pair (wstream, scales)" % what)
    return (N.in_place(stream, torch.float16, stream_shape, what + "[0]", device),
            N.in_place(scales, torch.float32, (n_scales,), what + "[1]", device))


def pack_workspace(workspace, need: int, what: str, device) -> torch.Tensor:
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    if (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != device
            or not workspace.is_contiguous()):
        raise ValueError("%s: workspace must be a contiguous uint8 tensor on %s" % (what, device))
    return workspace


def td_args(reward, done, gamma, n: int, device) -> None:
    """The checks of `td_target`'s reward [n], done [n] and gamma, all read in place."""
    if reward is None:
        raise ValueError("td_target: reward must be a contiguous float32 tensor of shape (%d,) on %s" % (n, device))
    N.in_place(reward, torch.float32, (n,), "td_target: reward", device)
    done_gamma_args(done, gamma, n, device)


def done_gamma_args(done, gamma, n: int, device) -> None:
    """The checks of `td_target`'s done [n], read in place, and gamma."""
    if (not isinstance(done, torch.Tensor) or done.dtype not in (torch.bool, torch.uint8) or done.device != device
            or not done.is_contiguous() or tuple(done.shape) != (n,)):
        raise ValueError("td_target: done must be a contiguous bool or uint8 tensor of shape (%d,) on %s" % (n, device))
    if not math.isfinite(float(gamma)):
        raise ValueError("td_target: gamma must be finite")


def td_select(out, reward, done, gamma, m) -> torch.Tensor:
    """The library path's epilogue: out = reward where done, reward + gamma m elsewhere."""
    return out.copy_(torch.where(done.view(torch.bool) if done.dtype == torch.uint8 else done, reward, reward + float(gamma) * m))


# ---------------------------------------------------------------------- the Polyak blend of a target network
def polyak_pairs(target, online, what: str):
    """[(online tensor, target tensor)] in the order of `target._WEIGHTS` for `target.soft_update_from(online, tau)`:
    `online` is an object of `target`'s class and shape or a mapping under the reference's key names.  Refuses what
    `share_state_dict` refuses (KeyError for a missing key, ValueError for a tensor that is not contiguous float32 of
    the right shape on the target's device) before anything is touched."""
    names = {a: k for k, a in target._SD.items()}
    if isinstance(online, Mapping):
        _require_keys([(target, online, what)])
        src = {a: online[names[a]] for a in target._WEIGHTS}
    elif isinstance(online, type(target)):
        src = {a: getattr(online, a) for a in target._WEIGHTS}
    else:
        raise ValueError("%s: online must be a %s of the same shape or a mapping of its weights under the reference's key names"
                         % (what, type(target).__name__))
    pairs = []
    for a in target._WEIGHTS:
        t, mine = src[a], getattr(target, a)
        if not is_f32(t, target.device, mine.shape):
            raise ValueError(_NOT_F32 % (what, names[a], tuple(mine.shape), target.device, "it is read in place"))
        if t.data_ptr() == mine.data_ptr():
            raise ValueError("%s: %s is the target's own tensor" % (what, names[a]))
        pairs.append((t, mine))
    return pairs


def polyak_tau(tau, what: str) -> float:
    tau = float(tau)
    if not math.isfinite(tau) or not 0.0 <= tau <= 1.0:
        raise ValueError("%s: tau must be finite and in [0, 1]" % what)
    return tau


SOFT_UPDATE_MAX = 32                                          # tensors per `risvec_soft_update` launch (kSoftUpdateMax)


def soft_update_runs(n: int) -> list:
    """The slices of n pairs that `soft_update_tensors` launches one by one: at most SOFT_UPDATE_MAX pairs each."""
    return [slice(k, min(k + SOFT_UPDATE_MAX, n)) for k in range(0, max(n, 1), SOFT_UPDATE_MAX)]


def soft_update_tensors(pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]], tau: float, device) -> None:
    """target = tau * online + (1 - tau) * target for (online, target) pairs of contiguous float32 device tensors, up to 32
    pairs in ONE launch on the current stream (`risvec_soft_update`, csrc/k_soft_update.hip) and more in runs of 32, in
    place, with the bits of that expression on float32 tensors (`ddpg_torch.py:122-127`).  The targets' version counters
    are not advanced."""
    N.require_hip(device)
    lib, stream = N.load(), N.stream(device)
    for run in soft_update_runs(len(pairs)):
        part = pairs[run]
        n = len(part)
        on = (C.c_void_p * n)(*(o.data_ptr() for o, _ in part))
        tg = (C.c_void_p * n)(*(t.data_ptr() for _, t in part))
        ne = (C.c_int64 * n)(*(t.numel() for _, t in part))
        N.check(lib.risvec_soft_update(n, on, tg, ne, tau, 1.0 - tau, stream))


# ---------------------------------------------------------------------- one network's weights and its weight stream
def _require_keys(sets) -> None:
    for ws, sd, what in sets:
        for k in ws._SD:
            if k not in sd:
                raise KeyError("%s: %r is missing" % (what, k))


def load_weight_sets(sets) -> None:
    """`load_state_dict` of several weight sets as one step: sets = [(WeightSet, mapping, name for messages)].  Everything
    is checked (the keys of every set first) before anything is copied."""
    _require_keys(sets)
    new = []
    for ws, sd, what in sets:
        for k, a in ws._SD.items():
            mine, t = getattr(ws, a), torch.as_tensor(sd[k], dtype=torch.float32)
            if tuple(t.shape) != tuple(mine.shape):
                raise ValueError("%s: %s has shape %s, this %s's is %s" % (what, k, tuple(t.shape), ws._NOUN, tuple(mine.shape)))
            new.append((mine, t, ws.device))
    for mine, t, device in new:
        mine.copy_(t.to(device))


def share_weight_sets(sets) -> None:
    """`share_state_dict` of several weight sets as one step (see `load_weight_sets`): everything is checked before any
    tensor is taken."""
    _require_keys(sets)
    new = []
    for ws, sd, what in sets:
        for k, a in ws._SD.items():
            t, shape = sd[k], getattr(ws, a).shape
            if not is_f32(t, ws.device, shape):
                raise ValueError(_NOT_F32 % (what, k, tuple(shape), ws.device,
                                             "it is used in place; load_state_dict copies and converts"))
            new.append((ws, a, t.detach()))
    for ws, a, t in new:
        setattr(ws, a, t)                                     # the same storage and version counter


class WeightSet:
    """The float32 weight tensors of one network, attributes named by `_WEIGHTS` and keyed by `_SD` as the reference's
    `state_dict()` keys them, and the weight stream of its fused kernel, built from the `_PACKED` ones and cached in
    `_packed` = (key, (wstream, scales)).  The methods need `device`, the weight attributes, `_packed` and `packs` only.
    A subclass that runs `_fused_weights` adds `pack`, `_pack_buffers` = None, `_pack_host`, `_pack_device` and
    `_new_pack_buffers`."""

    _NOUN = "network"                                         # what messages call an object of the class

    def state_dict(self) -> dict:
        """The reference network's `state_dict()` keys, CPU copies."""
        return {k: getattr(self, a).detach().cpu().clone() for k, a in self._SD.items()}

    def load_state_dict(self, sd: Mapping[str, object]) -> None:
        """Take the weights of the reference network's `state_dict()` as it is (tensors or arrays; online and target
        checkpoints alike).  Load checkpoints with `torch.load(..., weights_only=True)`."""
        load_weight_sets([(self, sd, "load_state_dict")])

    def share_state_dict(self, sd: Mapping[str, torch.Tensor]) -> None:
        """Use the learner's own tensors as the weights, by reference (reference key names; typically the learner
        network's `state_dict()`): nothing is copied, now or later.  An in-place update of them is seen through their
        version counters, and the next call rebuilds the weight stream first -- with pack="device" in two launches.
        Tensors must be float32, contiguous, on this object's device and of its shapes."""
        share_weight_sets([(self, sd, "share_state_dict")])

    def soft_update_from(self, online, tau: float) -> None:
        """`update_network_parameters` (`ddpg_torch.py:104-130`) for this (target) network: every weight tensor becomes
        tau * online + (1 - tau) * own, in place, in one launch, bit for bit what that expression gives on float32
        tensors.  online: another object of this class and shape, or a mapping under the reference's key names (the
        learner network's `state_dict()`; contiguous float32 tensors of this object's shapes on its device, read in
        place).  tau in [0, 1]; tau = 1 is the constructor's hard copy (:35).  The write goes through raw pointers, so the
        tensors' version counters are NOT advanced: the weight stream is marked stale here and the next call rebuilds
        it.  A refused argument changes nothing."""
        tau = polyak_tau(tau, "soft_update_from")
        soft_update_tensors(polyak_pairs(self, online, "soft_update_from"), tau, self.device)
        self.mark_stale()

    def mark_stale(self) -> None:
        """Have the next call rebuild the weight stream: for writers that do not advance the weights' version counters."""
        self._packed = (None, self._packed[1])

    def _stale(self):
        """None while the cached weight stream is current, else (key, packed tensors): the stream has to be rebuilt from
        these tensors and is current under this key -- until one of them is replaced or updated in place, or `mark_stale`."""
        ws = tuple(getattr(self, a) for a in self._PACKED)
        key = tuple((t.data_ptr(), t._version) for t in ws)
        return None if self._packed[0] == key else (key, ws)

    def _fused_weights(self):
        """(wstream, scales) of the fused kernel, rebuilt first where stale (pack="host": library kernels into new
        tensors; pack="device": two launches into the buffers of the first rebuild)."""
        stale = self._stale()
        if stale is not None:
            key, ws = stale
            if self.pack == "device":
                if self._pack_buffers is None:
                    self._pack_buffers = self._new_pack_buffers()     # ((wstream, scales), workspace)
                out, workspace = self._pack_buffers
                self._packed = (key, self._pack_device(*ws, out=out, workspace=workspace))
            else:
                self._packed = (key, self._pack_host(*ws))
            self.packs += 1
        return self._packed[1]
