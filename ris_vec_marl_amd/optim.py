"""The learner's statements between `backward()` and the next TD target, for every network at once:

    torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm)       one scope per network
    optimizer.step()                                                  one `torch.optim.Adam` per network
    target = tau * online + (1 - tau) * target                        the Polyak blend of the network's target

(`Simulation-MARL-BCD/global_sac_critic.py:364-370` and `:246-249`, `sac_agent.py:296-303`; the SARL learner's
`Adam(..., weight_decay=0.01)` without a clip).  `BatchedAdam.step` runs them for any number of networks ("groups") in two
launches (`risvec_adam_step`, csrc/k_adam.hip), one without clipping; `step_torch` is the same computation with library
operators, the comparator, and serves CPU tensors.  Which bits are promised is DESIGN.md's subject: the norm is
reproducible from run to run, the blend has the bits of `soft_update_tensors`, and the Adam statements are float32
statement by statement within a few units in the last place of PyTorch's own kernels, not its bits.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _native as N
from ._weights import polyak_tau

_WHAT = "BatchedAdam"


def _per_group(x, n: int, name: str, check) -> list:
    vals = list(x) if isinstance(x, (list, tuple)) else [x] * n
    if len(vals) != n:
        raise ValueError("%s: %s has %d values, there are %d groups" % (_WHAT, name, len(vals), n))
    return [check(v, name) for v in vals]


def _lr(v, name):
    if isinstance(v, torch.Tensor):
        raise ValueError("%s: a tensor %s is not supported (the step size is formed on the host)" % (_WHAT, name))
    v = float(v)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError("%s: %s=%r must be finite and >= 0" % (_WHAT, name, v))
    return v


def _max_norm(v, name):
    if v is None:
        return None
    v = float(v)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError("%s: %s=%r must be None (no clipping) or finite and >= 0" % (_WHAT, name, v))
    return v


def _expand_target(t):
    """A target entry as a list of tensors / None: a sequence as it is, an object with the `WeightSet` attributes as its
    weight tensors in `_WEIGHTS` order (for the MARL critics the order of the reference module's `parameters()`; a group
    listed in another order passes its targets as tensors)."""
    if hasattr(t, "_WEIGHTS"):
        return [getattr(t, a) for a in t._WEIGHTS], [t]
    return list(t), []


class BatchedAdam:
    """`clip_grad_norm_` + `torch.optim.Adam` + the target blend for a list of networks.

    groups: a sequence of parameter lists, one per network (typically `module.parameters()`): contiguous float32 tensors
    on one device, read and written in place; a tensor may appear once.  lr, weight_decay (coupled L2, as `Adam` has it)
    and max_norm (None: no clipping) are one value or one per group; betas and eps are shared.  The moments are allocated
    once, zeroed, each at its parameter's offset from a 16-byte boundary.  write_clipped_grads=True writes grad * coef
    back as `clip_grad_norm_` does in place (off by default: the learner drops its gradients before the next
    `backward()`).  No default anywhere uses this class: the learner opts in."""

    def __init__(self, groups, lr=1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay=0.0, max_norm=1.0, device=None,
                 write_clipped_grads: bool = False):
        try:
            groups = [list(g) for g in groups]
        except TypeError:
            raise ValueError("%s: groups is a sequence of parameter lists" % _WHAT) from None
        if not groups or any(not g for g in groups):
            raise ValueError("%s: groups is a non-empty sequence of non-empty parameter lists" % _WHAT)
        first = groups[0][0]
        if not isinstance(first, torch.Tensor):
            raise ValueError("%s: parameters must be tensors" % _WHAT)
        self.device = first.device if device is None else N.resolve_device(device)
        seen = set()
        for gi, g in enumerate(groups):
            for k, p in enumerate(g):
                name = "groups[%d][%d]" % (gi, k)
                if not isinstance(p, torch.Tensor) or p.dtype != torch.float32:
                    raise ValueError("%s: %s must be a float32 tensor" % (_WHAT, name))
                if not p.is_contiguous():
                    raise ValueError("%s: %s is not contiguous (parameters are written in place)" % (_WHAT, name))
                if p.device != self.device:
                    raise ValueError("%s: %s is on %s, not on %s" % (_WHAT, name, p.device, self.device))
                if p.numel() < 1:
                    raise ValueError("%s: %s is empty" % (_WHAT, name))
                if id(p) in seen or p.data_ptr() in seen:
                    raise ValueError("%s: %s appears twice (a parameter belongs to one group)" % (_WHAT, name))
                seen.update((id(p), p.data_ptr()))
        n = len(groups)
        self.lr = _per_group(lr, n, "lr", _lr)
        self.weight_decay = _per_group(weight_decay, n, "weight_decay", _lr)
        self.max_norm = _per_group(max_norm, n, "max_norm", _max_norm)
        try:
            b1, b2 = (float(b) for b in betas)
        except (TypeError, ValueError):
            raise ValueError("%s: betas is a pair of floats" % _WHAT) from None
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError("%s: betas=%r must lie in [0, 1)" % (_WHAT, (b1, b2)))
        eps = float(eps)
        if not math.isfinite(eps) or eps < 0.0:
            raise ValueError("%s: eps=%r must be finite and >= 0" % (_WHAT, eps))
        self.betas, self.eps = (b1, b2), eps
        self.write_clipped_grads = bool(write_clipped_grads)
        self.groups = groups
        self.t = 0                                            # optimiser steps taken
        self.table_uploads = 0                                # how often the descriptor table went to the device
        self._params = [p for g in groups for p in g]
        self._group_of = [gi for gi, g in enumerate(groups) for _ in g]
        # the moments: two flat buffers, every slice at its parameter's offset from a 16-byte boundary
        offs, total = [], 0
        for p in self._params:
            start = (total + 3) // 4 * 4 + ((p.data_ptr() >> 2) & 3)
            offs.append(start)
            total = start + p.numel()
        self._moments = torch.zeros(2, (total + 3) // 4 * 4, dtype=torch.float32, device=self.device)
        self.exp_avg = [self._moments[0, o:o + p.numel()].view(p.shape) for o, p in zip(offs, self._params)]
        self.exp_avg_sq = [self._moments[1, o:o + p.numel()].view(p.shape) for o, p in zip(offs, self._params)]
        # the workgroup layout follows from the element counts alone
        blocks = [(p.numel() + N.ADAM_CHUNK - 1) // N.ADAM_CHUNK for p in self._params]
        self._first_block = [0] * len(blocks)
        for i in range(1, len(blocks)):
            self._first_block[i] = self._first_block[i - 1] + blocks[i - 1]
        self.n_blocks = self._first_block[-1] + blocks[-1]
        self._blocks = blocks
        self._key = None                                      # the pointers the device table was built from
        self._dev = None                                      # device buffers, at the first step()
        self._clip = any(m is not None for m in self.max_norm)

    # ------------------------------------------------------------------ construction from / to torch.optim.Adam
    @classmethod
    def from_torch(cls, optimizers, max_norm=1.0, write_clipped_grads: bool = False) -> "BatchedAdam":
        """One group per `torch.optim.Adam` in `optimizers`, with its hyper-parameters and any state it already has (step
        count and moments, copied).  Refused: another optimiser class, amsgrad, maximize, decoupled weight decay (AdamW),
        a tensor lr, differentiable, param groups of one optimiser with different hyper-parameters, betas or eps that
        differ between optimisers, and step counts that differ anywhere (one count is kept for all)."""
        what = "BatchedAdam.from_torch"
        optimizers = list(optimizers)
        if not optimizers:
            raise ValueError("%s: no optimizers" % what)
        groups, lrs, wds, shared, steps = [], [], [], None, set()
        for oi, opt in enumerate(optimizers):
            if not isinstance(opt, torch.optim.Adam):
                raise ValueError("%s: optimizers[%d] is a %s, not a torch.optim.Adam" % (what, oi, type(opt).__name__))
            hyper, params = None, []
            for pg in opt.param_groups:
                for flag in ("amsgrad", "maximize", "differentiable"):
                    if pg.get(flag, False):
                        raise ValueError("%s: optimizers[%d] has %s=True" % (what, oi, flag))
                if pg.get("decoupled_weight_decay", False) or isinstance(opt, torch.optim.AdamW):
                    raise ValueError("%s: optimizers[%d] uses decoupled weight decay (AdamW)" % (what, oi))
                if isinstance(pg["lr"], torch.Tensor):
                    raise ValueError("%s: optimizers[%d] has a tensor lr" % (what, oi))
                if any(isinstance(b, torch.Tensor) for b in pg["betas"]):
                    raise ValueError("%s: optimizers[%d] has tensor betas" % (what, oi))
                h = (float(pg["lr"]), float(pg["weight_decay"]), tuple(float(b) for b in pg["betas"]), float(pg["eps"]))
                if hyper is not None and h != hyper:
                    raise ValueError("%s: optimizers[%d] has param groups with different hyper-parameters" % (what, oi))
                hyper = h
                params += list(pg["params"])
            if shared is not None and hyper[2:] != shared:
                raise ValueError("%s: optimizers[%d] has betas / eps %r, optimizers[0] has %r" % (what, oi, hyper[2:], shared))
            shared = hyper[2:]
            for p in params:
                st = opt.state.get(p, {})
                steps.add(int(st["step"]) if "step" in st else 0)
            groups.append(params)
            lrs.append(hyper[0])
            wds.append(hyper[1])
        if len(steps) != 1:
            raise ValueError("%s: step counts differ (%s); one count is kept for all parameters" % (what, sorted(steps)))
        self = cls(groups, lr=lrs, betas=shared[0], eps=shared[1], weight_decay=wds, max_norm=max_norm,
                   write_clipped_grads=write_clipped_grads)
        self.t = steps.pop()
        if self.t:
            i = 0
            for opt, g in zip(optimizers, groups):
                for p in g:
                    st = opt.state[p]
                    self.exp_avg[i].copy_(st["exp_avg"])
                    self.exp_avg_sq[i].copy_(st["exp_avg_sq"])
                    i += 1
        return self

    def to_torch(self, optimizers) -> None:
        """Write the step count and the moments (copies) into `torch.optim.Adam` objects over the same parameters, one
        per group: the reverse of `from_torch`."""
        optimizers = list(optimizers)
        if len(optimizers) != len(self.groups):
            raise ValueError("BatchedAdam.to_torch: %d optimizers for %d groups" % (len(optimizers), len(self.groups)))
        for gi, (opt, g) in enumerate(zip(optimizers, self.groups)):
            theirs = [p for pg in opt.param_groups for p in pg["params"]]
            if len(theirs) != len(g) or any(a is not b for a, b in zip(theirs, g)):
                raise ValueError("BatchedAdam.to_torch: optimizers[%d] is not over the parameters of group %d" % (gi, gi))
        i = 0
        for opt, g in zip(optimizers, self.groups):
            for p in g:
                opt.state[p] = {"step": torch.tensor(float(self.t)), "exp_avg": self.exp_avg[i].detach().clone(),
                                "exp_avg_sq": self.exp_avg_sq[i].detach().clone()}
                i += 1

    def state_dict(self) -> dict:
        """Step count, moments (CPU copies, nested like `groups`) and hyper-parameters."""
        def nest(flat):
            it = iter(flat)
            return [[next(it).detach().cpu().clone() for _ in g] for g in self.groups]
        return {"step": self.t, "exp_avg": nest(self.exp_avg), "exp_avg_sq": nest(self.exp_avg_sq), "lr": list(self.lr),
                "betas": self.betas, "eps": self.eps, "weight_decay": list(self.weight_decay), "max_norm": list(self.max_norm)}

    def load_state_dict(self, sd) -> None:
        """Take what `state_dict` gave; everything is checked before anything is copied."""
        what, n = "BatchedAdam.load_state_dict", len(self.groups)
        t = int(sd["step"])
        if t < 0:
            raise ValueError("%s: step=%d" % (what, t))
        new = []
        for key, mine in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            flat = [x for g in sd[key] for x in g]
            if [len(g) for g in sd[key]] != [len(g) for g in self.groups]:
                raise ValueError("%s: %s does not match the groups" % (what, key))
            for a, b in zip(mine, flat):
                b = torch.as_tensor(b, dtype=torch.float32)
                if tuple(b.shape) != tuple(a.shape):
                    raise ValueError("%s: %s has a tensor of shape %s, the parameter's is %s" % (what, key, tuple(b.shape), tuple(a.shape)))
                new.append((a, b))
        lr = _per_group(sd.get("lr", self.lr), n, "lr", _lr)
        wd = _per_group(sd.get("weight_decay", self.weight_decay), n, "weight_decay", _lr)
        mn = _per_group(sd.get("max_norm", self.max_norm), n, "max_norm", _max_norm)
        b1, b2 = (float(b) for b in sd.get("betas", self.betas))
        eps = float(sd.get("eps", self.eps))
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or not math.isfinite(eps) or eps < 0.0:
            raise ValueError("%s: betas=%r eps=%r" % (what, (b1, b2), eps))
        for a, b in new:
            a.copy_(b)
        self.t, self.lr, self.weight_decay, self.max_norm, self.betas, self.eps = t, lr, wd, mn, (b1, b2), eps
        self._clip = any(m is not None for m in mn)
        self._key = None                                      # the group table carries lr, weight_decay and max_norm

    # ------------------------------------------------------------------ arguments of a step
    def _grads(self, grads) -> list:
        if grads is None:
            flat = [p.grad for p in self._params]
        else:
            try:
                nested = [list(g) for g in grads]
            except TypeError:
                raise ValueError("%s: grads is a nested sequence like groups" % _WHAT) from None
            if [len(g) for g in nested] != [len(g) for g in self.groups]:
                raise ValueError("%s: grads does not match the groups" % _WHAT)
            flat = [x for g in nested for x in g]
        for i, g in enumerate(flat):
            if g is None:
                raise ValueError("%s: parameter %d (group %d) has no gradient (all parameters step together: one step count)"
                                 % (_WHAT, i, self._group_of[i]))
        return flat

    def _check_grads(self, flat) -> None:
        for i, (g, p) in enumerate(zip(flat, self._params)):
            if (not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.device != self.device or not g.is_contiguous()
                    or g.shape != p.shape):
                raise ValueError("%s: the gradient of parameter %d must be a contiguous float32 tensor of shape %s on %s"
                                 % (_WHAT, i, tuple(p.shape), self.device))

    def _targets(self, targets, tau):
        """-> (flat list of target tensors / None, owners to mark stale, tau)"""
        if targets is None:
            if tau is not None:
                raise ValueError("%s: tau is given without targets" % _WHAT)
            return None, [], None
        if tau is None:
            raise ValueError("%s: targets need tau" % _WHAT)
        tau = polyak_tau(tau, _WHAT + ".step")
        owners = []
        if hasattr(targets, "nets") and not isinstance(targets, (list, tuple)):
            owners.append(targets)
            nets = []
            for x in targets.nets:                            # BatchedTwinCritic: nets; BatchedLocalCritics: pairs of nets
                nets += list(x) if isinstance(x, (list, tuple)) else [x]
            targets = nets
        try:
            targets = list(targets)
        except TypeError:
            raise ValueError("%s: targets is a nested sequence like groups" % _WHAT) from None
        if len(targets) != len(self.groups):
            raise ValueError("%s: %d target groups for %d groups" % (_WHAT, len(targets), len(self.groups)))
        flat = []
        for gi, (tg, g) in enumerate(zip(targets, self.groups)):
            if tg is None:
                flat += [None] * len(g)
                continue
            ts, own = _expand_target(tg)
            owners += own
            if len(ts) != len(g):
                raise ValueError("%s: targets[%d] has %d tensors, group %d has %d" % (_WHAT, gi, len(ts), gi, len(g)))
            flat += ts
        return flat, owners, tau

    def _check_targets(self, flat) -> None:
        ptrs = {p.data_ptr() for p in self._params}
        for i, (t, p) in enumerate(zip(flat, self._params)):
            if t is None:
                continue
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous()
                    or t.shape != p.shape):
                raise ValueError("%s: the target of parameter %d must be a contiguous float32 tensor of shape %s on %s"
                                 % (_WHAT, i, tuple(p.shape), self.device))
            if t.data_ptr() in ptrs:
                raise ValueError("%s: the target of parameter %d is a parameter (a parameter cannot be its own target)" % (_WHAT, i))

    # ------------------------------------------------------------------ the device step
    def _changed(self, grads, targets):
        """None while every pointer is the one the device table holds, else the new key."""
        def ptr(t):
            return t.data_ptr() if isinstance(t, torch.Tensor) else 0
        key = (tuple(p.data_ptr() for p in self._params), tuple(ptr(g) for g in grads),
               None if targets is None else tuple(ptr(t) for t in targets))
        return None if key == self._key else key

    def _upload(self, grads, targets) -> None:
        """Build the descriptor table from the current pointers and send it to the device: a stream-ordered copy from a
        pinned tensor made for this upload alone (an earlier upload may still be in flight from its own)."""
        n, ng = len(self._params), len(self.groups)
        tens = (N.RisVecAdamTensor * n)()
        for i, p in enumerate(self._params):
            t = targets[i] if targets is not None else None
            tens[i] = N.RisVecAdamTensor(p.data_ptr(), grads[i].data_ptr(), self.exp_avg[i].data_ptr(), self.exp_avg_sq[i].data_ptr(),
                                         t.data_ptr() if t is not None else None, p.numel(), self._group_of[i],
                                         self._first_block[i], 0)
        grp = (N.RisVecAdamGroup * ng)()
        i = 0
        for gi, g in enumerate(self.groups):
            nb = sum(self._blocks[i:i + len(g)])
            mn = self.max_norm[gi]
            grp[gi] = N.RisVecAdamGroup(self.lr[gi], self.weight_decay[gi], -1.0 if mn is None else mn, self._first_block[i], nb, 0)
            i += len(g)
        if self._dev is None:
            bmap = torch.repeat_interleave(torch.arange(n, dtype=torch.int32), torch.tensor(self._blocks)).to(torch.int32)
            nbytes = 64 * n + 32 * ng + 4 * self.n_blocks
            self._dev = {"blob": torch.empty(nbytes, dtype=torch.uint8, device=self.device), "map": bmap,
                         "partials": torch.empty(self.n_blocks, dtype=torch.float64, device=self.device),
                         "norms": torch.zeros(ng, dtype=torch.float32, device=self.device)}
        pinned = torch.empty(self._dev["blob"].numel(), dtype=torch.uint8, pin_memory=True)
        pinned[:64 * n] = torch.frombuffer(tens, dtype=torch.uint8)
        pinned[64 * n:64 * n + 32 * ng] = torch.frombuffer(grp, dtype=torch.uint8)
        pinned[64 * n + 32 * ng:] = self._dev["map"].view(torch.uint8)
        self._dev["blob"].copy_(pinned, non_blocking=True)
        self._host = (tens, grp)                              # what risvec_adam_step checks
        self.table_uploads += 1

    def step(self, targets=None, tau: Optional[float] = None, grads=None):
        """One optimiser step of every group on the current stream: `k_adam_sqsum` + `k_adam_step`, or `k_adam_step`
        alone where no group clips.  -> norms, an [n_groups] float32 device tensor with the `total_norm` that
        `clip_grad_norm_` returns per group (overwritten by the next step), or None without clipping.

        Gradients are the parameters' `.grad`, or `grads` (nested like `groups`).  A parameter without a gradient raises
        ValueError and nothing is changed: PyTorch skips such a parameter and keeps a step count per parameter; here every
        parameter shares one count, and the reference's critics and policies always have all their gradients.

        targets: nested like `groups`, tensors to blend (`target = tau * param + (1 - tau) * target` with the new
        parameter, the bits of `soft_update_tensors`) or None per tensor or per group; a group's entry may be an object
        with the `WeightSet` attributes, and the whole argument a `BatchedTwinCritic` / `BatchedLocalCritics`; those are
        `mark_stale()`d.  The descriptor table is sent to the device again only when a pointer changed
        (`zero_grad(set_to_none=True)` moves `.grad`); `table_uploads` counts it.  Afterwards the version counters of the
        parameters and the blended targets are advanced, so autograd's saved-tensor checks and a critic object that
        shares the tensors (`share_state_dict`) see the update.  Nothing synchronises, and nothing is allocated after the
        first call while the pointers stay."""
        flat_g = self._grads(grads)
        flat_t, owners, tau = self._targets(targets, tau)
        changed = self._changed(flat_g, flat_t)
        if changed is not None:
            self._check_grads(flat_g)
            if flat_t is not None:
                self._check_targets(flat_t)
        N.require_hip(self.device)
        if changed is not None:
            self._upload(flat_g, flat_t)
            self._key = changed
        n, ng = len(self._params), len(self.groups)
        blend = flat_t is not None and any(t is not None for t in flat_t)
        flags = ((N.ADAM_CLIP if self._clip else 0) | (N.ADAM_WRITE_GRAD if self.write_clipped_grads else 0)
                 | (N.ADAM_BLEND if blend else 0))
        d = self._dev
        base = d["blob"].data_ptr()
        tens, grp = self._host
        N.check(N.load().risvec_adam_step(
            n, ng, self.n_blocks, base, base + 64 * n, base + 64 * n + 32 * ng, C.cast(tens, C.c_void_p), C.cast(grp, C.c_void_p),
            self.betas[0], self.betas[1], self.eps, self.t + 1, tau if blend else 0.0, 1.0 - tau if blend else 1.0, flags,
            d["partials"].data_ptr(), 8 * self.n_blocks, d["norms"].data_ptr(), N.stream(self.device)))
        self.t += 1
        touched = list(self._params)
        if blend:
            touched += [t for t in flat_t if t is not None]
        if self.write_clipped_grads and self._clip:
            touched += flat_g
        torch.autograd.graph.increment_version(touched)
        for o in owners:
            o.mark_stale()
        return d["norms"] if self._clip else None

    # ------------------------------------------------------------------ the same with library operators
    @torch.no_grad()
    def step_torch(self, targets=None, tau: Optional[float] = None, grads=None):
        """`step` with library operators, on any device: per group the statements of `clip_grad_norm_`
        (`get_total_norm`, `max_norm / (total_norm + 1e-6)`, `clamp(max=1)`, the product), then `torch.optim.Adam`'s
        single-tensor float32 statements one by one, then the reference's blend loop.  Same arguments, same result type;
        the gradients are left alone unless `write_clipped_grads`."""
        flat_g = self._grads(grads)
        self._check_grads(flat_g)
        flat_t, owners, tau = self._targets(targets, tau)
        if flat_t is not None:
            self._check_targets(flat_t)
        b1, b2 = self.betas
        step = self.t + 1
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        bc2_sqrt = bc2 ** 0.5
        norms, i = [], 0
        for gi, g in enumerate(self.groups):
            sl = slice(i, i + len(g))
            gs = flat_g[sl] if self.write_clipped_grads else [x.clone() for x in flat_g[sl]]
            total = torch.nn.utils.get_total_norm(gs, 2.0, False, False)
            norms.append(total)
            if self.max_norm[gi] is not None:
                coef = torch.clamp(self.max_norm[gi] / (total + 1e-6), max=1.0)
                for x in gs:
                    x.mul_(coef)
            step_size = self.lr[gi] / bc1
            for p, x, m, v in zip(g, gs, self.exp_avg[sl], self.exp_avg_sq[sl]):
                if self.weight_decay[gi] != 0:
                    x = x.add(p, alpha=self.weight_decay[gi])
                m.lerp_(x, 1 - b1)
                v.mul_(b2).addcmul_(x, x, value=1 - b2)
                denom = (v.sqrt() / bc2_sqrt).add_(self.eps)
                p.addcdiv_(m, denom, value=-step_size)
            i += len(g)
        if flat_t is not None:
            for p, t in zip(self._params, flat_t):
                if t is not None:
                    t.copy_(tau * p + (1 - tau) * t)
        self.t = step
        for o in owners:
            o.mark_stale()
        return torch.stack(norms).to(torch.float32) if self._clip else None


__all__ = ["BatchedAdam"]
