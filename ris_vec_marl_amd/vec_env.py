"""`VecEnviron`: E independent RIS-VEC environments resident on one MI355X.

Host-side mirror of the reference's `Environ` class (Environment.py:56) for the hot
path only: same method names, same argument meaning, batched over a leading env
axis and returning torch tensors that live on the GPU.  All arithmetic happens in
the HIP kernels of `csrc/` behind the C ABI of `include/risvec.h`; torch is used
for device memory and streams.  There is no CPU fallback: without a HIP device (or
without the built extension) every compute call raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from ._currency import Currency
from .params import CHANNEL_MODELS, EnvParams

# module constants of the reference (Environment.py:29-42)
RIS_x, RIS_y, RIS_z = 220, 220, 25
BS_x, BS_y, BS_z = 0, 0, 25
ro = 10 ** -2
lamb = 1
d = 0.5
sigma = 10 ** (-7)
alpha1 = 2.2
alpha2 = 2.5


class ParamAttrs:
    """Gives an env object the reference's flat attribute surface: `env.w_d = 1.0`,
    `env.noise_power` ... are forwarded to `self.params` (an `EnvParams`)."""

    def __getattr__(self, name):
        # only called when normal lookup fails
        params = self.__dict__.get("params")
        if params is not None and name in EnvParams._FIELDS:
            return getattr(params, name)
        raise AttributeError("%s object has no attribute %r" % (type(self).__name__, name))

    def __setattr__(self, name, value):
        params = self.__dict__.get("params")
        if params is not None and name in EnvParams._FIELDS:
            setattr(params, name, value)
        else:
            object.__setattr__(self, name, value)


class VecEnviron(ParamAttrs, Currency):
    """Batched environment.  Constructor mirrors Environment.py:57 plus batching args."""

    def __init__(self, down_lane, up_lane, left_lane, right_lane, width, height, n_veh, M, control_bit,
                 n_envs: int = 1, device: str = "cuda", seed: int = 0, env_offset: int = 0,
                 params: Optional[EnvParams] = None, lazy_theta: bool = False):
        object.__setattr__(self, "params", params if params is not None else EnvParams())
        self.down_lanes = list(down_lane)
        self.up_lanes = list(up_lane)
        self.left_lanes = list(left_lane)
        self.right_lanes = list(right_lane)
        self.width = width
        self.height = height
        self.n_veh = int(n_veh)
        self.M = int(M)
        self.control_bit = int(control_bit)
        self.n_envs = int(n_envs)
        self.env_offset = int(env_offset)
        self.seed = int(seed)
        self.device = N.resolve_device(device)
        if not 1 <= self.n_veh <= N.MAX_VEH:
            raise ValueError("n_veh must be in [1, %d]" % N.MAX_VEH)
        if self.n_envs < 1 or self.M < 1:
            raise ValueError("n_envs and M must be >= 1")
        if not 0 <= self.control_bit <= 6:
            raise ValueError("control_bit must be in [0, 6]")
        # Environment.py:169, 175-179
        self.possible_angles = np.linspace(0, 2 * np.pi, 2 ** self.control_bit, endpoint=False)
        self.distance_B_R = float(np.sqrt((BS_x - RIS_x) ** 2 + (BS_y - RIS_y) ** 2 + (BS_z - RIS_z) ** 2))
        self.angle_B_R = (RIS_x - BS_x) / self.distance_B_R
        m = np.arange(self.M, dtype=np.float64)
        ph = 2 * (np.pi / lamb) * d * self.angle_B_R * m
        self.phase_R = np.cos(ph) + 1j * np.sin(ph)
        self._epoch = 0          # reset counter   (RNG counter for spawn draws)
        self._moves = 0          # renew_positions counter
        self._steps = 0          # step counter    (RNG counter for arrivals)
        self._chan = 0           # 3GPP-gain / random-phase counter
        self._obs_stale = True   # obs[E,V,5] does not reflect the state tensors (no step since the last reset)
        self._sarl_obs_mark = None   # (_epoch, _steps) at which the SARL observation tensor was current (bind_sarl_rollout)
        self._t: Dict[str, torch.Tensor] = {}
        # lazy_theta: between BCD sweeps keep theta BY INDEX (one byte per element, theta_idx): `step(bcd=True)` then
        # neither writes nor reads the complex64 tensor (67 MB out + 67 MB in per step at BASELINE configs[4]); it is
        # materialised when somebody asks for it (`tensors`, any other consumer).  Same step outputs bit for bit.
        self.lazy_theta = bool(lazy_theta)
        # what theta, its indices, h_r and the caches derived from them are known to hold: every "this is current" bit a
        # launch carries is decided by the Currency base (_currency.py), which owns the fields behind them
        self._init_currency()
        self._cstate: Optional[N.RisVecState] = None
        self._cparams: Optional[N.RisVecParams] = None
        self._cparams_version = -1

    # ------------------------------------------------------------------ device state
    def _lanes(self):
        return dict(up_lanes=self.up_lanes, down_lanes=self.down_lanes, left_lanes=self.left_lanes,
                    right_lanes=self.right_lanes)

    def _ensure_device(self) -> None:
        if self._cstate is not None:
            return
        lib = N.load()       # raises if the extension is not built
        del lib
        self.device = N.resolve_device(self.device)      # a bare "cuda" becomes cuda:<current>
        N.require_hip(self.device)
        E, V, M = self.n_envs, self.n_veh, self.M
        dev = self.device
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=dev)   # noqa: E731
        t = self._t
        t["pos"] = z(E, V, 2, dt=torch.float64)
        t["dir"] = z(E, V, dt=torch.int32)
        t["vel"] = z(E, V)
        t["dist_r"] = z(E, V)
        t["ang_r"] = z(E, V)
        t["pl"] = z(E, V)
        t["h_r"] = z(E, V, M, 2)        # all-zero until compute_parms(), like Environment.py:162
        t["theta"] = z(E, M, 2)         # all-zero start, Environment.py:171
        t["b"] = torch.from_numpy(np.stack([self.phase_R.real, self.phase_R.imag], -1).astype(np.float32)).to(dev)
        # step()'s per-env float32 state and outputs are views into ONE allocation (each view 256-byte aligned): the
        # kernels do not care, and a host that wants them all after a step -- the E = 1 facade, which returns the
        # reference's 7-tuple and 13 last_* scalars as NumPy values -- reads them back with one copy instead of nine
        slab_shapes = [("reward", (E, V)), ("over_power", (E, V)), ("data_buf", (E, V)), ("data_t", (E, V)),
                       ("data_p", (E, V)), ("over_data", (E, V)), ("rate", (E, V)), ("gain", (E, V)), ("mec_q", (E,)),
                       ("metrics", (E, N.METRICS)), ("power_w", (E, 2, V)), ("obs", (E, V, 5))]
        offs, n = {}, 0
        for k, shp in slab_shapes:
            offs[k] = n
            n += (int(np.prod(shp)) + 63) // 64 * 64
        slab = z(n)
        for k, shp in slab_shapes:
            t[k] = slab[offs[k]:offs[k] + int(np.prod(shp))].view(*shp)
        self._out_slab, self._out_offsets = slab, {k: (offs[k], shp) for k, shp in slab_shapes}
        # BCD column sums (sum_v h_r) * b in f64, lane-major slabs of 64 envs: [ceil(E/64), M, 64, 2]
        t["c_col"] = z((E + 63) // 64, M, 64, 2, dt=torch.float64)
        t["s_sum"] = z(E, 2, dt=torch.float64)         # sum_m theta_m c_m left by the last sweep
        t["z_r"] = z(E, V, 2, dt=torch.float64)        # steering base exp(-j pi angle) per vehicle: h_r[e,v,m] = z^m
        # candidate index of every theta element as the last BCD sweep left it: [E, 32 ceil(M/32)] bytes
        t["theta_idx"] = z(E, (M + 31) // 32 * 32, dt=torch.uint8)
        # the float64 angle every h_r row is a function of (ang_r: its float32) and, where the rows are whole 16-element
        # chunks, directly behind it the float64 head exp(-j pi ang 16 c) of every chunk (risvec_steer_heads): one
        # allocation, because that is how RISVEC_STEP_STEER_HEADS_CURRENT finds the heads
        if M % 16 == 0:
            steer = z(E * V * (1 + 2 * (M // 16)), dt=torch.float64)
            t["steer_ang"] = steer[:E * V].view(E, V)
            t["steer_head"] = steer[E * V:].view(E, V, M // 16, 2)
            assert t["steer_head"].data_ptr() % 16 == 0 or V not in (4, 8, 16)
        else:
            t["steer_ang"] = z(E, V, dt=torch.float64)
        s = N.RisVecState()
        s.abi_version = N.ABI_VERSION
        s.struct_bytes = C.sizeof(N.RisVecState)
        s.n_envs, s.n_veh, s.n_ris, s.control_bit = E, V, M, self.control_bit
        s.env_offset = self.env_offset
        for k in ("pos", "dir", "vel", "dist_r", "ang_r", "pl", "h_r", "theta", "b", "gain", "data_buf",
                  "mec_q", "rate", "data_t", "data_p", "reward", "over_power", "obs", "metrics", "power_w", "c_col",
                  "s_sum", "over_data", "z_r", "theta_idx", "steer_ang"):
            setattr(s, k, t[k].data_ptr())
        s.h_d = None
        self._cstate = s
        self._place_stream()

    # how the h_r allocation was chosen (None: not needed / switched off); bench.py reports it
    placement: Optional[dict] = None

    # send RISVEC_STEP_STEER_HEADS_CURRENT with RISVEC_STEP_H_R_STEER_CURRENT while the heads are current (same outputs
    # either way; False keeps the GEN members on sincospi: tests and A/Bs)
    steer_heads: bool = True

    def _place_stream(self) -> None:
        """h_r is THE stream of the fused step.  Once it no longer fits the Infinity Cache, the rate at which the kernels
        stream it depends on WHERE the allocation landed in HBM: two levels ~8 % apart, a property of the allocation (in
        one process the first few GB handed out stream slower than later ones; `tools/placement_probe.py`,
        EXPERIMENTS.md round 3).  So the stream is placed by measurement: up to 10 candidate allocations are timed with
        the fused step kernel itself (on the all-zero state, wiped afterwards) and the fastest is kept; the
        others go back to torch's allocator.  A few milliseconds at construction, at most 25 % of the free memory in
        flight; RISVEC_NO_PLACEMENT=1 switches it off."""
        import os
        t = self._t
        nbytes = t["h_r"].numel() * 4
        if nbytes <= (256 << 20) or os.environ.get("RISVEC_NO_PLACEMENT"):
            return
        free, _ = torch.cuda.mem_get_info(self.device)
        n_max = min(10, 1 + int(0.25 * free // nbytes))
        if n_max < 2:
            return
        lib, cs, pp, stream = N.load(), C.byref(self._cstate), C.byref(self._p()), N.stream(self.device)
        E, V = self.n_envs, self.n_veh
        act = torch.zeros(E, 2, V, device=self.device)
        part = torch.full((E, V), -1, dtype=torch.int32, device=self.device)
        ngr = torch.full((E,), V, dtype=torch.int32, device=self.device)
        flags = N.STEP_METRICS | N.STEP_OBS

        def gain_us(h) -> float:                       # the fused step itself on an all-zero state (wiped afterwards)
            self._cstate.h_r = h.data_ptr()
            best = float("inf")
            for i in range(4):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                N.check(lib.risvec_step_fused(cs, pp, act.data_ptr(), part.data_ptr(), ngr.data_ptr(), None, self.seed, i, flags,
                                              stream))
                b.record()
                b.synchronize()
                if i:                                  # the first launch warms the code path
                    best = min(best, a.elapsed_time(b) * 1e3)
            return best

        cands = [(gain_us(t["h_r"]), t["h_r"])]
        while len(cands) < n_max:
            c = torch.zeros_like(cands[0][1])
            cands.append((gain_us(c), c))
            if min(x[0] for x in cands) < 0.96 * max(x[0] for x in cands):
                break                                  # both levels seen: the faster one is known
        us, keep = min(cands, key=lambda x: x[0])
        t["h_r"] = keep
        self._cstate.h_r = keep.data_ptr()
        self.placement = dict(candidates=len(cands), step_kernel_us=[round(x[0], 1) for x in cands], kept_us=round(us, 1))
        self._out_slab.zero_()                         # the timing steps ran on (and dirtied) the all-zero state

    def set_direct_link(self, h_d: Optional[torch.Tensor]) -> None:
        """Optional direct BS link amplitude h_d [E,V] complex64 (the reference has none:
        Environment.py:263-273); None restores the reference behaviour."""
        self._ensure_device()
        if h_d is None:
            self._t.pop("h_d", None)
            self._cstate.h_d = None
            return
        h = torch.view_as_real(h_d.to(self.device, torch.complex64)).contiguous()
        if tuple(h.shape) != (self.n_envs, self.n_veh, 2):
            raise ValueError("h_d must have shape [n_envs, n_veh]")
        self._t["h_d"] = h
        self._cstate.h_d = h.data_ptr()

    def _p(self) -> N.RisVecParams:
        if self._cparams is None or self._cparams_version != self.params.version:
            self._cparams = self.params.to_c(self._lanes(), self.width, self.height)
            self._cparams_version = self.params.version
        return self._cparams

    def _arg(self, x, dtype, shape, name) -> Optional[torch.Tensor]:
        return N.converted(x, dtype, shape, name, self.device)

    def _bound(self, x, dtype, shape, name) -> Optional[torch.Tensor]:
        return N.in_place(x, dtype, shape, name, self.device)

    # ------------------------------------------------------------------ tensors (views)
    @property
    def tensors(self) -> Dict[str, torch.Tensor]:
        self._ensure_device()
        self._sync_theta()
        return self._t

    def _theta_from_index(self) -> None:
        N.check(N.load().risvec_theta_from_index(C.byref(self._cstate), N.stream(self.device)))

    def _theta_by_index_supported(self) -> bool:
        return bool(N.load().risvec_theta_by_index_supported(self.n_veh, self.M))

    def __getattr__(self, name):
        t = self.__dict__.get("_t")
        alias = _TENSOR_ALIASES.get(name)
        if alias is not None and t is not None:
            self._ensure_device()
            return self._t[alias]
        return ParamAttrs.__getattr__(self, name)

    @property
    def elements_phase_shift_complex(self) -> torch.Tensor:
        return torch.view_as_complex(self.tensors["theta"])

    @property
    def phases_R_i(self) -> torch.Tensor:
        return torch.view_as_complex(self.tensors["h_r"])

    # ------------------------------------------------------------------ reference methods
    def make_new_game(self, spawn_ints=None, buf0=None) -> None:
        """Environment.py:733-737 (+381-410).  Optional injected draws: spawn_ints
        [E,V,3] int32 (aux, coord, velocity), buf0 [E] int32."""
        self._ensure_device()
        E, V = self.n_envs, self.n_veh
        si = self._arg(spawn_ints, torch.int32, (E, V, 3), "spawn_ints")
        b0 = self._arg(buf0, torch.int32, (E,), "buf0")
        self._epoch += 1
        N.check(N.load().risvec_reset(C.byref(self._cstate), C.byref(self._p()), N.ptr(si), N.ptr(b0),
                                      self.seed, self._epoch, N.stream(self.device)))
        self._obs_stale = True         # DataBuf changed under the observation the last step wrote

    def renew_positions(self, u_turn=None, return_n_used: bool = False):
        """Environment.py:412-542.  u_turn [E,V,8] float32 injected uniform draws, consumed left to right, one per
        detected lane crossing.  A move may need 2 * n_lanes of them and a row holds 8: with more than four lanes per
        direction the move is refused (RisVecError, RISVEC_ERR_UNSUPPORTED)."""
        self._ensure_device()
        E, V = self.n_envs, self.n_veh
        u = self._arg(u_turn, torch.float32, (E, V, 8), "u_turn")
        nu = torch.zeros(E, V, dtype=torch.int32, device=self.device) if return_n_used else None
        self._moves += 1
        N.check(N.load().risvec_mobility(C.byref(self._cstate), C.byref(self._p()), N.ptr(u), N.ptr(nu),
                                         self.seed, self._moves, N.stream(self.device)))
        return nu

    def compute_parms(self) -> None:
        """Environment.py:241-253: pos -> distances_R_i, angles_R_i, phases_R_i (+ path-loss factor)."""
        self._ensure_device()
        N.check(N.load().risvec_geometry(C.byref(self._cstate), C.byref(self._p()), N.stream(self.device)))
        self._geometry_written()
        self._write_steer_heads()

    def _write_steer_heads(self) -> None:
        """The chunk heads of the steer_ang now in the state (risvec_steer_heads), where the shape keeps them."""
        head = self._t.get("steer_head")
        if head is None or head.data_ptr() % 16:
            return
        N.check(N.load().risvec_steer_heads(C.byref(self._cstate), head.data_ptr(), N.stream(self.device)))
        self._heads_written()

    def rebuild_colsum(self) -> None:
        """Recompute the BCD cache c_col[e,m] = (sum_v h_r[e,v,m]) b[m] (float64).  compute_parms()
        does it already; call this after writing `tensors["h_r"]` directly (which also ends the
        validity of the steering form of the fused step, `steer=True`).  theta, its cached sum aside, is
        left as it is: candidate indices the last sweep kept stay valid (the next sweep re-sums theta.c)."""
        self._ensure_device()
        N.check(N.load().risvec_colsum(C.byref(self._cstate), N.stream(self.device)))
        self._colsum_rebuilt()

    def colsum_rows(self) -> torch.Tensor:
        """The BCD cache as [E, M] complex128 (a copy; the device layout is lane-major slabs)."""
        c = torch.view_as_complex(self.tensors["c_col"])            # [S, M, 64]
        return c.permute(0, 2, 1).reshape(-1, self.M)[: self.n_envs].clone()

    def invalidate_colsum(self) -> None:
        """Announce a direct write to `tensors["h_r"]` (and/or `tensors["theta"]`): the next BCD rebuilds c_col,
        re-sums theta.c and re-derives the candidate indices, and the steering form of the fused step
        (`steer=True`) is refused until compute_parms() writes steering vectors again.  theta is handled as by
        invalidate_theta(): if it was not written, what the sweeps left in it is kept."""
        self._h_r_write_announced()

    def invalidate_theta(self) -> None:
        """Announce a direct write to `tensors["theta"]`: the written tensor becomes theta, and the next BCD sweep
        re-sums theta.c and re-derives the candidate indices (the phase setters and the sweeps themselves keep
        track on their own).  With lazy_theta, where the last sweeps may have kept theta by index only, a theta
        tensor that torch has not written since (its `_version` has not moved) is first materialised from those
        indices, so an announcement without a theta write loses no sweep."""
        self._theta_write_announced()

    def optimize_phase_shift(self, return_idx: bool = False, reuse_colsum: Optional[bool] = None):
        """Environment.py:208-220 (one BCD sweep, objective of :222-231).  The column sums the
        sweep needs are pure geometry; they are reused when known current (after
        compute_parms()/rebuild_colsum()), otherwise rebuilt first.  reuse_colsum overrides."""
        self._ensure_device()
        idx = torch.zeros(self.n_envs, self.M, dtype=torch.int32, device=self.device) if return_idx else None
        flags = self._sweep_flags(reuse_colsum, False)
        N.check(N.load().risvec_bcd(C.byref(self._cstate), C.byref(self._p()), N.ptr(idx), flags, N.stream(self.device)))
        self._sweep_ran(flags, False)
        return idx

    def update_channel_gains(self, u_los=None, z_shadow=None, small=None) -> None:
        """Environment.py:255-327, dispatching on `channel_model` like the reference
        (unknown keywords fall back to a 0 dB path loss, :315-317)."""
        self._ensure_device()
        model = str(self.params.channel_model)
        if model == "free":
            self._sync_theta()
            N.check(N.load().risvec_gain(C.byref(self._cstate), C.byref(self._p()), N.stream(self.device)))
            return
        E, V = self.n_envs, self.n_veh
        ul = self._arg(u_los, torch.float32, (E, V), "u_los")
        zs = self._arg(z_shadow, torch.float32, (E, V), "z_shadow")
        sm = self._arg(small, torch.float32, (E, V), "small")
        self._chan += 1
        N.check(N.load().risvec_gain_3gpp(C.byref(self._cstate), C.byref(self._p()),
                                          CHANNEL_MODELS.get(model, N.CH_OTHER), N.ptr(ul), N.ptr(zs),
                                          N.ptr(sm), self.seed, self._chan, N.stream(self.device)))

    def get_channel_gains(self) -> torch.Tensor:
        """Environment.py:374-376."""
        return self.tensors["gain"]

    def get_next_phase(self, action_phase) -> None:
        """Environment.py:233-239: theta = exp(j * angle), angle [E,M]."""
        self._ensure_device()
        a = self._arg(action_phase, torch.float32, (self.n_envs, self.M), "action_phase")
        N.check(N.load().risvec_set_phase(C.byref(self._cstate), N.ptr(a), N.stream(self.device)))
        self._theta_set(False)

    def Random_phase(self, idx=None) -> None:
        """Environment.py:203-206; idx [E,M] int32 indices into possible_angles (optional)."""
        self._ensure_device()
        i = self._arg(idx, torch.int32, (self.n_envs, self.M), "idx")
        self._chan += 1
        N.check(N.load().risvec_random_phase(C.byref(self._cstate), N.ptr(i), self.seed, self._chan,
                                             N.stream(self.device)))
        self._theta_set(True)      # with 2^b = 8 the kernel writes each element's index as well

    def data_rate(self, p_off, partner, n_groups) -> torch.Tensor:
        """Environment.py:331-372 on the cached gains: p_off [E,V] offload power in W -> rate [E,V]."""
        self._ensure_device()
        E, V = self.n_envs, self.n_veh
        pw = self._arg(p_off, torch.float32, (E, V), "p_off")
        pt = self._arg(partner, torch.int32, (E, V), "partner")
        ng = self._arg(n_groups, torch.int32, (E,), "n_groups")
        out = torch.empty(E, V, dtype=torch.float32, device=self.device)
        N.check(N.load().risvec_data_rate(C.byref(self._cstate), C.byref(self._p()), N.ptr(pw), N.ptr(pt),
                                          N.ptr(ng), N.ptr(out), N.stream(self.device)))
        return out

    def _steer_flag(self, steer: bool, fused: bool) -> int:
        if not steer:
            return 0
        if not fused:
            raise ValueError("steer=True is a form of the fused gain+step kernel: pass fused=True")
        if not self._steer_valid:
            raise ValueError("steer=True needs h_r to be the steering vectors compute_parms() wrote "
                             "(call compute_parms(); h_r written by hand has no steering base)")
        return N.STEP_STEER

    @staticmethod
    def _step_flags(metrics: bool, power_w: bool, obs: bool, policy_action: bool) -> int:
        return ((N.STEP_METRICS if metrics else 0) | (N.STEP_POWER_W if power_w else 0)
                | (N.STEP_OBS if obs else 0) | (N.STEP_POLICY_ACTION if policy_action else 0))

    def _model(self, fused: bool, steer: bool, fading) -> Optional[int]:
        """Which kind of launch a step call is NOW (`params.channel_model` may change between calls): RISVEC_CH_* when a
        fused form updates the 3GPP gains (what `update_channel_gains` dispatches on; unknown keywords: CH_OTHER, a
        0 dB path loss), None for a RIS-cascade / cached-gain launch.  Each kind refuses what the other owns."""
        model = str(self.params.channel_model)
        if fused and model != "free":
            if steer:
                raise ValueError("steer=True is a form of the RIS cascade; channel_model=%r has no RIS in the gain"
                                 % (model,))
            return CHANNEL_MODELS.get(model, N.CH_OTHER)
        if fading is not None:
            raise ValueError("fading= is accepted by the fused step forms under a 3GPP channel_model only "
                             "(channel_model=%r)" % (model,))
        return None

    @staticmethod
    def _fading(conv, fading, shape):
        """Injected fading draws (u_los, z_shadow, small) of a fused 3GPP step -> (tensors, RisVecFading or None)."""
        if fading is None:
            return None, None
        if len(fading) != 3 or any(x is None for x in fading):
            raise ValueError("fading must be (u_los, z_shadow, small), all three given")
        ts = tuple(conv(x, torch.float32, shape, n) for x, n in zip(fading, ("u_los", "z_shadow", "small")))
        return ts, N.RisVecFading(*(N.ptr(x) for x in ts))

    # Every step call has ONE implementation, `_bind_*(conv, ...)`: validate, marshal once, return the launcher.  `conv`
    # is the whole difference between the public twins: `bind_*` passes `_bound` (inputs used in place or refused), the
    # unbound method passes `_arg` (converted, copied if needed) and calls the launcher once.
    def step(self, action_power, partner, n_groups, arrivals=None, fused: bool = False, bcd: bool = False,
             metrics: bool = True, power_w: bool = True, obs: bool = True, policy_action: bool = False,
             steer: bool = False, fading=None) -> Tuple[torch.Tensor, ...]:
        """Environment.py:547-731 for every env.

        action_power [E,2,V] float32 (or the policy output [E,V,2] with policy_action=True,
        marl_train_bcd.py:1601-1608); partner [E,V] int32 / n_groups [E] int32 encode
        `noma_groups` (see `compat.encode_noma_groups`); arrivals [E,V] int32 = injected
        Poisson draws (None: in-kernel Philox).  fused=True recomputes the RIS cascaded
        gains in the same launch (the north-star kernel); bcd=True additionally runs a BCD
        sweep first; steer=True (with fused) uses the fact that compute_parms made every h_r row a
        geometric sequence z^m and evaluates the cascade by Horner in float64 from the 16-byte base
        instead of reading the 8M-byte row (same results to ~1e-7; ~4x fewer bytes per step).
        Under a 3GPP channel_model the fused forms update the 3GPP gains instead (`risvec_step_fused_3gpp`: what
        update_channel_gains() + step(fused=False) do, in one launch; bcd=True runs optimize_phase_shift() first, as
        the driver does); fading=(u_los, z_shadow, small) [E,V] injects their draws (None: Philox).
        Returns the reference's 7-tuple, batched:
        (per_user_reward [E,V], global_reward [E], DataBuf, data_t, data_p, over_power, over_data);
        the tensors are owned by the env and overwritten by the next step."""
        self._bind_step(self._arg, action_power, partner, n_groups, arrivals, fused, bcd, metrics, power_w, obs,
                        policy_action, steer, fading)()
        t = self._t
        return (t["reward"], t["metrics"][:, 0], t["data_buf"], t["data_t"], t["data_p"], t["over_power"],
                t["over_data"])

    def bind_step(self, action_power, partner, n_groups, arrivals=None, fused: bool = False, bcd: bool = False,
                  metrics: bool = True, power_w: bool = True, obs: bool = True, policy_action: bool = False,
                  steer: bool = False, fading=None):
        """Validate and marshal a `step()` call ONCE and return a zero-argument callable that
        launches one step per call on the stream current at bind time, reading the SAME input
        tensors each time (update them in place between calls).  Cuts the per-step host cost
        from ~10 us of Python argument handling to one ctypes call, which matters when a
        batched step is only a few microseconds of GPU time (small E)."""
        # the launcher reads these tensors IN PLACE on every call, so they must already be what the
        # kernel reads: a silent .to()/.contiguous() copy would detach the caller's later updates
        return self._bind_step(self._bound, action_power, partner, n_groups, arrivals, fused, bcd, metrics, power_w, obs,
                               policy_action, steer, fading)

    def _bind_step(self, conv, action_power, partner, n_groups, arrivals, fused, bcd, metrics, power_w, obs,
                   policy_action, steer, fading):
        self._ensure_device()
        E, V = self.n_envs, self.n_veh
        a = conv(action_power, torch.float32, (E, V, 2) if policy_action else (E, 2, V), "action_power")
        pt = conv(partner, torch.int32, (E, V), "partner")
        ng = conv(n_groups, torch.int32, (E,), "n_groups")
        ar = conv(arrivals, torch.int32, (E, V), "arrivals")
        fused = fused or bcd                           # a sweep only exists in front of the fused step
        fd_t, fd = self._fading(conv, fading, (E, V))
        self._model(fused, steer, fd)                  # refuse now what every launch would refuse
        flags3 = self._step_flags(metrics, power_w, obs, policy_action)
        base_flags = flags3 | self._steer_flag(steer, fused)
        lib = N.load()
        fn = lib.risvec_step_fused_bcd if bcd else (lib.risvec_step_fused if fused else lib.risvec_step)
        fn3 = lib.risvec_step_fused_3gpp
        cs, seed, stream = C.byref(self._cstate), C.c_uint64(self.seed), N.stream(self.device)
        pa, pp, pn, par = N.ptr(a), N.ptr(pt), N.ptr(ng), N.ptr(ar)
        pfd = C.byref(fd) if fd is not None else None
        by_index = not steer                           # a launch that may read theta as candidate indices
        current = not bcd and not steer                # ... that may be told "theta_idx matches theta", "h_r is what
                                                       # compute_parms() wrote"

        def launch() -> None:
            model = self._model(fused, steer, fd) if fused else None
            if model is not None:            # the fused forms under a 3GPP channel model (the RIS is not in the gain)
                if bcd:
                    self.optimize_phase_shift()
                self._chan += 1
                rc = fn3(cs, C.byref(self._p()), model, pa, pp, pn, par, pfd, seed, self._steps, self._chan, flags3, None,
                         stream)
                if rc:
                    N.check(rc)
            else:
                flags = base_flags | self._sweep_flags(None, True) if bcd else base_flags
                if fused:
                    flags |= self._fused_launch(by_index, current)
                rc = fn(cs, C.byref(self._p()), pa, pp, pn, par, seed, self._steps, flags, stream)
                if rc:
                    N.check(rc)
                if bcd:
                    self._sweep_ran(flags, True)
            self._steps += 1
            self._obs_stale = not obs

        launch.inputs = (a, pt, ng, ar, fd_t, fd)      # the closure owns the marshalled tensors
        return launch

    def _traj_shapes(self, actions) -> Tuple[int, Dict[str, tuple]]:
        """(T, shapes of the per-step records) of a T-step call on `actions` [T,E,...]."""
        shape = np.shape(actions)
        if len(shape) != 4 or shape[0] < 1:
            raise ValueError("actions must be a [T, E, ...] array holding at least one step, got shape %s" % (tuple(shape),))
        T, E, V = int(shape[0]), self.n_envs, self.n_veh
        return T, {"reward": (T, E, V), "obs": (T, E, V, 5), "metrics": (T, E, N.METRICS)}

    def step_many(self, actions, partner, n_groups, arrivals=None, metrics: bool = True, power_w: bool = False,
                  obs: bool = True, policy_action: bool = False, record: Sequence[str] = ("reward", "obs", "metrics"),
                  out: Optional[Dict[str, torch.Tensor]] = None, fused: bool = True, fading=None) -> Dict[str, torch.Tensor]:
        """T consecutive fused `step()` calls in ONE launch (`risvec_step_fused_multi`): the driver's step loop
        marl_train_bcd.py:1304-1611 between two channel refreshes with the NOMA groups frozen, as they are
        inside an episode.  actions [T,E,2,V] float32 (or [T,E,V,2] with policy_action=True); partner / n_groups as
        for `step()` (the same for every step); arrivals [T,E,V] int32 injected draws or None (Philox with the
        counters T single calls would use).  The env's tensors end up exactly as after the last of T single
        `step(..., fused=True)` calls, bit for bit; `record` names the per-step records to keep
        ("reward" [T,E,V], "obs" [T,E,V,5], "metrics" [T,E,16]) -- returned as a dict, written into `out`'s
        tensors when given.  h_r / theta cannot change inside the launch, so the gains are computed once and each
        env's queues stay in registers: this is the launch to use when a batched step is shorter than a kernel
        launch (small E).  fused=False (`risvec_step_multi`) is the same on the CACHED gains -- T `step(...,
        fused=False)` calls, the reference driver's own cadence (gains only every 100 steps), any shape, h_r / theta
        not read at all.  Under a 3GPP channel_model fused=True is `risvec_step_fused_3gpp_multi`: T fused 3GPP steps,
        fresh fading every step (fading=(u_los, z_shadow, small) [T,E,V] injects it)."""
        self._ensure_device()
        shapes = self._traj_shapes(actions)[1]
        rec: Dict[str, torch.Tensor] = {}
        for k in record:
            if k not in shapes:
                raise ValueError("record: unknown trajectory record %r (choose from %s)" % (k, sorted(shapes)))
            if out is not None and k in out:
                rec[k] = out[k]
            else:
                rec[k] = torch.empty(shapes[k], dtype=torch.float32, device=self.device)
        self._bind_step_many(self._arg, actions, partner, n_groups, arrivals, metrics, power_w, obs, policy_action, rec,
                             fused, fading)()
        return rec

    def bind_step_many(self, actions: torch.Tensor, partner: torch.Tensor, n_groups: torch.Tensor,
                       arrivals: Optional[torch.Tensor] = None, metrics: bool = True, power_w: bool = False,
                       obs: bool = True, policy_action: bool = False,
                       out: Optional[Dict[str, torch.Tensor]] = None, fused: bool = True, fading=None):
        """`step_many` validated and marshalled once: returns a zero-argument launcher that advances the env by
        T steps per call, reading `actions` [T,E,...] (and `arrivals`) in place and writing the per-step records
        into `out`'s tensors ("reward" [T,E,V], "obs" [T,E,V,5], "metrics" [T,E,16]; any subset)."""
        return self._bind_step_many(self._bound, actions, partner, n_groups, arrivals, metrics, power_w, obs,
                                    policy_action, out, fused, fading)

    def _bind_step_many(self, conv, actions, partner, n_groups, arrivals, metrics, power_w, obs, policy_action, out,
                        fused, fading):
        self._ensure_device()
        E, V = self.n_envs, self.n_veh
        T, shapes = self._traj_shapes(actions)
        a = conv(actions, torch.float32, (T, E, V, 2) if policy_action else (T, E, 2, V), "actions")
        pt = conv(partner, torch.int32, (E, V), "partner")
        ng = conv(n_groups, torch.int32, (E,), "n_groups")
        ar = conv(arrivals, torch.int32, (T, E, V), "arrivals")
        if not obs and "obs" in (out or {}):
            raise ValueError("record 'obs' needs obs=True")
        # the records are written in place whoever asks: never converted
        rec = {k: self._bound(t, torch.float32, shapes[k], "out[%r]" % k) for k, t in (out or {}).items()}
        tj = N.RisVecTraj(N.ptr(rec.get("reward")), N.ptr(rec.get("obs")), N.ptr(rec.get("metrics")))
        fd_t, fd = self._fading(conv, fading, (T, E, V))
        self._model(fused, False, fd)                  # refuse now what every launch would refuse
        flags = self._step_flags(metrics, power_w, obs, policy_action)
        fn = N.load().risvec_step_fused_multi if fused else N.load().risvec_step_multi
        fn3 = N.load().risvec_step_fused_3gpp_multi
        cs, seed, stream = C.byref(self._cstate), C.c_uint64(self.seed), N.stream(self.device)
        pa, pp, pn, par, ptj = N.ptr(a), N.ptr(pt), N.ptr(ng), N.ptr(ar), C.byref(tj)
        pfd = C.byref(fd) if fd is not None else None

        def launch() -> None:
            model = self._model(fused, False, fd) if fused else None
            if model is not None:            # the fused form under a 3GPP channel model (the RIS is not in the gain)
                # handed the FIRST channel counter of its T draws; the single step advances before its call
                rc = fn3(cs, C.byref(self._p()), model, T, pa, pp, pn, par, pfd, seed, self._steps, self._chan + 1, ptj,
                         flags, stream)
                if rc:
                    N.check(rc)
                self._chan += T
            else:
                if fused:
                    self._fused_launch(False, False)     # reads the complex64 theta, takes no bits
                rc = fn(cs, C.byref(self._p()), T, pa, pp, pn, par, seed, self._steps, flags, ptj, stream)
                if rc:
                    N.check(rc)
            self._steps += T
            self._obs_stale = not obs

        launch.inputs = (a, pt, ng, ar, rec, tj, fd_t, fd)
        launch.n_steps = T
        return launch

    def sarl_step(self, action_power, action_phase=None, arrivals=None, sarl_params=None, obs: bool = True
                  ) -> Tuple[torch.Tensor, ...]:
        """The single-agent variant's step (Simulation-SARL/Environment.py:321-359) for every env:
        action_power [E,2,V] float32 used as given, action_phase [E,M] radians (None keeps the
        current theta), arrivals [E,V] int32 injected Poisson draws (None: Philox).  Returns the
        reference's 6-tuple, batched: (Reward [E], DataBuf, data_t, data_p, over_power, over_data)."""
        self._bind_sarl_step(self._arg, action_power, action_phase, arrivals, sarl_params, obs)()
        t = self._t
        return (t["metrics"][:, 0], t["data_buf"], t["data_t"], t["data_p"], t["over_power"], t["over_data"])

    def bind_sarl_step(self, action_power: torch.Tensor, action_phase: Optional[torch.Tensor] = None,
                       arrivals: Optional[torch.Tensor] = None, sarl_params=None, obs: bool = True):
        """`sarl_step` validated and marshalled once: returns a zero-argument launcher that reads the SAME device
        tensors on every call (update them in place between calls).  The parameters are those of `sarl_params` at
        bind time."""
        return self._bind_sarl_step(self._bound, action_power, action_phase, arrivals, sarl_params, obs)

    def _bind_sarl_step(self, conv, action_power, action_phase, arrivals, sarl_params, obs):
        from .sarl import SarlParams
        self._ensure_device()
        E, V, M = self.n_envs, self.n_veh, self.M
        a = conv(action_power, torch.float32, (E, 2, V), "action_power")
        ph = conv(action_phase, torch.float32, (E, M), "action_phase")
        ar = conv(arrivals, torch.int32, (E, V), "arrivals")
        sp = (sarl_params or SarlParams()).to_c()
        fn, cs, psp, seed, stream = N.load().risvec_sarl_step, C.byref(self._cstate), C.byref(sp), C.c_uint64(self.seed), N.stream(self.device)
        pa, pph, par, flags = N.ptr(a), N.ptr(ph), N.ptr(ar), N.STEP_OBS if obs else 0

        def launch() -> None:
            self._sync_theta()
            rc = fn(cs, psp, pa, pph, par, seed, self._steps, flags, stream)
            if rc:
                N.check(rc)
            if ph is not None:
                self._theta_set(False)
            self._steps += 1
            self._obs_stale = False        # sarl_observe assembles its own observation from the state tensors

        launch.inputs = (a, ph, ar, sp)
        return launch

    def sarl_rollout(self, mu, noise=None, replay=None, z=None, arrivals=None, sarl_params=None, done: bool = False
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """One SARL rollout step in one launch (see `bind_sarl_rollout`), inputs converted as needed.  Returns
        (action [E, 2V+M], phase [E, M], obs_full [E, V, M//V + 5])."""
        launch = self._bind_sarl_rollout(self._arg, mu, noise, replay, z, arrivals, sarl_params)
        launch(done)
        return launch.action, launch.phase, launch.obs

    def bind_sarl_rollout(self, mu: torch.Tensor, noise=None, replay=None, z: Optional[torch.Tensor] = None,
                          arrivals: Optional[torch.Tensor] = None, sarl_params=None):
        """Everything `ddpg_train.py:114-185` does between the actor's output and the replay buffer, for every env in ONE
        launch (`risvec_sarl_rollout`): OU exploration noise on `noise.x` in place (an `OUNoise`; None: the action is
        `mu`; `z` [E, 2V+M] injects its N(0,1) draws), a = clip(mu + x, +-0.999), the power / phase map, get_next_phase,
        the cascaded gains and `step()`, every agent's observation with its phase slice, and -- with `replay`, a
        `SarlReplayBuffer(mem, M//V + 5, 2V+M, V)` -- the transition store (state = the observation the launch found).
        Returns `launch(done=False)`; `mu` [E, 2V+M] (the raw actor output), `z` and `arrivals` are read in place on every
        call.  `launch.action`, `launch.phase` and `launch.obs` are the output tensors; `launch.obs` is the env's SARL
        observation, shared by every launcher of this env and, before the first step or after anything else stepped or
        reset the env, assembled from the state with a zero phase slice (SENV:105), as `observe()` does for MARL.
        Shapes: V in {4, 8, 16}, even M with V <= M <= 256; the launch raises `RisVecError` elsewhere (`sarl_step` serves
        every shape)."""
        return self._bind_sarl_rollout(self._bound, mu, noise, replay, z, arrivals, sarl_params)

    def _bind_sarl_rollout(self, conv, mu, noise, replay, z, arrivals, sarl_params):
        from .sarl import SarlParams
        self._ensure_device()
        E, V, M = self.n_envs, self.n_veh, self.M
        A, tn = 2 * V + M, M // V
        m = conv(mu, torch.float32, (E, A), "mu")
        zz = conv(z, torch.float32, (E, A), "z")
        ar = conv(arrivals, torch.int32, (E, V), "arrivals")
        if zz is not None and noise is None:
            raise ValueError("z injects the draws of `noise`: give an OUNoise")
        r = N.RisVecSarlRollout()
        r.struct_bytes = C.sizeof(N.RisVecSarlRollout)
        r.mu, r.z = m.data_ptr(), N.ptr(zz)
        if noise is not None:
            self._bound(noise.x, torch.float32, (E, A), "noise.x")
            r.ou_x = noise.x.data_ptr()
            r.ou_theta, r.ou_mu, r.ou_sigma, r.ou_dt = noise.theta, noise.mu, noise.sigma, noise.dt
            r.ou_seed, r.ou_env_offset = noise.seed, noise.env_offset
        if replay is not None:
            if (replay.device != self.device or replay.n_agents != V or replay.input_shape != tn + 5
                    or replay.n_actions != A or replay.mem_size < E):
                raise ValueError("bind_sarl_rollout: the replay buffer must live on %s with n_agents=%d, input_shape=%d, "
                                 "n_actions=%d and mem_size >= %d" % (self.device, V, tn + 5, A, E))
            for k in replay._ARRAYS:
                setattr(r, k, getattr(replay, k).data_ptr())
            r.mem_size = replay.mem_size
        action = torch.empty(E, A, dtype=torch.float32, device=self.device)
        phase = torch.empty(E, M, dtype=torch.float32, device=self.device)
        obs = self.sarl_observation()
        r.action, r.phase, r.obs_full = action.data_ptr(), phase.data_ptr(), obs.data_ptr()
        sp = (sarl_params or SarlParams()).to_c()
        fn, cs, psp, pr, seed, stream = (N.load().risvec_sarl_rollout, C.byref(self._cstate), C.byref(sp), C.byref(r),
                                         C.c_uint64(self.seed), N.stream(self.device))
        par = N.ptr(ar)

        def launch(done: bool = False) -> None:
            self.sarl_observation()              # the ring's `state` is the observation tensor as the kernel finds it
            r.done = 1 if done else 0
            if replay is not None:
                r.mem_cntr = replay.mem_cntr
            rc = fn(cs, psp, pr, par, seed, self._steps, N.STEP_OBS, stream)
            if rc:
                N.check(rc)
            if replay is not None:
                replay.mem_cntr += E
            self._steps += 1
            self._theta_set(False)
            self._obs_stale = False
            self._sarl_obs_mark = (self._epoch, self._steps)

        launch.action, launch.phase, launch.obs = action, phase, obs
        launch.inputs = (m, zz, ar, noise, replay, sp, r)
        return launch

    def bind_step_store(self, replay, power_raw: torch.Tensor, partner: torch.Tensor, n_groups: torch.Tensor,
                        probs: torch.Tensor, mask: Optional[torch.Tensor] = None, arrivals: Optional[torch.Tensor] = None,
                        fused: bool = True, metrics: bool = True, power_w: bool = False, fading=None):
        """The rollout step with the transition store fused in (`risvec_step_ring`; marl_train_bcd.py:1601-1611,
        1776-1799): ONE launch runs `step()` on the raw policy output `power_raw` [E,V,2] and appends this step's E
        transitions to `replay` (a `VecReplayBuffer` with input_shape 5, n_actions V+2, n_agents V) -- state = the
        observation the env holds when the launch starts, action row = [probs_i with zero diagonal | raw power_i],
        rewards and the new observation straight from the step's registers.  Ring contents and env tensors are those
        of `bind_step(policy_action=True)` followed by `replay.bind_store(..., policy_out=(power_raw, probs))`, bit
        for bit.  Returns `launch(done=False, use_mask=True)`; all tensors are read in place on every call.
        fused=True needs a shape with a software-pipelined kernel ((8,64), (8,36), (8,40), (4,16), (16,64), (16,256));
        fused=False steps on the cached gains, any M.  Under a 3GPP channel_model fused=True updates the 3GPP gains
        in the same launch instead (`risvec_step_fused_3gpp` with the ring; any M, V in {4, 8, 16}); fading=(u_los,
        z_shadow, small) [E,V] device tensors inject its draws, read in place."""
        self._ensure_device()
        E, V = self.n_envs, self.n_veh
        a = self._bound(power_raw, torch.float32, (E, V, 2), "power_raw")
        pt = self._bound(partner, torch.int32, (E, V), "partner")
        ng = self._bound(n_groups, torch.int32, (E,), "n_groups")
        pr = self._bound(probs, torch.float32, (E, V, V), "probs")
        mk = self._bound(mask, torch.uint8, (E, V, V), "mask")
        ar = self._bound(arrivals, torch.int32, (E, V), "arrivals")
        if replay.device != self.device or replay.n_agents != V or replay.input_shape != 5 or replay.n_actions != V + 2:
            raise ValueError("bind_step_store: the replay buffer must live on %s with n_agents=%d, input_shape=5, n_actions=%d"
                             % (self.device, V, V + 2))
        fd_t, fd = self._fading(self._bound, fading, (E, V))
        self._model(fused, False, fd)                  # refuse now what every launch would refuse
        flags = self._step_flags(metrics, power_w, True, True)
        ring = N.RisVecStepRing()
        ring.rb = replay._c
        ring.probs, ring.mask = pr.data_ptr(), None
        fn, cs, seed, stream = N.load().risvec_step_ring, C.byref(self._cstate), C.c_uint64(self.seed), N.stream(self.device)
        fn3 = N.load().risvec_step_fused_3gpp
        pa, pp, pn, par, pmask = N.ptr(a), N.ptr(pt), N.ptr(ng), N.ptr(ar), N.ptr(mk)
        fz = 1 if fused else 0
        pfd = C.byref(fd) if fd is not None else None

        def launch(done: bool = False, use_mask: bool = True) -> None:
            if self._obs_stale:
                self.observe()                   # the ring's `state` is the observation tensor as the kernel finds it
            model = self._model(fused, False, fd) if fused else None
            ring.mem_cntr, ring.done = replay.mem_cntr, 1 if done else 0
            ring.mask = pmask if use_mask else None
            if model is not None:                # fused under a 3GPP channel model: 3GPP gains + step + store
                self._chan += 1
                rc = fn3(cs, C.byref(self._p()), model, pa, pp, pn, par, pfd, seed, self._steps, self._chan, flags,
                         C.byref(ring), stream)
            else:
                fl = flags | self._fused_launch(False, True) if fused else flags
                rc = fn(cs, C.byref(self._p()), C.byref(ring), pa, pp, pn, par, seed, self._steps, fl, fz, stream)
            if rc:
                N.check(rc)
            replay.mem_cntr += E
            self._steps += 1
            self._obs_stale = False

        launch.inputs = (a, pt, ng, pr, mk, ar, ring, replay, fd_t, fd)
        return launch

    # ------------------------------------------------------------------ driver-side helpers
    def observe(self) -> torch.Tensor:
        """marl_train_bcd.py:819-827 for all agents: [E,V,5].  After a step the kernel has
        already written it; before the first step it is assembled from the state."""
        t = self.tensors
        if self._obs_stale:
            # what marl_get_state reads at this point: the CURRENT attributes (a reset replaces DataBuf
            # and leaves data_t / data_p / vehicle_rate of the last step alone, Environment.py:733-737)
            o = t["obs"]
            o[..., 0] = t["data_buf"] / 10
            o[..., 1] = t["data_t"] / 10
            o[..., 2] = t["data_p"] / 10
            o[..., 3] = 0
            o[..., 4] = t["rate"] / 20
            self._obs_stale = False
        return t["obs"]

    def sarl_observation(self) -> torch.Tensor:
        """ddpg_train.py:47-73 for all agents: [E, V, M//V + 5] = each agent's slice of the phase action followed by
        the 5-float tail.  The rollout launch (`bind_sarl_rollout`) writes it; before the first step, and after
        anything else stepped or reset the env, it is assembled from the state with a zero phase slice
        (elements_phase_shift_real starts all zero, SENV:105)."""
        self._ensure_device()
        t, tn = self._t, self.M // self.n_veh
        if "sarl_obs" not in t:
            t["sarl_obs"] = torch.zeros(self.n_envs, self.n_veh, tn + 5, dtype=torch.float32, device=self.device)
        o = t["sarl_obs"]
        if self._sarl_obs_mark != (self._epoch, self._steps):
            o[..., :tn] = 0
            for k, (key, div) in enumerate((("data_buf", 10), ("data_t", 10), ("data_p", 10), ("over_data", 10), ("rate", 20))):
                o[..., tn + k] = t[key] / div
            self._sarl_obs_mark = (self._epoch, self._steps)
        return o

    def metrics_dict(self) -> Dict[str, torch.Tensor]:
        """The 13 `last_*` scalars + global_reward, each [E] (Environment.py:612-677, 706-711)."""
        m = self.tensors["metrics"]
        return {name: m[:, i] for i, name in enumerate(N.METRIC_NAMES)}

    def begin_episode(self, i_episode: int, env_refresh_every: int = 5) -> bool:
        """Call cadence of marl_train_bcd.py:1268-1271."""
        if i_episode % max(1, int(env_refresh_every)) == 0:
            self.renew_positions()
            self.compute_parms()
            return True
        return False

    def begin_step(self, i_step: int, ris_every: int = 100) -> bool:
        """Call cadence of marl_train_bcd.py:1307-1309 (K_STEPS_FOR_RIS_OPTIMIZATION = 100)."""
        if i_step % max(1, int(ris_every)) == 0:
            self.optimize_phase_shift()
            self.update_channel_gains()
            return True
        return False

    # ------------------------------------------------------------------ checkpoint
    _STATE_KEYS = ("pos", "dir", "vel", "dist_r", "ang_r", "pl", "h_r", "z_r", "steer_ang", "theta", "gain", "data_buf", "mec_q",
                   "rate", "data_t", "data_p", "reward", "over_power", "over_data", "obs", "metrics", "power_w")

    def state_dict(self) -> Dict[str, object]:
        t = self.tensors
        sd: Dict[str, object] = {k: t[k].detach().cpu().clone() for k in self._STATE_KEYS}
        sd["counters"] = dict(epoch=self._epoch, moves=self._moves, steps=self._steps, chan=self._chan,
                              seed=self.seed, env_offset=self.env_offset, obs_stale=self._obs_stale,
                              **self._checkpoint_record())
        return sd

    def load_state_dict(self, sd: Dict[str, object]) -> None:
        """Restore a `state_dict()`.  The Philox streams are keyed by (seed, global env id), so a
        checkpoint only resumes bit-identically in an env built with the SAME seed and env_offset:
        a mismatch raises instead of silently diverging."""
        c = sd["counters"]
        for key, mine in (("seed", self.seed), ("env_offset", self.env_offset)):
            if key in c and int(c[key]) != int(mine):
                raise ValueError("load_state_dict: checkpoint was taken with %s=%d, this env has %s=%d (the RNG "
                                 "streams are keyed by it; build the env with the checkpoint's value)"
                                 % (key, int(c[key]), key, int(mine)))
        t = self.tensors
        for k in self._STATE_KEYS:
            if k in sd:                # power_w joined the checkpoint in round 2, steer_ang with the rebuilt rows
                t[k].copy_(sd[k])
        self._epoch, self._moves, self._steps, self._chan = c["epoch"], c["moves"], c["steps"], c["chan"]
        self._checkpoint_loaded(bool(c.get("steer_valid", False)), bool(c.get("h_r_steer", False)), "steer_ang" in sd)
        if "steer_ang" in sd:
            self._write_steer_heads()
        self._obs_stale = bool(c.get("obs_stale", self._steps == 0))
        self._sarl_obs_mark = None


# reference attribute name -> tensor key
_TENSOR_ALIASES = {
    "DataBuf": "data_buf", "data_t": "data_t", "data_p": "data_p", "over_data": "over_data",
    "vehicle_rate": "rate", "channel_gains": "gain", "distances_R_i": "dist_r", "angles_R_i": "ang_r",
    "mec_queue_cycles": "mec_q", "last_power_W": "power_w", "positions": "pos", "directions": "dir",
    "velocities": "vel",
}
