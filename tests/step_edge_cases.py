"""The case table of the step() edge tests (plain NumPy, no GPU): states that sit ON the branch edges of step()
(`step_pre` / `step_tail` / `noma_rate` / `log2_1p` in csrc/risvec_step.hpp), for the float64 oracle and the kernels alike.

The random step tests draw states and then leave out, through `step_mask` (tests/test_hip_parity.py), whatever lands near
a discontinuity.  Here every case is placed on one, and a DYADIC parameter set makes that exact: every field is a power of
two or a short dyadic number, so every product in front of the logarithm is exact in float32 and in float64, and the
device (float32 parameters) and the oracle (float64) decide every comparison from the same numbers.

With the base set: pw0 = a0 (while s <= 1), SINR = pw0 * gain / 2^-46, data_t = rate * 3.90625 kbit, bc = B * 256000 cycles,
cap = share * 2^20 cycles (so B = 2 kbit clears exactly at a share of 0.48828125), the edge serves 2^21 cycles per step,
one arrival is 0.9765625 kbit.

`cases(V)` returns the named cases, `batches(V)` the same grouped by parameter set (an env has one), `tests/
test_step_edges_host.py` checks the table against the oracle and `tests/test_step_edges_hip.py` runs it on the device.
"""
import dataclasses
from typing import Dict, List

import numpy as np

from oracle import risvec_oracle as orc

SECOND = orc.PARTNER_SECOND
SINGLE = orc.PARTNER_SINGLE
NONE = orc.PARTNER_NONE
NOISE = 2.0 ** -46

# the 16 physics fields step() reads (qos_enable is the 17th, a flag) and their dyadic base values
BASE = dict(bandwidth=4.0, noise_power=NOISE, P_max=2.0, power_scale=0.5, time_fast=2.0 ** -10, k=2.0 ** -93,
            f_local_max=2.0 ** 30, f_edge_max=2.0 ** 31, cycles_per_bit=256.0, cpu_share_floor=0.125, w_d=1.0, w_e=2.0,
            reward_clip=50.0, R_min_bpsHz=0.25, D_max_s=0.125, qos_penalty=1.5)
# "one field at a time": the other dyadic value of each field
OTHER = dict(bandwidth=8.0, noise_power=2.0 ** -45, P_max=4.0, power_scale=0.25, time_fast=2.0 ** -9, k=2.0 ** -90,
             f_local_max=2.0 ** 29, f_edge_max=2.0 ** 30, cycles_per_bit=512.0, cpu_share_floor=0.25, w_d=0.5, w_e=4.0,
             reward_clip=1.0, R_min_bpsHz=0.5, D_max_s=2.0 ** -10, qos_penalty=2.5)
EDGE_CAP = BASE["f_edge_max"] * BASE["time_fast"]          # 2^21 cycles
CLEAR_SHARE = 0.48828125                                   # cap == bc at B = 2 kbit
ARRIVAL_KBIT = BASE["time_fast"] * 1000.0                  # 0.9765625

# the edges a case may sit on; every OTHER edge of a case is asserted far away (tests/test_step_edges_host.py)
EDGES = ("rate", "delay", "s", "clip", "clear", "queue", "tie")


def dyadic_params(**over) -> orc.OracleParams:
    p = orc.OracleParams()
    for k, v in BASE.items():
        setattr(p, k, v)
    p.qos_enable = True
    p.rate = 1.0
    for k, v in over.items():
        setattr(p, k, v)
    return p


def f32_next(x, n=1):
    """the float32 n steps above (n < 0: below) the float32 x"""
    x = np.float32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return float(x)


@dataclasses.dataclass
class Case:
    name: str
    data_buf0: np.ndarray            # [n, V] kbit
    mec_q0: np.ndarray               # [n] cycles
    gain: np.ndarray                 # [n, V]
    action: np.ndarray               # [n, 2, V]
    partner: np.ndarray              # [n, V]
    n_groups: np.ndarray             # [n]
    arrivals: np.ndarray             # [n, V]
    over: Dict[str, float] = dataclasses.field(default_factory=dict)       # parameter overrides on the dyadic base
    on: frozenset = frozenset()                                            # the edges (of EDGES) the case sits on
    # outputs the device must return bit for bit as the float32 image of the oracle's: key -> bool mask ([n, V]; [n] for
    # mec_q and viol); keys: data_p, mec_q, data_buf, reward, rate, viol (metrics slot 11 = count / V)
    exact: Dict[str, np.ndarray] = dataclasses.field(default_factory=dict)
    # values the oracle must return exactly: key -> float64 array, NaN where nothing is claimed (keys of the oracle's dict,
    # plus "util" = metrics slot 9)
    expect: Dict[str, np.ndarray] = dataclasses.field(default_factory=dict)
    meta: Dict[str, np.ndarray] = dataclasses.field(default_factory=dict)

    @property
    def n(self) -> int:
        return self.data_buf0.shape[0]

    def inputs(self):
        return (self.data_buf0, self.mec_q0, self.gain, self.action, self.partner, self.n_groups, self.arrivals)


def _filler(V, n=1):
    """n envs of an ordinary state, far from every edge: V singles, a backlog the CPU cannot clear, some offloading."""
    v = np.arange(V, dtype=np.float64)
    one = np.ones((n, 1))
    return dict(data_buf0=one * (3.0 + 0.25 * v), mec_q0=np.zeros(n), gain=one * (NOISE * (9.0 + 2.0 * v)),
                action=np.ones((n, 1, 1)) * np.stack([np.full(V, 0.25), np.full(V, 0.25)]),
                partner=np.full((n, V), SINGLE, dtype=np.int64), n_groups=np.full(n, V, dtype=np.int64),
                arrivals=(one * (v % 3)).astype(np.int64))


def _case(name, V, n=1, over=None, on=()):
    return Case(name=name, over=dict(over or {}), on=frozenset(on), **_filler(V, n))


def _mask(c, key, sel=None):
    shape = (c.n,) if key in ("mec_q", "viol") else c.data_buf0.shape
    m = c.exact.setdefault(key, np.zeros(shape, dtype=bool))
    if sel is None:
        m[...] = True
    else:
        m[sel] = True


def _claim(c, key, sel, value):
    shape = (c.n,) if key in ("mec_q", "util", "global_reward") else c.data_buf0.shape
    e = c.expect.setdefault(key, np.full(shape, np.nan))
    e[sel] = value
    if key in ("data_p", "mec_q", "data_buf", "reward"):
        _mask(c, key, sel)
    if key == "vehicle_rate":
        _mask(c, "rate", sel)


def _pair(c, e, first, second):
    c.partner[e, first] = second
    c.partner[e, second] = first + SECOND


def ordinary(V, over=None, name="ordinary"):
    """The state of the one-field-at-a-time cases: every field of the parameter set moves some output.  A pair (0, 1)
    whose far user's rate lies between the two R_min values, a last vehicle that is a single with no power and no CPU share
    of its own (rate 0: a QoS violation, the floor decides its CPU), the vehicles between them in no group, and a queue
    the edge cannot drain in one step."""
    c = _case(name, V, 1, over)
    c.partner[0, 2:V - 1] = NONE
    _pair(c, 0, 0, 1)
    c.action[0, :, V - 1] = 0.0
    c.n_groups[0] = 2
    c.mec_q0[0] = 3.0 * 2.0 ** 19
    _mask(c, "viol")
    return c


def cases(V: int) -> List[Case]:
    assert V >= 3
    out: List[Case] = []

    # ---- local clear: cap == bc, one float below, one float above (vehicle 0; ENV:585-592)
    c = _case("clear", V, 3, on=("clear",))
    c.data_buf0[:, 0] = 2.0
    c.arrivals[:, 0] = 3
    c.action[:, 1, 0] = [CLEAR_SHARE, f32_next(CLEAR_SHARE, -1), f32_next(CLEAR_SHARE, +1)]
    for e in (0, 2):
        _claim(c, "data_p", (e, 0), 2.0)
        _claim(c, "data_buf", (e, 0), 3 * ARRIVAL_KBIT)           # 2.9296875: nothing left, nothing offloaded
    out.append(c)

    # ---- empty env (everything 0; rate 0 < R_min: the reward is the penalty), and with both QoS thresholds at 0
    for name, over, on, rew in (("empty", {}, (), -BASE["qos_penalty"]),
                                ("empty/R_min=D_max=0", dict(R_min_bpsHz=0.0, D_max_s=0.0), ("rate", "delay"), 0.0)):
        c = _case(name, V, 1, over, on)
        c.data_buf0[:] = 0; c.gain[:] = 0; c.action[:] = 0; c.arrivals[:] = 0
        for key in ("data_p", "data_t", "data_buf", "vehicle_rate", "over_power", "delay"):
            _claim(c, key, np.s_[:], 0.0)
        _claim(c, "reward", np.s_[:], rew)
        _claim(c, "mec_q", np.s_[:], 0.0)
        _claim(c, "util", np.s_[:], 0.0)
        _claim(c, "global_reward", np.s_[:], rew)
        _mask(c, "viol")
        out.append(c)

    # ---- MEC queue: Q0 one float below, at, one float above what the edge serves in a step (ENV:604-610)
    q = [f32_next(EDGE_CAP, -1), EDGE_CAP, EDGE_CAP + 0.25]
    assert q[0] == EDGE_CAP - 0.125 and f32_next(EDGE_CAP, +1) == q[2]
    c = _case("queue/idle", V, 3, on=("queue",))                  # nobody in a group: nothing offloaded
    c.partner[:] = NONE
    c.n_groups[:] = 0
    c.mec_q0[:] = q
    _claim(c, "mec_q", np.s_[:], [0.0, 0.0, 0.25])
    _claim(c, "util", np.s_[:], [1.0 - 2.0 ** -24, 1.0, 1.0])
    _claim(c, "vehicle_rate", np.s_[:], 0.0)
    _mask(c, "viol")
    out.append(c)
    c = _case("queue/offload", V, 3)                              # with offload on top the queue is far past the edge
    c.mec_q0[:] = q
    out.append(c)

    # ---- NOMA (ENV:331-372); vehicles 0 and 1 unless said otherwise, the rest singles
    c = _case("noma/tie", V, 3, on=("tie",))                      # exact ties: 0 listed first, 0 listed second, two zero gains
    c.n_groups[:] = V - 1
    _pair(c, 0, 0, 1); _pair(c, 1, 1, 0); _pair(c, 2, 0, 1)
    c.gain[:, 1] = c.gain[:, 0]
    c.gain[2, :2] = 0.0
    _claim(c, "vehicle_rate", (2, slice(0, 2)), 0.0)
    out.append(c)
    c = _case("noma/ratio", V, 5)
    c.n_groups[:] = V - 1
    for e in range(5):
        _pair(c, e, 0, 1)
    c.gain[0, :2] = [NOISE * 2.0 ** 10, NOISE * 2.0 ** -10]       # gain ratios of 2^20 both ways
    c.gain[1, :2] = [NOISE * 2.0 ** -10, NOISE * 2.0 ** 10]
    c.action[2, 0, 1] = 0.0                                       # a partner whose power is 0 (listed second)
    c.action[3, 0, 0] = 0.0                                       # ... listed first
    _claim(c, "vehicle_rate", (2, 1), 0.0)
    _claim(c, "vehicle_rate", (3, 0), 0.0)
    c.partner[4, :2] = SINGLE                                     # a pair that includes vehicle V-1, listed second ...
    _pair(c, 4, 0, V - 1)
    out.append(c)
    c = _case("noma/last+dropped", V, 2)
    _pair(c, 0, V - 1, 1)                                         # ... and listed first
    c.n_groups[0] = V - 1
    _pair(c, 1, 0, 1)                                             # dropped vehicles next to pairs
    c.partner[1, 2] = NONE
    if V >= 5:
        _pair(c, 1, 3, 4)
        c.partner[1, 5:] = NONE
    c.n_groups[1] = V - 2 if V < 5 else 2                          # V = 4: vehicle 3 is still a single
    _claim(c, "vehicle_rate", (1, 2), 0.0)
    if V > 5:
        _claim(c, "vehicle_rate", (1, slice(5, V)), 0.0)
    _mask(c, "viol")
    out.append(c)
    c = _case("noma/n_groups", V, 3)                              # n_groups of 0, 1 and V with every vehicle a single
    c.n_groups[:] = [0, 1, V]
    out.append(c)

    # ---- projection and shares (ENV:555-561, 572-580), vehicle 0
    c = _case("proj/s==1", V, 2, on=("s",))                       # s = 0.5 a0 + 0.5 a1: exactly 1, and the next float above
    c.action[0, :, 0] = [1.0, 1.0]
    c.action[1, :, 0] = [1.0 + 2.0 ** -22, 1.0]
    out.append(c)
    c = _case("proj/shares", V, 6)
    c.action[0, :, 0] = [-0.5, -0.25]                             # negative actions: no power, the floor's CPU
    _claim(c, "vehicle_rate", (0, 0), 0.0)
    c.action[1, :, 0] = [0.25, 1.5]                               # a1 > 1: the share clips, the power does not (s = 0.875)
    c.action[2, :, 0] = [0.5, 2.0]                                # ... and with s = 1.25 the projection runs
    fl = BASE["cpu_share_floor"]
    c.action[3:, 1, 0] = [f32_next(fl, -1), fl, f32_next(fl, +1)]  # a1 below, at and above the floor
    out.append(c)

    # ---- parameter branches
    for fl in (float("nan"), float("inf"), -1.0, 0.0, 0.95, 2.0):  # ENV:574-577: 0.10, 0.10, 0, 0, 0.95, 0.95
        c = _case("floor=%r" % fl, V, 1, dict(cpu_share_floor=fl))
        c.data_buf0[0, 0] = 2.0
        c.action[0, :, 0] = 0.0                                   # the floor's CPU, and nothing offloaded
        c.action[0, 1, 1] = 0.5
        if orc.effective_floor(fl) == 0.0:                        # no CPU at all: a delay of 5e17 s, the clip's reward
            _claim(c, "reward", (0, 0), -BASE["reward_clip"])
            _claim(c, "data_p", (0, 0), 0.0)
        out.append(c)
    c = _case("qos_enable=False", V, 1, dict(qos_enable=False))   # rates of 0 and no penalty
    c.partner[:] = NONE
    c.n_groups[:] = 0
    _claim(c, "vehicle_rate", np.s_[:], 0.0)
    _mask(c, "viol")
    out.append(c)
    c = _case("reward_clip=2^-3", V, 1, dict(reward_clip=0.125))  # a heavy backlog: the reward is -clip exactly
    c.data_buf0[:] = 200.0 + np.arange(V)
    c.action[0, 1, :] = 0.0
    _claim(c, "reward", np.s_[:], -0.125)
    _claim(c, "global_reward", np.s_[:], -0.125)
    _mask(c, "viol")
    out.append(c)
    c = _case("reward_clip=0", V, 1, dict(reward_clip=0.0))
    _claim(c, "reward", np.s_[:], 0.0)
    _claim(c, "global_reward", np.s_[:], 0.0)
    out.append(c)

    # ---- one field at a time, on an ordinary state
    out.append(ordinary(V))
    for k in BASE:
        out.append(ordinary(V, {k: OTHER[k]}, "field/%s" % k))

    # ---- log2_1p: pw0 == 1 and gain = x 2^-46, so the SINR is exactly x; singles, n_groups = 1
    xs = [2.0 ** k for k in range(-40, 41)] + [f32_next(0.0625, k) for k in range(-8, 9)]
    n = (len(xs) + V - 1) // V
    x = np.ones(n * V)
    x[:len(xs)] = xs
    c = _case("log2_1p", V, n)
    c.data_buf0[:] = 1.0
    c.action[:, 0, :] = 1.0
    c.action[:, 1, :] = 0.5
    c.n_groups[:] = 1
    c.gain[:] = (x * NOISE).reshape(n, V)
    c.meta["x"] = x.reshape(n, V)
    c.meta["at_switch"] = (np.arange(n * V) >= 81).reshape(n, V) & (np.arange(n * V) < len(xs)).reshape(n, V)
    out.append(c)
    return out


@dataclasses.dataclass
class Batch:
    params: orc.OracleParams
    over: Dict[str, float]
    cases: List[Case]
    slices: List[slice]
    data_buf0: np.ndarray
    mec_q0: np.ndarray
    gain: np.ndarray
    action: np.ndarray
    partner: np.ndarray
    n_groups: np.ndarray
    arrivals: np.ndarray

    @property
    def E(self) -> int:
        return self.data_buf0.shape[0]

    def inputs(self):
        return (self.data_buf0, self.mec_q0, self.gain, self.action, self.partner, self.n_groups, self.arrivals)

    def oracle(self):
        return orc.step(*self.inputs(), self.params)

    def mask(self, key):
        """the cases' `exact[key]` masks, concatenated"""
        shape = (self.E,) if key in ("mec_q", "viol") else self.data_buf0.shape
        m = np.zeros(shape, dtype=bool)
        for c, sl in zip(self.cases, self.slices):
            if key in c.exact:
                m[sl] = c.exact[key]
        return m


def batches(V: int, table=None) -> List[Batch]:
    """The cases grouped by parameter set, in table order (the base set first)."""
    groups: Dict[str, List[Case]] = {}
    for c in (table if table is not None else cases(V)):
        groups.setdefault(repr(sorted(c.over.items())), []).append(c)
    out = []
    for cs in groups.values():
        slices, lo = [], 0
        for c in cs:
            slices.append(slice(lo, lo + c.n))
            lo += c.n
        cat = {k: np.concatenate([getattr(c, k) for c in cs]) for k in
               ("data_buf0", "mec_q0", "gain", "action", "partner", "n_groups", "arrivals")}
        out.append(Batch(params=dyadic_params(**cs[0].over), over=cs[0].over, cases=cs, slices=slices, **cat))
    return out


def _rel(a, b):
    """|a - b| relative to the larger magnitude; 0 where both are 0 (the sample sits on the edge)"""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    big = np.maximum(np.abs(a), np.abs(b))
    return np.where(big > 0, np.abs(a - b) / np.where(big > 0, big, 1.0), 0.0)


def edge_distances(o, inputs, p) -> Dict[str, np.ndarray]:
    """Relative distance of every sample to every discontinuity of step(): the oracle's own `margin` entries (the two QoS
    thresholds, the s > 1 projection, the reward clip) and the three it does not list (local clear cap >= bc, the MEC
    queue min(edge_cap, Q), the near / far tie)."""
    B, Q0, gain, action, partner, n_groups, _ = inputs
    m = o["margin"]
    d = {}
    if p.qos_enable:
        d["rate"] = _rel(o["vehicle_rate"], p.R_min_bpsHz)
        d["delay"] = _rel(o["delay"], p.D_max_s)
    d["s"] = np.abs(m["s"])
    d["clip"] = _rel(np.abs(m["raw_reward"]), p.reward_clip)
    cpu = np.maximum(np.clip(action[:, 1, :], 0.0, 1.0), orc.effective_floor(p.cpu_share_floor))
    d["clear"] = _rel(cpu * p.f_local_max * p.time_fast, B * 1000.0 * p.cycles_per_bit)
    d["queue"] = _rel(Q0 + o["ein_sum"], p.f_edge_max * p.time_fast)[:, None] * np.ones_like(B)
    pidx = np.where(partner >= 0, partner % SECOND, 0)
    gp = np.take_along_axis(gain, pidx, axis=1)
    d["tie"] = np.where(partner >= 0, _rel(gp, gain), 1.0)
    return d
