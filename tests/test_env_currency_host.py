"""What `VecEnviron` tells the kernels about theta, its candidate indices and h_r -- on the host, no GPU and no built
library: a recording stand-in takes the place of librisvec.so, the env lives on the CPU (tensor `_version` counters work
there too), and every launch's flag word is compared with a literal composed from the `N.STEP_*` / `N.BCD_*` names.
Only the public API of `VecEnviron` and the `compat` facade is used, plus what the stand-in saw: no private field is
read, so the file pins the behaviour, not the bookkeeping behind it.  A wrong bit makes a kernel read stale bytes without
any error; this is where such a bit shows in seconds."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ris_vec_marl_amd import _native as N  # noqa: E402
from ris_vec_marl_amd import VecEnviron, reference_lanes  # noqa: E402
from ris_vec_marl_amd.compat import Environ  # noqa: E402
from ris_vec_marl_amd.replay import VecReplayBuffer  # noqa: E402

E, V = 4, 8
CPU = torch.device("cpu")

BASE = N.STEP_METRICS | N.STEP_POWER_W | N.STEP_OBS
IDX = N.STEP_THETA_IDX_CURRENT
ROWS = N.STEP_H_R_STEER_CURRENT | N.STEP_STEER_HEADS_CURRENT
BYI = N.STEP_THETA_BY_INDEX
RC, RS, RI = N.STEP_REUSE_COLSUM, N.STEP_REUSE_SSUM, N.STEP_REUSE_IDX
BRC, BRS, BRI, BNT = N.BCD_REUSE_COLSUM, N.BCD_REUSE_SSUM, N.BCD_REUSE_IDX, N.BCD_NO_THETA

# where each entry point takes its flag word
FLAG_POS = {"risvec_step": 8, "risvec_step_fused": 8, "risvec_step_fused_bcd": 8, "risvec_step_ring": 9,
            "risvec_step_fused_multi": 9, "risvec_step_multi": 9, "risvec_step_fused_3gpp": 11,
            "risvec_step_fused_3gpp_multi": 13, "risvec_bcd": 3, "risvec_sarl_step": 7, "risvec_sarl_rollout": 6}
QUIET = ("risvec_reset", "risvec_mobility", "risvec_theta_by_index_supported")       # no part of any expectation

FUSED, SWEEP, CACHED, RING = "risvec_step_fused", "risvec_step_fused_bcd", "risvec_step", "risvec_step_ring"
FROM_INDEX, HEADS, GEOMETRY = ("risvec_theta_from_index", None), ("risvec_steer_heads", None), ("risvec_geometry", None)


class Recorder:
    """Stands in for the ctypes handle of librisvec.so: every entry point exists, records (name, args), returns 0
    (1 for risvec_theta_by_index_supported)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("risvec_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return 1 if name == "risvec_theta_by_index_supported" else 0

        self.__dict__[name] = entry
        return entry

    def take(self):
        """[(entry point, flag word or None)] of the calls since the last take()."""
        out = [(n, a[FLAG_POS[n]] if n in FLAG_POS else None) for n, a in self.calls if n not in QUIET]
        del self.calls[:]
        return out


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(N, "load", lambda: r)
    monkeypatch.setattr(N, "require_hip", lambda device: None)
    monkeypatch.setattr(N, "stream", lambda device: 0)
    return r


class Rig:
    """An env at (E, V, M, control_bit) after the anchors' setup, with fixed step inputs."""

    def __init__(self, rec, M=64, control_bit=3, lazy=False, setup=True):
        L = reference_lanes()
        self.rec, self.M = rec, M
        self.env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, control_bit,
                              n_envs=E, device="cpu", seed=1, lazy_theta=lazy)
        self.act = torch.zeros(E, 2, V)
        self.partner = torch.full((E, V), -1, dtype=torch.int32)
        self.ng = torch.full((E,), V, dtype=torch.int32)
        if setup:
            self.env.make_new_game()
            self.env.renew_positions()
            self.env.compute_parms()
            self.env.Random_phase()
            rec.take()

    def step(self, **kw):
        """One step(); the calls it made."""
        self.env.step(self.act, self.partner, self.ng, **kw)
        return self.rec.take()

    def fused(self):
        return self.step(fused=True)

    def sweep(self):
        return self.step(bcd=True)

    def sweeps(self, n):
        for _ in range(n):
            self.sweep()

    def did(self, call, *args, **kw):
        """The calls a method of the env made."""
        getattr(self.env, call)(*args, **kw)
        return self.rec.take()

    def ring(self, **kw):
        """A bound step-with-store launcher on a replay buffer of the CPU."""
        rb = VecReplayBuffer(64, 5, V + 2, V, device="cpu")
        launch = self.env.bind_step_store(rb, torch.zeros(E, V, 2), self.partner, self.ng, torch.zeros(E, V, V), power_w=True,
                                          **kw)
        self.rec.take()
        return launch


def swept(rec, n=2, **kw):
    """A rig after n sweep + step launches: column sums, the sweep sum and the indices are all current; with lazy_theta
    and n >= 2 theta is held by index (the complex64 tensor lags)."""
    r = Rig(rec, **kw)
    r.sweeps(n)
    return r


# ---------------------------------------------------------------------------------------------------- the anchors
def test_anchor_eager(rec):
    r = Rig(rec)
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]
    assert r.sweep() == [(SWEEP, BASE | RC)]
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI)]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]
    r.env.tensors["h_r"].add_(0)
    assert r.fused() == [(FUSED, BASE | IDX)]
    assert r.did("invalidate_colsum") == []
    assert r.sweep() == [(SWEEP, BASE)]
    r.env.compute_parms()
    r.sweeps(2)
    rec.take()
    sd = r.env.state_dict()
    assert rec.take() == []
    assert r.did("load_state_dict", sd) == [HEADS]
    assert r.fused() == [(FUSED, BASE | ROWS)]
    assert r.sweep() == [(SWEEP, BASE)]                      # a checkpoint carries no column sums


def test_anchor_step_store(rec):
    r = Rig(rec)
    launch = r.ring(fused=True)
    launch()
    assert rec.take() == [(RING, BASE | N.STEP_POLICY_ACTION | IDX | ROWS)]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]
    r.env.tensors["h_r"].add_(0)
    launch()
    assert rec.take() == [(RING, BASE | N.STEP_POLICY_ACTION | IDX)]
    cached = r.ring(fused=False)
    cached()
    assert rec.take() == [(RING, BASE | N.STEP_POLICY_ACTION)]


def test_anchor_lazy(rec):
    r = Rig(rec, lazy=True)
    assert r.fused() == [(FUSED, BASE)]
    assert r.sweep() == [(SWEEP, BASE | RC)]
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI | BYI)]
    assert r.fused() == [(FUSED, BASE | BYI)]
    r.env.tensors
    assert rec.take() == [FROM_INDEX]
    r.env.tensors
    assert rec.take() == []
    assert r.fused() == [(FUSED, BASE | BYI)]
    assert r.did("invalidate_colsum") == []
    assert r.sweep() == [(SWEEP, BASE)]
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI | BYI)]


# ---------------------------------------------------------------------------------------------------- the shapes
def test_rows_that_are_no_whole_chunks(rec):
    """M = 36: no rebuilding kernel, so no h_r bits, no chunk heads and no `steer_head` tensor; the index bit is sent."""
    r = Rig(rec, M=36, setup=False)
    r.env.make_new_game()
    r.env.renew_positions()
    assert r.did("compute_parms") == [GEOMETRY]
    assert "steer_head" not in r.env.tensors and "steer_ang" in r.env.tensors
    r.env.Random_phase()
    rec.take()
    assert r.fused() == [(FUSED, BASE | IDX)]
    assert r.sweep() == [(SWEEP, BASE | RC)]
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI)]
    assert r.fused() == [(FUSED, BASE | IDX)]
    launch = r.ring(fused=True)
    launch()
    assert rec.take() == [(RING, BASE | N.STEP_POLICY_ACTION | IDX)]
    assert r.did("load_state_dict", r.env.state_dict()) == []
    assert r.fused() == [(FUSED, BASE)]
    lz = swept(rec, 2, M=36, lazy=True)
    assert lz.fused() == [(FUSED, BASE | BYI)]


@pytest.mark.parametrize("lazy", [False, True])
def test_control_bit_2_has_no_index_forms(rec, lazy):
    """2^b != 8: Random_phase and the sweeps leave no indices; the h_r bits do not depend on that (eager only)."""
    rows = 0 if lazy else ROWS
    r = Rig(rec, control_bit=2, lazy=lazy)
    assert r.fused() == [(FUSED, BASE | rows)]
    assert r.sweep() == [(SWEEP, BASE | RC)]
    assert r.sweep() == [(SWEEP, BASE | RC | RS)]
    assert r.sweep() == [(SWEEP, BASE | RC | RS)]
    assert r.fused() == [(FUSED, BASE | rows)]
    assert r.did("optimize_phase_shift") == [("risvec_bcd", BRC | BRS)]
    r.env.tensors
    assert rec.take() == []
    assert r.did("Random_phase") == [("risvec_random_phase", None)]
    assert r.fused() == [(FUSED, BASE | rows)]
    assert r.sweep() == [(SWEEP, BASE | RC)]


def test_step_setup_is_at_the_anchor_shape(rec):
    r = Rig(rec, setup=False)
    r.env.make_new_game()
    r.env.renew_positions()
    assert rec.take() == []
    assert r.did("compute_parms") == [GEOMETRY, HEADS]
    assert "steer_head" in r.env.tensors


# ---------------------------------------------------------------------------------------------------- writers of theta
def test_random_phase(rec):
    r = swept(rec)
    assert r.did("Random_phase") == [("risvec_random_phase", None)]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]         # with 2^b = 8 the kernel writes the indices too
    assert r.sweep() == [(SWEEP, BASE | RC)]                 # ... but the sweep re-derives its own
    lz = swept(rec, 3, lazy=True)
    assert lz.did("Random_phase") == [("risvec_random_phase", None)]
    assert lz.fused() == [(FUSED, BASE)]
    lz.env.tensors
    assert rec.take() == []                                  # the written tensor is theta: nothing to materialise


def test_get_next_phase(rec):
    r = swept(rec)
    assert r.did("get_next_phase", torch.zeros(E, r.M)) == [("risvec_set_phase", None)]
    assert r.fused() == [(FUSED, BASE | ROWS)]
    assert r.sweep() == [(SWEEP, BASE | RC)]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]
    lz = swept(rec, 3, lazy=True)
    lz.env.get_next_phase(torch.zeros(E, lz.M))
    rec.take()
    assert lz.fused() == [(FUSED, BASE)]
    lz.env.tensors
    assert rec.take() == []


def test_sarl_step(rec):
    r = swept(rec)
    r.env.sarl_step(r.act)                                   # no phase: theta stays
    assert rec.take() == [("risvec_sarl_step", N.STEP_OBS)]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI)]
    r.env.sarl_step(r.act, torch.zeros(E, r.M))
    assert rec.take() == [("risvec_sarl_step", N.STEP_OBS)]
    assert r.fused() == [(FUSED, BASE | ROWS)]
    assert r.sweep() == [(SWEEP, BASE | RC)]


def test_sarl_rollout(rec):
    r = swept(rec)
    r.env.sarl_rollout(torch.zeros(E, 2 * V + r.M))
    assert rec.take() == [("risvec_sarl_rollout", N.STEP_OBS)]
    assert r.fused() == [(FUSED, BASE | ROWS)]
    assert r.sweep() == [(SWEEP, BASE | RC)]
    lz = swept(rec, 3, lazy=True)
    lz.env.sarl_rollout(torch.zeros(E, 2 * V + lz.M))
    assert rec.take() == [("risvec_sarl_rollout", N.STEP_OBS)]       # theta is an output of this launch
    lz.env.tensors
    assert rec.take() == []
    assert lz.fused() == [(FUSED, BASE)]


def test_stand_alone_sweep(rec):
    r = Rig(rec)
    assert r.did("optimize_phase_shift") == [("risvec_bcd", BRC)]
    assert r.did("optimize_phase_shift") == [("risvec_bcd", BRC | BRS | BRI)]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI)]
    assert r.did("optimize_phase_shift", return_idx=True) == [("risvec_bcd", BRC | BRS | BRI)]
    lz = Rig(rec, lazy=True)
    assert lz.did("optimize_phase_shift") == [("risvec_bcd", BRC)]
    assert lz.did("optimize_phase_shift") == [("risvec_bcd", BRC | BRS | BRI | BNT)]
    assert lz.fused() == [(FUSED, BASE | BYI)]
    assert lz.sweep() == [(SWEEP, BASE | RC | RS | RI | BYI)]
    lz.env.tensors
    assert rec.take() == [FROM_INDEX]
    assert lz.did("optimize_phase_shift") == [("risvec_bcd", BRC | BRS | BRI | BNT)]
    lz.env.tensors
    assert rec.take() == [FROM_INDEX]


def test_facade_setter(rec):
    L = reference_lanes()
    env = Environ(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, 64, 3, device="cpu", seed=1)
    env.make_new_game()
    env.renew_positions()
    env.compute_parms()
    env.Random_phase()
    rec.take()
    env.optimize_phase_shift()
    env.optimize_phase_shift()
    assert rec.take() == [("risvec_bcd", BRC), ("risvec_bcd", BRC | BRS | BRI)]
    env.elements_phase_shift_complex = np.ones(64)
    assert rec.take() == []
    env.optimize_phase_shift()
    env.optimize_phase_shift()
    assert rec.take() == [("risvec_bcd", BRC), ("risvec_bcd", BRC | BRS | BRI)]


def test_unannounced_theta_write(rec):
    """A torch write moves the tensor's version: the index bit goes at once.  The sweeps hear of it through
    invalidate_theta() only."""
    r = swept(rec)
    r.env.tensors["theta"].add_(0)
    assert r.fused() == [(FUSED, BASE | ROWS)]
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI)]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]         # the sweep wrote both again
    r.env.tensors["theta"].add_(0)
    assert r.did("invalidate_theta") == []
    assert r.fused() == [(FUSED, BASE | ROWS)]
    assert r.sweep() == [(SWEEP, BASE | RC)]


# ------------------------------------------------------------------------------------- writers of h_r and the angles
def test_compute_parms_and_rebuild_colsum(rec):
    r = swept(rec)
    assert r.did("compute_parms") == [GEOMETRY, HEADS]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]
    assert r.sweep() == [(SWEEP, BASE | RC | RI)]            # c changed: the sweep sum is re-summed, the indices hold
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI)]
    assert r.did("rebuild_colsum") == [("risvec_colsum", None)]
    assert r.fused() == [(FUSED, BASE | IDX)]                # announced: h_r was written by hand
    assert r.sweep() == [(SWEEP, BASE | RC | RI)]
    assert r.did("compute_parms") == [GEOMETRY, HEADS]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]


def test_invalidate_colsum(rec):
    r = swept(rec)
    assert r.did("invalidate_colsum") == []
    assert r.fused() == [(FUSED, BASE)]
    assert r.sweep() == [(SWEEP, BASE)]
    assert r.fused() == [(FUSED, BASE | IDX)]
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI)]
    assert r.did("compute_parms") == [GEOMETRY, HEADS]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]


def test_torch_writes_to_h_r_and_the_angles(rec):
    r = swept(rec)
    r.env.tensors["steer_ang"].add_(0)
    assert r.fused() == [(FUSED, BASE | IDX | N.STEP_H_R_STEER_CURRENT)]      # the heads bit goes, the h_r bit stays
    assert r.did("compute_parms") == [GEOMETRY, HEADS]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]
    r.env.phases_R_i.mul_(1)                                  # the complex view shares the version counter
    assert r.fused() == [(FUSED, BASE | IDX)]
    assert r.sweep() == [(SWEEP, BASE | RC | RI)]            # (compute_parms above reset the sweep sum)
    assert r.step(fused=True, steer=True) == [(FUSED, BASE | N.STEP_STEER)]   # steer=True hears announcements only


def test_steer_heads_switch(rec):
    r = Rig(rec)
    r.env.steer_heads = False
    assert r.fused() == [(FUSED, BASE | IDX | N.STEP_H_R_STEER_CURRENT)]
    launch = r.ring(fused=True)
    launch()
    assert rec.take() == [(RING, BASE | N.STEP_POLICY_ACTION | IDX | N.STEP_H_R_STEER_CURRENT)]
    r.env.steer_heads = True
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]


# ----------------------------------------------------------------------- announcements while theta is held by index
@pytest.mark.parametrize("announce,after", [("invalidate_colsum", BASE), ("invalidate_theta", BASE | RC)])
@pytest.mark.parametrize("theta_written", [False, True])
def test_announcement_while_theta_is_held_by_index(rec, announce, after, theta_written):
    """h_r is written through a reference taken before the sweeps and the write announced while the complex64 theta lags
    behind the indices.  Theta not written: the swept theta must be materialised before the indices are dropped.
    Theta written through torch: the written tensor wins, nothing is materialised."""
    r = Rig(rec, lazy=True)
    h_r, theta = r.env.tensors["h_r"], r.env.tensors["theta"]
    r.sweeps(3)
    assert rec.take() == []
    h_r.add_(0)
    if theta_written:
        theta.add_(0)
    assert r.did(announce) == ([] if theta_written else [FROM_INDEX])
    assert r.sweep() == [(SWEEP, after)]
    r.env.tensors
    assert rec.take() == []
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI | BYI)]


# ---------------------------------------------------------------------------------------------------- the sweep sum
@pytest.mark.parametrize("lazy", [False, True])
def test_sweep_sum_is_refreshed_every_64_sweeps(rec, lazy):
    r = Rig(rec, lazy=lazy)
    byi = BYI if lazy else 0
    for k in range(1, 67):
        want = BASE | RC if k == 1 else BASE | RC | RI | byi | (0 if k == 65 else RS)
        assert r.sweep() == [(SWEEP, want)], k
    r.env.tensors
    assert rec.take() == ([FROM_INDEX] if lazy else [])


def test_reuse_colsum_override(rec):
    r = swept(rec)
    assert r.did("optimize_phase_shift", reuse_colsum=False) == [("risvec_bcd", BRI)]        # no column sums, no sweep sum
    assert r.did("optimize_phase_shift") == [("risvec_bcd", BRC | BRS | BRI)]
    r.env.invalidate_colsum()
    assert r.did("optimize_phase_shift", reuse_colsum=True) == [("risvec_bcd", BRC)]
    r.env.invalidate_colsum()
    assert r.did("optimize_phase_shift") == [("risvec_bcd", 0)]
    lz = swept(rec, 3, lazy=True)
    assert lz.did("optimize_phase_shift", reuse_colsum=False) == [("risvec_bcd", BRI | BNT)]


# -------------------------------------------------------------------------- consumers of the complex64 tensor
def test_consumers_materialise_a_lagging_theta(rec):
    multi = N.STEP_METRICS | N.STEP_OBS
    r = swept(rec, 3, lazy=True)
    assert r.did("update_channel_gains") == [FROM_INDEX, ("risvec_gain", None)]
    assert r.did("update_channel_gains") == [("risvec_gain", None)]

    r = swept(rec, 3, lazy=True)
    r.env.step_many(r.act[None], r.partner, r.ng, fused=True)
    assert rec.take() == [FROM_INDEX, ("risvec_step_fused_multi", multi)]
    r.env.step_many(r.act[None], r.partner, r.ng, fused=True)
    assert rec.take() == [("risvec_step_fused_multi", multi)]

    r = swept(rec, 3, lazy=True)
    r.env.sarl_step(r.act)
    assert rec.take() == [FROM_INDEX, ("risvec_sarl_step", N.STEP_OBS)]

    r = swept(rec, 3, lazy=True)
    sd = r.env.state_dict()
    assert rec.take() == [FROM_INDEX]
    assert r.fused() == [(FUSED, BASE | BYI)]                # the indices stay current
    assert r.did("load_state_dict", sd) == [HEADS]
    assert r.fused() == [(FUSED, BASE)]

    r = swept(rec, 3, lazy=True)
    launch = r.ring(fused=True)
    assert rec.take() == []
    launch()
    assert rec.take() == [FROM_INDEX, (RING, BASE | N.STEP_POLICY_ACTION)]       # no bit of any kind under lazy_theta
    launch()
    assert rec.take() == [(RING, BASE | N.STEP_POLICY_ACTION)]


def test_cached_steps_leave_a_lagging_theta_alone(rec):
    r = swept(rec, 3, lazy=True)
    assert r.step(fused=False) == [(CACHED, BASE)]
    r.env.step_many(r.act[None], r.partner, r.ng, fused=False)
    assert rec.take() == [("risvec_step_multi", N.STEP_METRICS | N.STEP_OBS)]
    cached = r.ring(fused=False)
    cached()
    assert rec.take() == [(RING, BASE | N.STEP_POLICY_ACTION)]
    r.env.tensors
    assert rec.take() == [FROM_INDEX]


# ---------------------------------------------------------------------------------------------------- steer=True
def test_steer_form_is_refused_without_a_steering_base(rec):
    r = Rig(rec, setup=False)
    r.env.make_new_game()
    with pytest.raises(ValueError, match="steering vectors"):
        r.step(fused=True, steer=True)
    r.env.compute_parms()
    rec.take()
    assert r.step(fused=True, steer=True) == [(FUSED, BASE | N.STEP_STEER)]
    with pytest.raises(ValueError, match="fused=True"):
        r.step(steer=True)
    for announce in ("rebuild_colsum", "invalidate_colsum"):
        getattr(r.env, announce)()
        with pytest.raises(ValueError, match="steering vectors"):
            r.step(fused=True, steer=True)
        with pytest.raises(ValueError, match="steering vectors"):
            r.env.bind_step(r.act, r.partner, r.ng, fused=True, steer=True)
        r.env.compute_parms()
        rec.take()
        assert r.step(fused=True, steer=True) == [(FUSED, BASE | N.STEP_STEER)]
    lz = swept(rec, 3, lazy=True)
    assert lz.step(fused=True, steer=True) == [FROM_INDEX, (FUSED, BASE | N.STEP_STEER)]      # reads the complex64 theta


# ---------------------------------------------------------------------------------------------------- lazy_theta toggled
def test_lazy_theta_switched_off_while_theta_is_held_by_index(rec):
    r = swept(rec, 3, lazy=True)
    r.env.lazy_theta = False
    assert r.fused() == [FROM_INDEX, (FUSED, BASE)]
    assert r.fused() == [(FUSED, BASE | ROWS)]               # the by-index sweep left the tensor behind: no index bit
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI)]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]


def test_lazy_theta_switched_on_later(rec):
    r = swept(rec)
    r.env.lazy_theta = True
    assert r.fused() == [(FUSED, BASE | BYI)]
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI | BYI)]
    r.env.lazy_theta = False
    assert r.sweep() == [FROM_INDEX, (SWEEP, BASE | RC | RS | RI)]
    assert r.fused() == [(FUSED, BASE | IDX | ROWS)]


# ---------------------------------------------------------------------------------------------------- 3GPP channel models
@pytest.mark.parametrize("lazy", [False, True])
def test_3gpp_forms_send_none_of_the_bits(rec, lazy):
    F3 = "risvec_step_fused_3gpp"
    r = swept(rec, 3, lazy=lazy)
    r.env.channel_model = "3gpp_umi"
    assert r.fused() == [(F3, BASE)]
    nt = BNT if lazy else 0
    assert r.sweep() == [("risvec_bcd", BRC | BRS | BRI | nt), (F3, BASE)]
    launch = r.ring(fused=True)
    launch()
    assert rec.take() == [(F3, BASE | N.STEP_POLICY_ACTION)]
    r.env.step_many(r.act[None], r.partner, r.ng, fused=True)
    assert rec.take() == [("risvec_step_fused_3gpp_multi", N.STEP_METRICS | N.STEP_OBS)]
    assert r.step(fused=False) == [(CACHED, BASE)]
    r.env.channel_model = "free"
    byi = BYI if lazy else IDX | ROWS
    assert r.fused() == [(FUSED, BASE | byi)]


# ---------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_counters(rec):
    r = swept(rec)
    c = r.env.state_dict()["counters"]
    assert c["steer_valid"] is True and c["h_r_steer"] is True
    r.env.tensors["h_r"].add_(0)
    c = r.env.state_dict()["counters"]
    assert c["steer_valid"] is True and c["h_r_steer"] is False
    r.env.compute_parms()
    assert r.env.state_dict()["counters"]["h_r_steer"] is True
    r.env.invalidate_colsum()
    c = r.env.state_dict()["counters"]
    assert c["steer_valid"] is False and c["h_r_steer"] is False
    assert Rig(rec, setup=False).env.state_dict()["counters"]["h_r_steer"] is False


def test_checkpoint_round_trips(rec):
    r = swept(rec)
    sd = r.env.state_dict()
    rec.take()
    # with steer_ang: the rows can be rebuilt at once, the heads are recomputed from the loaded angles
    assert r.did("load_state_dict", sd) == [HEADS]
    assert r.fused() == [(FUSED, BASE | ROWS)]
    assert r.step(fused=True, steer=True) == [(FUSED, BASE | N.STEP_STEER)]
    assert r.sweep() == [(SWEEP, BASE)]
    assert r.sweep() == [(SWEEP, BASE | RC | RS | RI)]
    # without it: no h_r bits until the next compute_parms()
    old = {k: v for k, v in sd.items() if k != "steer_ang"}
    assert r.did("load_state_dict", old) == []
    assert r.fused() == [(FUSED, BASE)]
    assert r.step(fused=True, steer=True) == [(FUSED, BASE | N.STEP_STEER)]       # z_r is in every checkpoint
    assert r.did("compute_parms") == [GEOMETRY, HEADS]
    assert r.fused() == [(FUSED, BASE | ROWS)]
    # counters of a checkpoint from before the steering forms
    older = dict(sd, counters={k: v for k, v in sd["counters"].items() if k not in ("steer_valid", "h_r_steer")})
    assert r.did("load_state_dict", older) == [HEADS]
    assert r.fused() == [(FUSED, BASE)]
    with pytest.raises(ValueError, match="steering vectors"):
        r.step(fused=True, steer=True)
    assert r.did("compute_parms") == [GEOMETRY, HEADS]
    assert r.fused() == [(FUSED, BASE | ROWS)]
    # a checkpoint whose h_r had been written by hand
    r.env.tensors["h_r"].add_(0)
    assert r.did("load_state_dict", r.env.state_dict()) == [HEADS]
    assert r.fused() == [(FUSED, BASE)]
