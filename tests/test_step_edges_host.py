"""CPU tests of the step() edge-case table (tests/step_edge_cases.py) -- the table, not the kernel: every number in it is
a float32, the float64 oracle returns exactly what each case claims, every case is far from every discontinuity except the
one it is placed on, and `step_mask` (what the random step tests use to leave samples out) would leave out nothing but
those placed samples.  That last rule is what keeps tests/test_step_edges_hip.py, which masks nothing, from hiding
anything: a sample the mask does not flag is one the device and the oracle must agree on at the usual tolerance."""
import dataclasses

import numpy as np
import pytest

from oracle import risvec_oracle as orc
from tests import step_edge_cases as T

VS = [3, 5, 8, 16]
FAR = 1e-3


def step_mask(o, g_partner, gain, Q0):
    """tests/test_hip_parity.py::step_mask, restated (that module needs torch and a GPU to import); the GPU edge tests
    assert the two agree on the whole table."""
    m = o["margin"]
    near_qos = (np.abs(m["rate"]) < 2e-6 * np.maximum(1, np.abs(o["vehicle_rate"]))) | \
               (np.abs(m["delay"]) < 2e-6 * np.maximum(0.1, o["delay"]))
    noise_share = (o["ein_sum"] < 1e-3) & (o["ein_sum"] > 0) & (np.asarray(Q0) > 0)
    near_qos = near_qos | noise_share[:, None]
    near_proj = np.abs(m["s"]) < 1e-6
    pidx = np.where(g_partner >= 0, g_partner % (1 << 16), 0)
    gp = np.take_along_axis(gain, pidx, axis=1)
    near_tie = (g_partner >= 0) & (gp != gain) & (np.abs(gp - gain) < 1e-6 * gain)
    return near_qos, near_proj | near_tie


def _f32_exact(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return bool(np.all((x.astype(np.float32).astype(np.float64) == x) | np.isnan(x)))


@pytest.mark.parametrize("V", VS)
def test_every_input_and_parameter_is_a_float32(V):
    for c in T.cases(V):
        for k in ("data_buf0", "mec_q0", "gain", "action"):
            assert _f32_exact(getattr(c, k)), (c.name, k)
        assert c.partner.dtype == np.int64 and c.arrivals.dtype == np.int64 and c.n_groups.dtype == np.int64
        p = T.dyadic_params(**c.over)
        for k in T.BASE:
            # 0.95 is the reference's own clamp, not a field value, and a floor of 0.95 is the one non-dyadic number
            if not (k == "cpu_share_floor" and c.over.get(k) == 0.95):
                assert _f32_exact(getattr(p, k)), (c.name, k)
        assert c.on <= set(T.EDGES), c.name
    assert set(T.OTHER) == set(T.BASE) and len(T.BASE) == 16
    assert all(T.OTHER[k] != T.BASE[k] for k in T.BASE)


@pytest.mark.parametrize("V", VS)
def test_table_has_every_case_of_the_issue_and_stays_small(V):
    names = [c.name for c in T.cases(V)]
    assert len(set(names)) == len(names)
    for want in ("clear", "empty", "empty/R_min=D_max=0", "queue/idle", "queue/offload", "noma/tie", "noma/ratio",
                 "noma/last+dropped", "noma/n_groups", "proj/s==1", "proj/shares", "qos_enable=False", "reward_clip=2^-3",
                 "reward_clip=0", "ordinary", "log2_1p"):
        assert want in names, want
    assert sum(n.startswith("floor=") for n in names) == 6 and sum(n.startswith("field/") for n in names) == 16
    assert sum(c.n for c in T.cases(V)) <= 300
    b = T.batches(V)
    assert b[0].over == {} and sum(x.E for x in b) == sum(c.n for c in T.cases(V))
    sweep = [c for c in T.cases(V) if c.name == "log2_1p"][0]
    x = sweep.meta["x"].ravel()
    assert set(2.0 ** k for k in range(-40, 41)) <= set(x)
    sw = np.sort(x[sweep.meta["at_switch"].ravel()])
    assert len(sw) == 17 and sw[8] == 0.0625 and np.all(np.diff(sw.astype(np.float32)) > 0)
    assert sw[9] == float(np.nextafter(np.float32(0.0625), np.float32(1)))


@pytest.mark.parametrize("V", VS)
def test_oracle_returns_what_each_case_claims(V):
    for b in T.batches(V):
        o = b.oracle()
        o = dict(o, util=o["metrics"][:, 9])
        for c, sl in zip(b.cases, b.slices):
            for key, want in c.expect.items():
                got = o[key][sl]
                sel = ~np.isnan(want)
                assert sel.any(), (c.name, key)
                assert np.array_equal(got[sel], want[sel]), (c.name, key, got[sel], want[sel])     # values, not signs of 0
            for key, m in c.exact.items():
                assert m.any(), (c.name, key)


def test_the_issue_s_own_numbers():
    """B = 2 kbit clears at a share of 0.48828125: data_p == 2 and nothing offloaded there, data_p < 2 one float lower;
    Q0 = 2^21 leaves an empty queue, 2^21 + 0.25 leaves 0.25; three arrivals are 2.9296875 kbit."""
    V = 8
    c = [x for x in T.cases(V) if x.name == "clear"][0]
    o = orc.step(*c.inputs(), T.dyadic_params())
    assert o["data_p"][0, 0] == 2.0 and o["data_p"][2, 0] == 2.0 and o["data_p"][1, 0] < 2.0
    assert o["data_buf"][0, 0] == 2.9296875
    d = T.edge_distances(o, c.inputs(), T.dyadic_params())
    assert d["clear"][0, 0] == 0.0 and 0 < d["clear"][1, 0] < 1e-7 and 0 < d["clear"][2, 0] < 1e-7
    e = [x for x in T.cases(V) if x.name == "empty"][0]
    o = orc.step(*e.inputs(), T.dyadic_params())
    assert o["ein_sum"][0] == 0.0 and np.all(o["reward"] == -1.5)
    q = [x for x in T.cases(V) if x.name == "queue/idle"][0]
    o = orc.step(*q.inputs(), T.dyadic_params())
    assert list(o["mec_q"]) == [0.0, 0.0, 0.25] and np.all(o["ein_sum"] == 0.0)


@pytest.mark.parametrize("V", VS)
def test_every_other_discontinuity_is_far_away(V):
    """For every case and every edge it is NOT placed on, every sample is beyond 1e-3 relative; and a case that says it
    sits on an edge has a sample within float32 resolution of it."""
    for b in T.batches(V):
        o = b.oracle()
        d = T.edge_distances(o, b.inputs(), b.params)
        for c, sl in zip(b.cases, b.slices):
            for edge, dist in d.items():
                if edge in c.on:
                    assert dist[sl].min() < 2e-7, (c.name, edge, dist[sl].min())
                else:
                    assert dist[sl].min() > FAR, (c.name, edge, dist[sl].min(), np.argwhere(dist[sl] <= FAR)[:3])


@pytest.mark.parametrize("V", VS)
def test_step_mask_leaves_out_nothing_but_the_placed_samples(V):
    """`step_mask` on the whole table: no sample is flagged in any case that is not placed on a QoS threshold or on the
    projection (the two of the mask's tests that fire AT an edge: |rate - R_min| < 2e-6, |s - 1| < 1e-6; its tie test
    needs unequal gains), and in those cases exactly the placed samples are.  There is no 0/0 "noise share" env anywhere:
    B - bc / (Cpb 1000) is exactly 0 with the dyadic set."""
    for b in T.batches(V):
        o = b.oracle()
        near_qos, near_other = step_mask(o, b.partner, b.gain, b.mec_q0)
        assert not ((o["ein_sum"] < 1e-3) & (o["ein_sum"] > 0)).any()
        for c, sl in zip(b.cases, b.slices):
            if c.name == "empty/R_min=D_max=0":
                assert near_qos[sl].all() and not near_other[sl].any()             # every vehicle: 0 < 0 and 0 > 0
            elif c.name == "proj/s==1":
                assert not near_qos[sl].any()
                assert near_other[sl][:, 0].all() and not near_other[sl][:, 1:].any()
            else:
                assert not c.on & {"rate", "delay", "s"}, c.name
                assert not near_qos[sl].any() and not near_other[sl].any(), c.name


@pytest.mark.parametrize("V", VS)
def test_one_field_at_a_time_moves_an_output(V):
    """Each of the 16 fields, changed alone on the ordinary state, moves the reward, the backlog, the queue or the power by far more
    than the GPU tests' tolerance -- a kernel reading another field in its place cannot pass."""
    table = {c.name: c for c in T.cases(V)}
    base = orc.step(*table["ordinary"].inputs(), T.dyadic_params())
    for k in T.BASE:
        c = table["field/%s" % k]
        assert c.over == {k: T.OTHER[k]}
        for a, b in zip(c.inputs(), table["ordinary"].inputs()):
            assert np.array_equal(a, b)
        o = orc.step(*c.inputs(), T.dyadic_params(**c.over))
        moved = max(np.max(T._rel(o[key], base[key])) for key in ("reward", "data_buf", "mec_q", "last_power_W"))
        assert moved > 1e-3, (k, moved)
    # and no two fields move the outputs the same way
    outs = [np.concatenate([orc.step(*table["field/%s" % k].inputs(), T.dyadic_params(**{k: T.OTHER[k]}))[key].ravel()
                            for key in ("reward", "data_buf", "mec_q", "vehicle_rate", "last_power_W")]) for k in T.BASE]
    for i in range(len(outs)):
        for j in range(i):
            assert np.max(T._rel(outs[i], outs[j])) > 1e-3, (list(T.BASE)[i], list(T.BASE)[j])


def test_effective_floor_of_every_floor_case():
    want = {"nan": 0.10, "inf": 0.10, "-1.0": 0.0, "0.0": 0.0, "0.95": 0.95, "2.0": 0.95}
    for c in T.cases(4):
        if c.name.startswith("floor="):
            assert orc.effective_floor(c.over["cpu_share_floor"]) == want[c.name[6:]], c.name
    assert dataclasses.is_dataclass(T.Case)


@pytest.mark.parametrize("V", VS)
def test_tie_cases_tell_the_two_listings_apart(V):
    """On an exact tie the vehicle listed second is the near user (ENV:355-360).  The two listings of the tie case give
    vehicle 0 rates that differ by far more than any tolerance, so a `>` written as `>=` in `noma_rate`, or a partner
    read from the wrong lane, cannot pass; with two zero gains both rates are 0 whatever the rule."""
    c = [x for x in T.cases(V) if x.name == "noma/tie"][0]
    o = orc.step(*c.inputs(), T.dyadic_params())
    r = o["vehicle_rate"]
    assert c.partner[0, 0] == 1 and c.partner[1, 0] == 1 + T.SECOND and c.gain[0, 0] == c.gain[0, 1] == c.gain[1, 0]
    assert r[0, 0] < 0.7 * r[1, 0] and r[0, 1] > 1.4 * r[1, 1]            # far when listed first, near when second
    assert np.array_equal(r[0, :2], r[1, 1::-1])                          # the same pair of rates, the other way round
    assert np.all(r[2, :2] == 0.0)
