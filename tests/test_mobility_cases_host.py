"""The mobility case table (tests/mobility_cases.py) against the float64 oracle alone: no device.

Three conditions, all on the oracle: the instrumented walk IS `orc.mobility` (bit for bit, so the branch names it reports
are the oracle's branches); every case set reaches every branch name its table lists; and the Philox case makes the
kernel's own draws decide a turn at every draw index 0...7 in every direction.  A builder that misses one is changed; the
condition stays."""
import numpy as np
import pytest

from oracle import risvec_oracle as orc
from tests import mobility_cases as mc


@pytest.mark.parametrize("name", list(mc.SETS))
def test_walk_is_the_oracle_and_reaches_every_branch(name):
    build, V, want = mc.SETS[name]
    lanes, width, height, time_slow, pos, direc, vel, u_turn = build()
    n = direc.shape[0]
    assert n % V == 0 and n % 256 != 0 and vel.dtype == np.float32 and u_turn.dtype == np.float32
    assert set(np.unique(vel)) <= set(mc.VELOCITIES) and set(np.unique(u_turn)) <= set(mc.DRAWS)
    w_pos, w_dir, w_nd, seen = mc.walk_all(lanes, width, height, time_slow, pos, direc, vel, u_turn)
    E = n // V
    o_pos, o_dir, o_nd = orc.mobility(pos.reshape(E, V, 2), direc.reshape(E, V), vel.astype(np.float64).reshape(E, V),
                                      u_turn.astype(np.float64).reshape(E, V, 8), lanes, width, height, time_slow)
    assert np.array_equal(w_pos.reshape(E, V, 2), o_pos)
    assert np.array_equal(w_dir.reshape(E, V), o_dir)
    assert np.array_equal(w_nd.reshape(E, V), o_nd)
    assert sorted(want - seen) == []
    assert sorted(seen - want) == []              # and the table names everything the set can do


def test_draw_values_sit_on_the_threshold():
    d = mc.DRAWS.astype(np.float64)
    assert d[2] == float(np.float32(0.4)) and d[2] > 0.4 and not d[2] < 0.4          # 0.4f does not turn
    assert d[3] < 0.4 and np.nextafter(np.float32(d[3]), np.float32(1)) == np.float32(0.4)


def test_dyadic_set_is_exact():
    lanes, width, height, time_slow, pos, direc, vel, u_turn = mc.dyadic_set()
    dd = vel.astype(np.float64) * time_slow
    assert np.array_equal(dd * 8, vel.astype(np.float64))                            # vel * 0.125: no rounding
    assert all(float(x) * 4 == int(float(x) * 4) for k in lanes for x in lanes[k])


@pytest.mark.parametrize("off", mc.PHILOX_OFFSETS)
def test_philox_case_decides_a_turn_at_every_draw_index(off):
    lanes, width, height, time_slow, pos, direc, vel = mc.philox_case()
    E, V = direc.shape
    u = orc.philox_turn_draws(off + np.arange(E), V, 1, mc.PHILOX_SEED).astype(np.float64)
    o_pos, o_dir, o_nd = orc.mobility(pos, direc, vel.astype(np.float64), u, lanes, width, height, time_slow)
    assert o_nd.min() >= 1
    # draws are consumed until one turns: the last draw a vehicle used decided a turn iff it is below 0.4
    turned = np.take_along_axis(u, (o_nd - 1)[..., None], axis=2)[..., 0] < 0.4
    assert ((o_nd == 8) | turned).all()           # whoever did not turn crossed, and drew for, all eight lanes
    for d in (orc.DIR_U, orc.DIR_D, orc.DIR_L, orc.DIR_R):
        for k in range(8):
            assert ((direc == d) & turned & (o_nd == k + 1)).sum() >= 1, (mc.DIR_NAMES[d], k)
        assert ((direc == d) & ~turned & (o_nd == 8)).sum() >= 1, mc.DIR_NAMES[d]
    assert o_nd.max() == 8 and o_nd.min() == 1
