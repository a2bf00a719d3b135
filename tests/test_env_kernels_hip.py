"""The slow-cadence kernels every episode starts from (csrc/k_env.hip: reset, mobility, geometry, Random_phase) against
the float64 oracle, on every branch and edge; each test is one or two launches on a few thousand states.

* mobility: the case table of tests/mobility_cases.py (states ON every branch and equality edge of a move, up to 8 turn
  draws per move, lanes / map / time_slow varied) with injected draws, and its Philox case (every vehicle crosses all
  eight lanes, so draws .x/.y/.z/.w of both Philox sites decide turns) at env_offset 0 and 2^31 - 3.  Positions are float64
  and the kernel pins `fp contract(off)`: everything is compared for EQUALITY.
* reset: the Philox path at V with 0...3 extras (the V % 4 vehicles spawn anywhere on a down lane, in any direction) and
  two map heights, the injected path with one env per `aux` value.  Equality.
* geometry: M on both sides of every chunk edge up to the accepted 2048, both kernels (staged: M % 16 == 0), V up to 64,
  positions on the RIS's x, in the corners and under the BS.  float32 outputs at the bars of
  test_geometry_and_gain_golden (tests/test_hip_parity.py); the float64 steering angle and base at 1e-15 (figures printed:
  profiles/env_kernels_margins.txt has those of a green run).
* Random_phase: every control_bit, M on both sides of a block; the Philox indices for EQUALITY.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import risvec_oracle as orc  # noqa: E402  (checker)
from tests import mobility_cases as mc  # noqa: E402


def cpu(t):
    return t.detach().cpu().numpy()


def c128(t):
    return cpu(torch.view_as_complex(t)).astype(np.complex128)


def make_env(lanes, width, height, E, V, M=16, b=3, seed=11, env_offset=0, time_slow=None):
    from ris_vec_marl_amd import VecEnviron
    env = VecEnviron(lanes["down"], lanes["up"], lanes["left"], lanes["right"], width, height, V, M, b,
                     n_envs=E, device="cuda:0", seed=seed, env_offset=env_offset)
    if time_slow is not None:
        env.time_slow = time_slow
    return env


def put_vehicles(env, pos, direc, vel):
    t = env.tensors
    t["pos"].copy_(torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float64)))
    t["dir"].copy_(torch.from_numpy(direc.astype(np.int32)))
    t["vel"].copy_(torch.from_numpy(vel.astype(np.float32)))
    return t


# ---------------------------------------------------------------------------- mobility
@pytest.mark.parametrize("name", list(mc.SETS))
def test_mobility_case_set_injected(name):
    build, V, _ = mc.SETS[name]
    lanes, width, height, time_slow, pos, direc, vel, u_turn = build()
    E = direc.shape[0] // V
    assert (E * V) % 256 != 0                      # the last block is partial
    pos, direc, vel, u_turn = pos.reshape(E, V, 2), direc.reshape(E, V), vel.reshape(E, V), u_turn.reshape(E, V, 8)
    o_pos, o_dir, o_nd = orc.mobility(pos, direc, vel.astype(np.float64), u_turn.astype(np.float64), lanes, width, height,
                                      time_slow)
    env = make_env(lanes, width, height, E, V, time_slow=time_slow)
    t = put_vehicles(env, pos, direc, vel)
    nu = env.renew_positions(u_turn, return_n_used=True)
    print("[env kernels] %s: %d states, draws per move %s" % (name, E * V, np.bincount(o_nd.ravel(), minlength=9).tolist()))
    assert np.array_equal(cpu(nu), o_nd)
    assert np.array_equal(cpu(t["dir"]), o_dir)
    assert np.array_equal(cpu(t["pos"]), o_pos)    # float64, bit for bit
    assert np.array_equal(cpu(t["vel"]), vel)      # and the move leaves the velocities alone


@pytest.mark.parametrize("off", mc.PHILOX_OFFSETS)
def test_mobility_philox_every_draw_index(off):
    lanes, width, height, time_slow, pos, direc, vel = mc.philox_case()
    E, V = direc.shape
    env = make_env(lanes, width, height, E, V, seed=mc.PHILOX_SEED, env_offset=off, time_slow=time_slow)
    t = put_vehicles(env, pos, direc, vel)
    ids = off + np.arange(E, dtype=np.int64)
    deep = 0
    for move in (1, 2):                            # the second move: the counter advances, the draws are new ones
        nu = env.renew_positions(return_n_used=True)
        u = orc.philox_turn_draws(ids, V, move, mc.PHILOX_SEED).astype(np.float64)
        pos, direc, o_nd = orc.mobility(pos, direc, vel.astype(np.float64), u, lanes, width, height, time_slow)
        assert np.array_equal(cpu(nu), o_nd), "move %d" % move
        assert np.array_equal(cpu(t["dir"]), direc), "move %d" % move
        assert np.array_equal(cpu(t["pos"]), pos), "move %d" % move
        deep += int((o_nd > 4).sum())
    assert deep > 100                              # (tests/test_mobility_cases_host.py has the per-index conditions)


# ---------------------------------------------------------------------------- reset
@pytest.mark.parametrize("height", [400, 300])
@pytest.mark.parametrize("V", [1, 2, 3, 5, 7, 13, 64])
def test_reset_philox_extras(V, height):
    E, off, seed = 301, 2 ** 31 - 150, 99          # the env ids cross 2^31
    lanes = orc.default_lanes()
    env = make_env(lanes, 400, height, E, V, seed=seed, env_offset=off)
    env.make_new_game()
    spawn, b0 = orc.philox_reset(off + np.arange(E, dtype=np.int64), V, 1, seed, height=height)
    pos, direc, vel, buf = orc.reset(spawn, b0, lanes)
    n4 = 4 * (V // 4)
    if V % 4:                                      # the extras: every (down lane, direction) pair, coord = randint(0, height)
        aux, coord = spawn[:, n4:, 0], spawn[:, n4:, 1]
        assert set(np.unique(aux)) == set(range(16))
        assert coord.min() >= 0 and coord.max() < height and coord.max() >= height - 10
        assert spawn[:, n4:, 2].min() == 15 and spawn[:, n4:, 2].max() == 19
    t = env.tensors
    assert np.array_equal(cpu(t["pos"]), pos)
    assert np.array_equal(cpu(t["dir"]), direc)
    assert np.array_equal(cpu(t["vel"]), vel)
    assert np.array_equal(cpu(t["data_buf"]), buf)


def test_reset_injected_every_aux():
    E, V = 16, 7                                   # one env per aux value; vehicles 4, 5, 6 are extras
    rng = np.random.default_rng(3)
    spawn = np.zeros((E, V, 3), dtype=np.int64)
    spawn[:, :, 0] = rng.integers(0, 4, (E, V))
    spawn[:, 4, 0] = np.arange(16)
    spawn[:, 5, 0] = (np.arange(16) + 5) % 16
    spawn[:, 6, 0] = 15 - np.arange(16)
    spawn[:, :, 1] = rng.integers(0, 400, (E, V))
    spawn[:, :, 2] = rng.integers(10, 20, (E, V))
    b0 = rng.integers(5, 9, E)
    lanes = orc.default_lanes()
    pos, direc, vel, buf = orc.reset(spawn, b0, lanes)
    assert {(int(p), int(d)) for p, d in zip(pos[:, 4, 0] * 1000, direc[:, 4])} == \
        {(int(x * 1000), d) for x in lanes["down"] for d in range(4)}
    env = make_env(lanes, 400, 400, E, V)
    env.make_new_game(spawn.astype(np.int32), b0.astype(np.int32))
    t = env.tensors
    assert np.array_equal(cpu(t["pos"]), pos)
    assert np.array_equal(cpu(t["dir"]), direc)
    assert np.array_equal(cpu(t["vel"]), vel)
    assert np.array_equal(cpu(t["data_buf"]), buf)


# ---------------------------------------------------------------------------- geometry
# pi to the precision of the platform's long double (x87: 64 bits; its literal would be rounded to a double first)
PI_LD = np.longdouble(3.141592653589793) + np.longdouble(1.2246467991473532e-16)
STEER_BAR = 1e-15          # float64: a three-term sum (contracted or not), one sqrt, one divide, one sincospi


def geometry_positions(E, V):
    """Uniform over the map, then: x = 220 exactly (angle 0, on the RIS's x), the four corners of the 400 x 400 map -- (0, 0)
    is under the BS -- the RIS's own (x, y), and a vehicle one ulp from x = 220."""
    rng = np.random.default_rng(E * 100 + V)
    pos = rng.uniform(0.0, 400.0, (E * V, 2))
    special = [(220.0, 17.5), (220.0, 220.0), (0.0, 0.0), (400.0, 0.0), (0.0, 400.0), (400.0, 400.0),
               (np.nextafter(220.0, 400.0), 300.0), (220.0, 400.0)]
    assert E * V >= len(special)
    slots = np.linspace(0, E * V - 1, len(special)).astype(int)         # first and last thread included
    pos[slots] = special
    return pos.reshape(E, V, 2)


@pytest.mark.parametrize("V", [1, 17, 64])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 33, 255, 257, 1000, 2048])
def test_geometry_vs_oracle(M, V):
    E = 9 if V == 1 else 3
    pos = geometry_positions(E, V)
    env = make_env(orc.default_lanes(), 400, 400, E, V, M=M)
    t = env.tensors
    t["pos"].copy_(torch.from_numpy(pos))
    env.compute_parms()
    dist, ang, h_r = orc.geometry(pos, M)
    np.testing.assert_allclose(cpu(t["dist_r"]), dist, rtol=2e-7)
    np.testing.assert_allclose(cpu(t["ang_r"]), ang, rtol=2e-7, atol=1e-9)
    np.testing.assert_allclose(cpu(t["pl"]), orc.pathloss_factor(dist), rtol=3e-7)
    np.testing.assert_allclose(c128(t["h_r"]), h_r, rtol=0, atol=1.2e-7)
    assert (cpu(t["ang_r"])[pos[..., 0] == 220.0] == 0.0).all()
    # the float64 pair the fused step's GEN members rebuild the rows from, against extended precision
    ld = np.longdouble
    dx = pos[..., 0].astype(ld) - ld(220.0)
    ang_x = dx / np.sqrt(dx * dx + (pos[..., 1].astype(ld) - ld(220.0)) ** 2 + ld(1.5 - 25.0) ** 2)
    got_ang = cpu(t["steer_ang"])
    e_ang = float(np.max(np.abs(got_ang.astype(ld) - ang_x) / np.maximum(np.abs(ang_x), ld(1e-300))))
    # z_r = exp(-j pi steer_ang) of the DEVICE's angle; |z| = 1, so the complex error is the relative error
    z = c128(t["z_r"])
    arg = got_ang.astype(ld) * PI_LD
    e_z = float(np.max(np.hypot(z.real.astype(ld) - np.cos(arg), z.imag.astype(ld) + np.sin(arg))))
    print("[env margin] geometry M=%d V=%d: steer_ang %.3e  z_r %.3e  (bar %.0e)  h_r %.3e (bar 1.2e-07)"
          % (M, V, e_ang, e_z, STEER_BAR, float(np.abs(c128(t["h_r"]) - h_r).max())))
    assert e_ang <= STEER_BAR
    assert e_z <= STEER_BAR


# ---------------------------------------------------------------------------- Random_phase
@pytest.mark.parametrize("M", [1, 3, 40, 258])
@pytest.mark.parametrize("cbit", [0, 1, 2, 3, 4, 5, 6])
def test_random_phase_indices(cbit, M):
    E, off, seed = 7, 2 ** 31 - 4, 4
    env = make_env(orc.default_lanes(), 400, 400, E, 2, M=M, b=cbit, seed=seed, env_offset=off)
    ids = off + np.arange(E, dtype=np.int64)
    for call in (1, 2):                            # the second call: the counter advances
        env.Random_phase()
        want = orc.philox_phase_idx(ids, M, call, seed, cbit)
        assert want.min() >= 0 and want.max() < 2 ** cbit
        ang = orc.possible_angles(cbit)
        cand = (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex64).astype(np.complex128)
        theta = c128(env.tensors["theta"])
        d = np.abs(theta[..., None] - cand[None, None, :])
        assert np.array_equal(np.argmin(d, axis=2), want), "call %d" % call
        assert d.min(axis=2).max() <= 1.2e-7       # the float32 image of the candidate, nothing in between
        if cbit == 3:
            assert np.array_equal(cpu(env.tensors["theta_idx"])[:, :M].astype(np.int64), want)
    if cbit >= 2 and E * M >= 4 * 2 ** cbit:
        assert len(np.unique(want)) > 1
