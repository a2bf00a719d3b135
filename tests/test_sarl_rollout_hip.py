"""GPU tests of the one-launch SARL rollout step (`VecEnviron.bind_sarl_rollout`, `risvec_sarl_rollout`): OU noise,
clip, power / phase map, get_next_phase, cascade + step, the full observation and the transition store.

Every shape runs ONCE (`run_case`, cached): six steps of three envs built from the same seed in lock step -- the
one-launch form, the one-launch form storing into a ring, and the staged path (`sarl_action_map` -> `sarl_step` ->
`sarl_observe`) fed the kernel's own action -- and the tests assert on what that run recorded.

Bars: bit for bit wherever the same float32 operations run in the same order (the action row, the phase map, theta,
the ring against `store_batch`; at the compile-time shapes the whole step against the staged path); against the
float64 oracle the bounds of `test_sarl_step_golden` (tests/test_hip_parity.py), restated at each assert.
"""
import functools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import risvec_oracle as orc  # noqa: E402  (checker)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
RT = 1e-5
STEPS = 6
SEED = 21
# (E, V, M): two compile-time shapes; run-time-M members with ragged rows (22), V = 16 (120) and one env per ... four
# envs per wavefront at the largest M (256); a compile-time V = 16 shape.  Every E leaves a partial last wavefront.
SHAPES = [(777, 8, 40), (130, 4, 16), (301, 8, 22), (97, 16, 120), (33, 8, 256), (65, 16, 64)]
BITWISE = {(777, 8, 40), (130, 4, 16)}        # the staged path sums the cascade in the same order there
OU = dict(sigma=0.15, theta=0.2, dt=1e-2, mu=0.0)
STATE = ("theta", "gain", "rate", "data_t", "data_p", "data_buf", "reward", "over_power", "over_data", "obs")


def cpu(t):
    return t.detach().cpu().numpy()


def make_env(E, V, M, seed=SEED, env_offset=0):
    from ris_vec_marl_amd import VecEnviron, reference_lanes
    L = reference_lanes()
    env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3,
                     n_envs=E, device="cuda:0", seed=seed, env_offset=env_offset)
    env.make_new_game()
    env.compute_parms()
    return env


def inputs(E, V, M):
    """mu ~ U(-1, 1) and the injected N(0, 1) draws of the six steps (host, float32)."""
    rng = np.random.default_rng(1000 * V + M)
    A = 2 * V + M
    return (rng.uniform(-1, 1, (STEPS, E, A)).astype(np.float32), rng.standard_normal((STEPS, E, A)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def run_case(E, V, M):
    from ris_vec_marl_amd import OUNoise, SarlReplayBuffer, sarl_action_map, sarl_observe
    from ris_vec_marl_amd import _native as N
    dev = torch.device("cuda:0")
    A, tn = 2 * V + M, M // V
    mus, zs = inputs(E, V, M)
    env, env_r, env_s = make_env(E, V, M), make_env(E, V, M), make_env(E, V, M)
    mu, z = torch.empty(E, A, device=dev), torch.empty(E, A, device=dev)
    noise, noise_r = OUNoise(E, A, device=dev, **OU), OUNoise(E, A, device=dev, **OU)
    cap = int(2.5 * E)
    ring, ref = SarlReplayBuffer(cap, tn + 5, A, V, device=dev, seed=5), SarlReplayBuffer(cap, tn + 5, A, V, device=dev)
    launch = env.bind_sarl_rollout(mu, noise=noise, z=z)
    launch_r = env_r.bind_sarl_rollout(mu, noise=noise_r, replay=ring, z=z)
    t, ts = env.tensors, env_s.tensors
    static = dict(h_r=cpu(torch.view_as_complex(t["h_r"])).astype(np.complex128),
                  b=cpu(torch.view_as_complex(t["b"])).astype(np.complex128), dist=cpu(t["dist_r"]).astype(np.float64))
    rec = []
    for k in range(STEPS):
        mu.copy_(torch.from_numpy(mus[k]))
        z.copy_(torch.from_numpy(zs[k]))
        s = dict(x0=cpu(noise.x).copy(), buf0=cpu(t["data_buf"]).copy(), step=env._steps)
        obs_before = env.sarl_observation().clone()
        done = k == STEPS - 1
        launch(done)
        s["kernel"] = N.last_kernel()
        launch_r(done)
        s["kernel_ring"] = N.last_kernel()
        if k == 0:
            s["ring_state0"] = cpu(ring.state_memory[:E]).copy()
        ref.store_batch(obs_before, launch.action, t["metrics"][:, 0], launch.obs, done)
        # the staged path of the same checkout, fed the kernel's own action row
        power, phase = sarl_action_map(launch.action, V, M)
        env_s.sarl_step(power, phase)
        s["staged"] = {key: cpu(ts[key]).copy() for key in STATE}
        s["staged"]["metrics0"] = cpu(ts["metrics"][:, 0]).copy()
        s["staged"]["obs_full"] = cpu(sarl_observe(env_s, phase))
        s["staged"]["phase"] = cpu(phase)
        s["staged"]["power"] = cpu(power)
        s["clamp"] = cpu(torch.clamp(mu + noise.x, -0.999, 0.999))
        s["fused"] = {key: cpu(t[key]).copy() for key in STATE}
        s["fused"]["metrics0"] = cpu(t["metrics"][:, 0]).copy()
        s.update(x1=cpu(noise.x).copy(), action=cpu(launch.action).copy(), phase=cpu(launch.phase).copy(),
                 obs_full=cpu(launch.obs).copy())
        rec.append(s)
    return dict(rec=rec, static=static, ring=ring, ref=ref, env=env, mem_cntr=ring.mem_cntr, cap=cap)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(bits(a), bits(b)), "%s: %d of %d words differ" % (what, (bits(a) != bits(b)).sum(), a.size)


# ---------------------------------------------------------------------------------------------- 1. noise
@pytest.mark.parametrize("E,V,M", SHAPES)
def test_ou_noise_injected_draws(E, V, M):
    """x' against the float64 evaluation of noise.py:13-14 on the same float32 inputs: five float32 roundings at 2^-24
    on a running magnitude <= 1 + |x'|, with margin."""
    mus, zs = inputs(E, V, M)
    for k, s in enumerate(run_case(E, V, M)["rec"]):
        x, z = s["x0"].astype(np.float64), zs[k].astype(np.float64)
        th, mu, sg, dt = (np.float64(np.float32(OU[n])) for n in ("theta", "mu", "sigma", "dt"))
        want = x + th * (mu - x) * dt + sg * np.sqrt(dt) * z
        err = np.abs(s["x1"] - want)
        print("[rollout margin] OU injected (%d,%d,%d) step %d: max err / bound %.3f" % (E, V, M, k, (err / (5e-7 * (1 + np.abs(want)))).max()))
        assert (err <= 5e-7 * (1 + np.abs(want))).all()
        assert np.abs(s["x1"]).max() > 0


def philox_normals(env_ids, A, counter, seed):
    """z [E, A] as the kernel draws it: Philox4x32-10 at (env id, pair j, counter, site 11; seed); Box-Muller of the
    block's words (.x, .y) gives elements 2j and 2j + 1 (`orc.normal2`: float64 from the float32 uniforms)."""
    e = np.asarray(env_ids, dtype=np.uint64)[:, None]
    j = np.arange(A // 2, dtype=np.uint64)[None, :]
    r0, r1, _, _ = orc.philox4x32(e, j, np.uint64(counter), np.uint64(11), seed)
    z = np.empty((e.shape[0], A))
    z[:, 0::2], z[:, 1::2] = orc.normal2(r0, r1)
    return z


def test_ou_noise_philox_key_sharding_and_moments():
    from ris_vec_marl_amd import OUNoise
    E, V, M = 777, 8, 40
    A, dev = 2 * V + M, torch.device("cuda:0")
    mu = torch.from_numpy(inputs(E, V, M)[0][0]).to(dev)
    env = make_env(E, V, M)
    noise = OUNoise(E, A, device=dev, seed=99, **OU)
    launch = env.bind_sarl_rollout(mu, noise=noise)
    sg_sq = np.float64(np.float32(OU["sigma"])) * np.sqrt(np.float64(np.float32(OU["dt"])))
    x_prev = np.zeros((E, A))
    for k in range(2):
        launch()
        z = philox_normals(np.arange(E), A, k, 99)            # the step counter is the Philox counter
        th, dt = np.float64(np.float32(OU["theta"])), np.float64(np.float32(OU["dt"]))
        want = x_prev + th * (0.0 - x_prev) * dt + sg_sq * z
        got = cpu(noise.x).astype(np.float64)
        # the float32 formula (5e-7 (1 + |x'|), as for injected draws) on a float32 Box-Muller: logf, sqrtf, sincospif and
        # the product are each good to ~1 ulp, |z| <= 5.8 -> |dz| <= 4 x 6e-8 x 5.8 < 2e-6, which enters x' times sigma sqrt(dt)
        err = np.abs(got - want)
        assert (err <= 5e-7 * (1 + np.abs(want)) + sg_sq * 2e-6).all(), err.max()
        if k == 0:
            zd = got / sg_sq                                   # x = 0 before the first step: x' = sigma sqrt(dt) z
            n = zd.size
            assert abs(zd.mean()) <= 5 / math.sqrt(n)
            assert abs(zd.var() - 1.0) <= 5 * math.sqrt(2.0 / n)
        x_prev = got
    assert_same_bits(cpu(launch.action), cpu(torch.clamp(mu + noise.x, -0.999, 0.999)), "action with Philox noise")
    # two shards of the same batch draw what the whole batch drew
    E1 = 300
    x_whole = cpu(noise.x)
    for lo, hi in ((0, E1), (E1, E)):
        shard = make_env(hi - lo, V, M, env_offset=lo)
        nz = OUNoise(hi - lo, A, device=dev, seed=99, env_offset=lo, **OU)
        ls = shard.bind_sarl_rollout(mu[lo:hi].contiguous(), noise=nz)
        ls()
        ls()
        assert_same_bits(cpu(nz.x), x_whole[lo:hi], "noise state of shard [%d, %d)" % (lo, hi))


# ---------------------------------------------------------------------------------------------- 2. action row
@pytest.mark.parametrize("E,V,M", SHAPES)
def test_action_row_and_phase_map(E, V, M):
    for s in run_case(E, V, M)["rec"]:
        assert_same_bits(s["action"], s["clamp"], "action = clamp(mu + x', +-0.999)")
        assert_same_bits(s["phase"], s["staged"]["phase"], "phase = sarl_action_map(action)[1]")
        assert s["phase"].min() > 0 and s["phase"].max() < 2 * np.pi


# ---------------------------------------------------------------------------------------------- 3. staged path / oracle
@pytest.mark.parametrize("E,V,M", sorted(BITWISE))
def test_lock_step_with_the_staged_path_bit_for_bit(E, V, M):
    for k, s in enumerate(run_case(E, V, M)["rec"]):
        for key in STATE + ("metrics0",):
            assert_same_bits(s["fused"][key], s["staged"][key], "step %d %s" % (k, key))
        assert_same_bits(s["obs_full"], s["staged"]["obs_full"], "step %d launch.obs" % k)


@pytest.mark.parametrize("E,V,M", SHAPES)
def test_theta_gain_step_and_observation_against_the_oracle(E, V, M):
    case = run_case(E, V, M)
    st, sp = case["static"], orc.SarlParams()
    kept, total = 0, 0
    for k, s in enumerate(case["rec"]):
        f = s["fused"]
        # theta: what k_set_phase stores for the same float32 angles (the staged env's get_next_phase), bit for bit
        assert_same_bits(f["theta"], s["staged"]["theta"], "step %d theta" % k)
        theta = (f["theta"][..., 0] + 1j * f["theta"][..., 1]).astype(np.complex128)
        np.testing.assert_allclose(theta, np.exp(1j * s["phase"].astype(np.float64)), rtol=0, atol=1e-7)
        # gain: the existing bound of the SARL step (RT gain + pathloss 2 |img| 5e-7 M)
        gain_ref = orc.gain_free(theta, st["h_r"], st["b"], st["dist"])
        img = np.einsum("em,evm,m->ev", theta, st["h_r"], st["b"])
        atol = orc.pathloss_factor(st["dist"]) * 2 * np.abs(img) * (5e-7 * M)
        gain = f["gain"].astype(np.float64)
        assert (np.abs(gain - gain_ref) <= RT * gain_ref + atol).all()
        # step: the oracle on the device's own gains and the powers the kernel mapped (tolerances of test_sarl_step_golden)
        power = s["staged"]["power"].astype(np.float64)
        assert_same_bits(s["staged"]["power"][:, 0], ((s["action"][:, :V] + np.float32(1)) / np.float32(2)), "p0")
        buf0 = s["buf0"].astype(np.float64)
        arr = orc.philox_arrivals(np.arange(E), V, s["step"], SEED, sp.rate)
        o = orc.sarl_step(buf0, gain, power, arr, sp)
        ok = ~((np.abs(o["margin"]["buf"]) < 2e-5) | (np.abs(o["margin"]["over"]) < 2e-5))
        kept, total = kept + ok.sum(), total + ok.size
        np.testing.assert_allclose(f["rate"], o["vehicle_rate"], rtol=RT, atol=1e-7)
        np.testing.assert_allclose(f["data_t"], o["data_t"], rtol=RT, atol=1e-7)
        np.testing.assert_allclose(f["data_p"], o["data_p"], rtol=RT, atol=1e-7)
        kb = np.maximum(buf0, 1.0)
        assert (np.abs(f["data_buf"] - o["data_buf"])[ok] <= (RT * o["data_buf"] + 4e-7 * kb)[ok]).all()
        assert (np.abs(f["over_data"] - o["over_data"])[ok] <= (RT * o["over_data"] + 4e-7 * kb)[ok]).all()
        p1 = power[:, 1, :]
        proc = np.where(o["over_data"] > 0, p1 - o["over_power"], 0.0)
        assert (np.abs(f["over_power"] - o["over_power"])[ok] <= (RT * np.maximum(p1, proc) + 3e-6 * proc + 1e-7)[ok]).all()
        env_ok = ok.all(axis=1)
        r_floor = sp.t_factor2 * (4e-7 * kb).mean(axis=1) + 1e-7
        err = np.abs(f["metrics0"] - o["reward_mean"])
        assert (err <= RT * np.abs(o["reward_mean"]) + r_floor)[env_ok].all()
        # the full observation: each agent's phase slice + the tail of the device's own outputs
        want = orc.sarl_obs(s["phase"].astype(np.float64), *(f[n].astype(np.float64) for n in
                                                             ("data_buf", "data_t", "data_p", "over_data", "rate")))
        np.testing.assert_allclose(s["obs_full"], want, rtol=2e-6, atol=1e-8)
        assert_same_bits(s["obs_full"][..., M // V:], f["obs"], "tail of launch.obs = state.obs")
    print("[rollout margin] (%d,%d,%d): near-threshold samples left out %d of %d" % (E, V, M, total - kept, total))
    assert kept / total >= 0.98


# ---------------------------------------------------------------------------------------------- 4. ring
@pytest.mark.parametrize("E,V,M", SHAPES)
def test_ring_equals_store_batch_of_the_plain_launch(E, V, M):
    case = run_case(E, V, M)
    ring, ref, tn = case["ring"], case["ref"], M // V
    assert case["cap"] == int(2.5 * E) and ring.mem_cntr == STEPS * E == ref.mem_cntr
    for name in ring._ARRAYS:
        a, b = cpu(getattr(ring, name)), cpu(getattr(ref, name))
        assert_same_bits(a, b, name)
    first = case["rec"][0]["ring_state0"].reshape(E, V, tn + 5)
    assert (first[..., :tn] == 0).all() and (first[..., tn] > 0).all()      # zero theta slice, DataBuf / 10 behind it
    done = cpu(ring.terminal_memory)
    rows_last = (np.arange(E) + (STEPS - 1) * E) % case["cap"]
    assert done[rows_last].all() and done.sum() == E


def test_ring_sampling():
    E, V, M = 130, 4, 16
    ring = run_case(E, V, M)["ring"]
    max_mem = min(ring.mem_cntr, ring.mem_size)
    idx = torch.tensor([0, 1, max_mem - 1, 7, 7, E, 2 * E + 3], dtype=torch.int64)
    out = ring.sample_buffer(len(idx), idx=idx)
    for got, name in zip(out, ring._ARRAYS):
        want = cpu(getattr(ring, name))[idx.numpy()]
        assert got.shape == want.shape and np.array_equal(cpu(got), want), name
    B, n0 = 4096, ring._samples
    a = [cpu(x) for x in ring.sample_buffer(B)]
    rows = cpu(ring.last_batch)
    r0 = orc.philox4x32(np.arange(B, dtype=np.uint64), 0, np.uint64(n0 + 1), np.uint64(8), ring.seed)[0]
    assert np.array_equal(rows, ((r0.astype(np.uint64) * np.uint64(max_mem)) >> np.uint64(32)).astype(np.int64))
    assert rows.min() >= 0 and rows.max() < max_mem and len(np.unique(rows)) > max_mem // 2
    for got, name in zip(a, ring._ARRAYS):
        assert np.array_equal(got, cpu(getattr(ring, name))[rows]), name
    with pytest.raises(ValueError):
        ring.sample_buffer(2, idx=torch.tensor([0, max_mem]))


# ---------------------------------------------------------------------------------------------- 5. golden
@pytest.mark.parametrize("name", ["sarl_step_8_40", "sarl_step_4_16"])
def test_golden_rewards_through_the_rollout_launch(name):
    """The reference's own SARL step samples, driven through the one-launch form without noise: mu is the inverse map of
    their action_power / action_phase; envs with an element outside +-0.999 (which the clip would move) are skipped."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    E, V = g["data_buf0"].shape
    M = g["theta"].shape[1]
    mu64 = np.concatenate([2 * g["action_power"][:, 0] - 1, 2 * g["action_power"][:, 1] - 1, g["action_phase"] / np.pi - 1], axis=1)
    inside = (np.abs(mu64) <= 0.999).all(axis=1)
    assert inside.mean() > 0.9
    env = make_env(E, V, M)
    t = env.tensors
    t["pos"].copy_(torch.from_numpy(g["pos"]))
    env.compute_parms()
    t["data_buf"].copy_(torch.from_numpy(g["data_buf0"].astype(np.float32)))
    action, phase, _ = env.sarl_rollout(mu64.astype(np.float32), arrivals=g["arrivals"].astype(np.int32))
    assert_same_bits(cpu(action)[inside], mu64.astype(np.float32)[inside], "without noise the action is mu")
    sp = orc.SarlParams()
    gain = cpu(t["gain"]).astype(np.float64)
    o = orc.sarl_step(g["data_buf0"], gain, g["action_power"], g["arrivals"], sp)
    gain_ref = orc.gain_free(g["theta"], g["h_r"], g["b"], g["dist"])
    o_ref = orc.sarl_step(g["data_buf0"], gain_ref, g["action_power"], g["arrivals"], sp)
    np.testing.assert_allclose(o_ref["reward_mean"], g["reward_mean"], rtol=1e-12)
    near = (np.abs(o["margin"]["buf"]) < 2e-5) | (np.abs(o["margin"]["over"]) < 2e-5)
    same_branch = ((o_ref["margin"]["buf"] > 0) == (o["margin"]["buf"] > 0)).all(axis=1) & \
                  ((o_ref["margin"]["over"] > 0) == (o["margin"]["over"] > 0)).all(axis=1)
    sel = inside & (~near).all(axis=1) & same_branch
    assert sel.mean() > 0.95 * inside.mean()
    kb = np.maximum(g["data_buf0"], 1.0)
    r_floor = sp.t_factor2 * (4e-7 * kb).mean(axis=1) + 1e-7
    err = np.abs(cpu(t["metrics"][:, 0]) - g["reward_mean"])
    assert (err <= RT * np.abs(g["reward_mean"]) + r_floor + np.abs(o["reward_mean"] - o_ref["reward_mean"]))[sel].all()
    print("[rollout margin] %s: reward rel err vs reference %.3e" % (name, (err / np.abs(g["reward_mean"]))[sel].max()))


# ---------------------------------------------------------------------------------------------- 6. plumbing
def test_bound_and_unbound_twins_leave_identical_tensors():
    from ris_vec_marl_amd import OUNoise
    E, V, M = 130, 4, 16
    A, dev = 2 * V + M, torch.device("cuda:0")
    mus, zs = inputs(E, V, M)
    env_a, env_b = make_env(E, V, M), make_env(E, V, M)
    na, nb = OUNoise(E, A, device=dev, **OU), OUNoise(E, A, device=dev, **OU)
    mu, z = torch.empty(E, A, device=dev), torch.empty(E, A, device=dev)
    launch = env_a.bind_sarl_rollout(mu, noise=na, z=z)
    for k in range(2):
        mu.copy_(torch.from_numpy(mus[k]))
        z.copy_(torch.from_numpy(zs[k]))
        launch()
        out = env_b.sarl_rollout(mus[k], noise=nb, z=zs[k])           # host arrays: converted
        for a, b, what in zip((launch.action, launch.phase, launch.obs), out, ("action", "phase", "obs")):
            assert_same_bits(cpu(a), cpu(b), what)
        assert_same_bits(cpu(na.x), cpu(nb.x), "noise.x")
        for key in STATE + ("metrics",):
            assert_same_bits(cpu(env_a.tensors[key]), cpu(env_b.tensors[key]), key)
    assert env_a._steps == env_b._steps == 2
    with pytest.raises(ValueError):
        env_a.bind_sarl_rollout(mu.cpu(), noise=na)                   # a host tensor is refused by the bound form
    with pytest.raises(ValueError):
        env_a.bind_sarl_rollout(mu, z=z)                              # draws without a noise object


@pytest.mark.parametrize("V,M", [(5, 21), (8, 258)])
def test_shapes_without_a_member_are_refused_by_the_launch(V, M):
    from ris_vec_marl_amd import _native as N, sarl_action_map
    E = 8
    env = make_env(E, V, M)
    assert not N.load().risvec_sarl_rollout_supported(V, M)
    mu = torch.zeros(E, 2 * V + M, device="cuda:0")
    launch = env.bind_sarl_rollout(mu)
    with pytest.raises(N.RisVecError, match="staged path"):
        launch()
    assert env._steps == 0
    power, phase = sarl_action_map(mu, V, M)
    out = env.sarl_step(power, phase)                                 # the staged path serves the shape
    assert out[0].shape == (E,) and torch.isfinite(out[0]).all()


def test_last_kernel_names_the_member():
    for (E, V, M), want in (((777, 8, 40), "k_sarl_rollout<8,40,"), ((301, 8, 22), "k_sarl_rollout<8,G16,N1,"),
                            ((33, 8, 256), "k_sarl_rollout<8,G64,N2,")):
        s = run_case(E, V, M)["rec"][0]
        assert s["kernel"].startswith(want) and "RING" not in s["kernel"], s["kernel"]
        assert s["kernel_ring"].startswith(want) and s["kernel_ring"].endswith(",RING>"), s["kernel_ring"]


def test_sarl_rollout_example_runs():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "sarl_rollout.py"), "256", "1"], cwd=root,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "episode 0" in out.stdout and "env-steps/s" in out.stdout and "buffer 25600 rows" in out.stdout
