"""The fused step under a 3GPP channel model (k_step_3gpp<VP[,RING|MULTI]>; risvec_step_fused_3gpp / _multi) on the
GPU: parity with the reference's formulas (gain3gpp.npz) and the step oracle, and bit identity with the two-launch form
update_channel_gains() + step(fused=False) for every fused entry point of VecEnviron."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import risvec_oracle as orc  # noqa: E402  (checker)
from tests.test_hip_parity import (RT, check_step, cpu, load, make_vec, random_step_inputs,  # noqa: E402
                                   step_mask)

DEV = "cuda:0"
KEYS = ("gain", "data_buf", "mec_q", "rate", "data_t", "data_p", "reward", "over_power", "obs", "metrics", "power_w")


def _native():
    from ris_vec_marl_amd import _native as N
    return N


def make_env(E, V, M, model, K=0.0, seed=5, env_offset=0):
    env = make_vec(E, V, M, seed=seed, env_offset=env_offset, yaml=True)
    env.channel_model = model
    env.rician_K_dB = K
    env.make_new_game()
    env.renew_positions()
    rng = np.random.default_rng(99)
    B = rng.uniform(0, 12, (E + env_offset, V)).astype(np.float32)[env_offset:]
    Q = rng.uniform(0, 5e6, E + env_offset).astype(np.float32)[env_offset:]
    env.tensors["data_buf"].copy_(torch.from_numpy(np.ascontiguousarray(B)))
    env.tensors["mec_q"].copy_(torch.from_numpy(np.ascontiguousarray(Q)))
    return env


def step_inputs(E, V, seed, policy_action=False):
    rng = np.random.default_rng(seed)
    action, partner, ng, arrivals = random_step_inputs(E, V, rng)
    if policy_action:
        action = rng.uniform(-1.2, 1.2, (E, V, 2))
    return (torch.from_numpy(action.astype(np.float32)).to(DEV), torch.from_numpy(partner.astype(np.int32)).to(DEV),
            torch.from_numpy(ng.astype(np.int32)).to(DEV), torch.from_numpy(arrivals.astype(np.int32)).to(DEV))


def fading_draws(shape, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    u = torch.rand(shape, device=DEV, generator=g)
    z = torch.randn(shape, device=DEV, generator=g)
    sm = -torch.log1p(-torch.rand(shape, device=DEV, generator=g))
    return u, z, sm


def assert_same(a, b, keys=KEYS):
    for k in keys:
        assert torch.equal(a.tensors[k], b.tensors[k]), k


# 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,K,model", [("3gpp_umi", 0.0, "3gpp_umi"), ("3gpp_uma", 0.0, "3gpp_uma"),
                                         ("3gpp_umi", 6.0, "3gpp_umi"), ("3gpp_uma", 3.0, "3gpp_uma"),
                                         ("other", 0.0, "something_else")])
def test_fused_3gpp_step_vs_reference_formulas(tag, K, model):
    g = load("gain3gpp.npz")
    pre = "%s_K%g_" % (tag, K)
    pos = g[pre + "pos"]
    E, V = pos.shape[:2]
    p = orc.OracleParams.yaml_effective()
    env = make_vec(E, V, 16, yaml=True)
    env.channel_model = model
    env.rician_K_dB = K
    t = env.tensors
    t["pos"].copy_(torch.from_numpy(pos))
    rng = np.random.default_rng(7 + E)
    B0 = rng.uniform(0, 12, (E, V)).astype(np.float32); Q0 = rng.uniform(0, 5e6, E).astype(np.float32)
    t["data_buf"].copy_(torch.from_numpy(B0)); t["mec_q"].copy_(torch.from_numpy(Q0))
    action, partner, ng, arrivals = random_step_inputs(E, V, rng)
    action = action.astype(np.float32)
    fad = tuple(g[pre + k].astype(np.float32) for k in ("u_los", "z_shadow", "small"))
    out = env.step(action, partner.astype(np.int32), ng.astype(np.int32), arrivals.astype(np.int32), fused=True, fading=fad)
    assert _native().last_kernel() == "k_step_3gpp<%d>" % (1 << (V - 1).bit_length())
    g_dev = cpu(t["gain"]).astype(np.float64)
    np.testing.assert_allclose(g_dev, g[pre + "gain"], rtol=RT)
    np.testing.assert_allclose(cpu(env.get_channel_gains()), g[pre + "gain"], rtol=RT)
    o = orc.step(B0.astype(np.float64), Q0.astype(np.float64), g_dev, action.astype(np.float64), partner, ng, arrivals, p)
    near_qos, near_other = step_mask(o, partner, g_dev, Q0)
    okr = check_step(env, out, o, B0.astype(np.float64), p, near_qos, near_other)
    assert okr.mean() > 0.9


# 2 ----------------------------------------------------------------------------------------------------------------
FLAG_MIXES = [dict(obs=True, metrics=True, power_w=True, policy_action=False),
              dict(obs=False, metrics=False, power_w=False, policy_action=True),
              dict(obs=True, metrics=False, power_w=True, policy_action=True)]


@pytest.mark.parametrize("E,V,M", [(301, 8, 64), (4097, 5, 21), (301, 16, 256), (4097, 4, 16)])
@pytest.mark.parametrize("model,K", [("3gpp_umi", 6.0), ("3gpp_uma", 0.0)])
@pytest.mark.parametrize("mix", range(len(FLAG_MIXES)))
def test_fused_3gpp_step_equals_two_launches(E, V, M, model, K, mix):
    N = _native()
    fl = FLAG_MIXES[mix]
    a, b = make_env(E, V, M, model, K), make_env(E, V, M, model, K)
    for n in range(5):
        act, pt, ng, _ = step_inputs(E, V, 100 + n, fl["policy_action"])
        a.update_channel_gains()
        a.step(act, pt, ng, fused=False, **fl)
        b.step(act, pt, ng, fused=True, **fl)
        assert N.last_kernel() == N.step_kernel(b._cstate, N.STEP_3GPP, N.FORM_FUSED)
        assert N.last_kernel() == "k_step_3gpp<%d>" % (1 << (V - 1).bit_length())
    assert a._chan == b._chan and a._steps == b._steps == 5
    assert_same(a, b)


# 3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3, 7])
@pytest.mark.parametrize("injected", [False, True])
@pytest.mark.parametrize("E,V,M,model", [(301, 8, 64, "3gpp_umi"), (1001, 5, 21, "3gpp_uma"), (257, 16, 40, "other")])
def test_step_many_3gpp_equals_single_calls(T, injected, E, V, M, model):
    N = _native()
    a, b = make_env(E, V, M, model, 3.0), make_env(E, V, M, model, 3.0)
    acts = torch.stack([step_inputs(E, V, 200 + t)[0] for t in range(T)])
    _, pt, ng, _ = step_inputs(E, V, 300)
    arr = torch.randint(0, 4, (T, E, V), dtype=torch.int32, device=DEV) if injected else None
    fad = fading_draws((T, E, V), 17) if injected else None
    rec = a.step_many(acts, pt, ng, arr, power_w=True, fading=fad)
    assert N.last_kernel() == "k_step_3gpp<%d,MULTI>" % (1 << (V - 1).bit_length())
    assert N.last_kernel() == N.step_kernel(a._cstate, N.STEP_3GPP, N.FORM_FUSED_MULTI)
    for t in range(T):
        # (slices of [T,E,...] tensors cloned: a step's inputs must be 16-byte aligned)
        b.step(acts[t].clone(), pt, ng, None if arr is None else arr[t].clone(), fused=True, power_w=True,
               fading=None if fad is None else tuple(x[t].clone() for x in fad))
        assert torch.equal(rec["reward"][t], b.tensors["reward"]), t
        assert torch.equal(rec["obs"][t], b.tensors["obs"]), t
        assert torch.equal(rec["metrics"][t], b.tensors["metrics"]), t
    assert a._chan == b._chan and a._steps == b._steps == T
    assert_same(a, b)
    # the bound form: the same again from the same start
    c = make_env(E, V, M, model, 3.0)
    out = {k: torch.empty_like(v) for k, v in rec.items()}
    launch = c.bind_step_many(acts, pt, ng, arr, power_w=True, out=out, fading=fad)
    launch()
    for k in rec:
        assert torch.equal(out[k], rec[k]), k
    assert_same(a, c)


# 4 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,M", [(8, 22), (4, 16), (16, 64)])
def test_step_store_3gpp_equals_step_then_store(V, M):
    from ris_vec_marl_amd import VecReplayBuffer
    N = _native()
    E, T = 777, 7
    gen = torch.Generator(device=DEV); gen.manual_seed(31 + V + M)
    power = [torch.rand(E, V, 2, device=DEV, generator=gen) * 2.4 - 1.2 for _ in range(T)]
    probs = [torch.softmax(torch.randn(E, V, V, device=DEV, generator=gen), -1) for _ in range(T)]
    mask = (torch.rand(E, V, V, device=DEV, generator=gen) < 0.6).to(torch.uint8)
    partner = torch.full((E, V), -1, dtype=torch.int32, device=DEV); partner[:, 0] = 1; partner[:, 1] = (1 << 16)
    ng = torch.full((E,), V - 1, dtype=torch.int32, device=DEV)

    def build():
        return make_env(E, V, M, "3gpp_umi", 6.0), VecReplayBuffer(int(2.5 * E), 5, V + 2, V, device=DEV)

    env, buf = build()
    pw, pr = torch.empty(E, V, 2, device=DEV), torch.empty(E, V, V, device=DEV)
    step = env.bind_step(pw, partner, ng, None, fused=True, policy_action=True, power_w=False)
    for t in range(T):
        pw.copy_(power[t]); pr.copy_(probs[t])
        before = env.observe().clone()
        step()
        buf.store_batch(before, None, env.tensors["metrics"], env.tensors["reward"], env.tensors["obs"], t == T - 1,
                        mask if t % 2 == 0 else None, policy_out=(pw, pr))
    env2, buf2 = build()
    pw2, pr2 = torch.empty(E, V, 2, device=DEV), torch.empty(E, V, V, device=DEV)
    both = env2.bind_step_store(buf2, pw2, partner, ng, pr2, mask, fused=True)
    for t in range(T):
        pw2.copy_(power[t]); pr2.copy_(probs[t])
        both(done=t == T - 1, use_mask=t % 2 == 0)
        assert N.last_kernel() == "k_step_3gpp<%d,RING>" % V
    assert buf.mem_cntr == buf2.mem_cntr == T * E and env._steps == env2._steps == T and env._chan == env2._chan == T
    assert_same(env, env2, [k for k in KEYS if k != "power_w"])
    for k in buf._ARRAYS:
        assert torch.equal(getattr(buf, k), getattr(buf2, k)), k


# 5 ----------------------------------------------------------------------------------------------------------------
def test_bind_step_and_bcd_step_under_3gpp():
    E, V, M = 301, 8, 64
    a, b = make_env(E, V, M, "3gpp_uma", 3.0), make_env(E, V, M, "3gpp_uma", 3.0)
    act, pt, ng, _ = step_inputs(E, V, 400)
    launch = b.bind_step(act, pt, ng, None, fused=True)
    for _ in range(3):
        a.step(act, pt, ng, fused=True)
        launch()
    assert_same(a, b)
    with pytest.raises(ValueError):
        a.step(act, pt, ng, fused=True, steer=True)
    with pytest.raises(ValueError):                 # injected draws are a 3GPP-only input
        a.channel_model = "free"
        a.step(act, pt, ng, fused=True, fading=fading_draws((E, V), 1))
    # step(bcd=True): the sweep as optimize_phase_shift() runs it, then the fused 3GPP step
    c, d = make_env(E, V, M, "3gpp_umi", 0.0), make_env(E, V, M, "3gpp_umi", 0.0)
    for env in (c, d):
        env.compute_parms()
        env.Random_phase()
    for n in range(2):
        act, pt, ng, _ = step_inputs(E, V, 500 + n)
        c.optimize_phase_shift()
        c.update_channel_gains()
        c.step(act, pt, ng, fused=False)
        d.step(act, pt, ng, bcd=True)
        assert _native().last_kernel() == "k_step_3gpp<8>"
    c._sync_theta()
    d._sync_theta()
    assert torch.equal(c.tensors["theta"], d.tensors["theta"])
    assert_same(c, d)


# 6 ----------------------------------------------------------------------------------------------------------------
def test_shards_and_checkpoints_under_3gpp():
    E, V, M, k = 600, 8, 40, 250
    full = make_env(E, V, M, "3gpp_umi", 6.0)
    shard = make_env(E - k, V, M, "3gpp_umi", 6.0, env_offset=k)
    assert torch.equal(full.tensors["pos"][k:], shard.tensors["pos"])
    for n in range(3):
        act, pt, ng, _ = step_inputs(E, V, 600 + n)
        full.step(act, pt, ng, fused=True)
        shard.step(act[k:].clone(), pt[k:].clone(), ng[k:].clone(), fused=True)
    for key in KEYS:
        assert torch.equal(full.tensors[key][k:], shard.tensors[key]), key
    # checkpoint mid-rollout, resumed in a fresh env
    a = make_env(E, V, M, "3gpp_uma", 0.0)
    ins = [step_inputs(E, V, 700 + n) for n in range(4)]
    for act, pt, ng, _ in ins[:2]:
        a.step(act, pt, ng, fused=True)
    sd = a.state_dict()
    b = make_env(E, V, M, "3gpp_uma", 0.0)
    b.load_state_dict(sd)
    for act, pt, ng, _ in ins[2:]:
        a.step(act, pt, ng, fused=True)
        b.step(act, pt, ng, fused=True)
    assert a._chan == b._chan
    assert_same(a, b)
