"""The production (Philox) draws of the two sampled kernels that no other test restates: the 3GPP fading of
`draws_3gpp` (k_gain_3gpp, k_step_3gpp<VP[,MULTI]>) and the Normal / Gumbel draws of `k_policy_sample`, each against
the float64 restatement in oracle/ (`philox_fading`, `philox_draws`) at the kernel's own counter, seed and global env id.

Bounds (derived, not tuned).  The float32 Box-Muller of risvec_dev.hpp::normal2 is good to |dz| <= DZ = 2e-6 (logf,
sqrtf, sincospif and a product at ~1 ulp each on |z| <= 5.8; tests/test_sarl_rollout_hip.py).  U = 2^-24 is one float32
rounding, ULP = 2^-23 the error of a 1-ulp library function.
  gain     RT g (the float32 result, float64 arithmetic before it) + g (ln 10 / 10) sigma_shadow DZ (the shadow is
           10^(z sigma / 10)); Rice adds large shadow 2 sqrt(2) sqrt(small) sg DZ: small = hr^2 + hi^2 moves by
           2 sg (|hr| + |hi|) DZ <= 2 sqrt(2) sqrt(small) sg DZ, which does not shrink with small (cancellation in hr).
  power    tanh is 1-Lipschitz: std DZ + 4 U (|eps| std + |mu|) on its argument (expf at 1 ulp, product, sum) + tanhf's
           own 2 ulp.
  probs    z = (logit + g) / tau with g = -logf(-logf(u)): |dz| <= (ULP + ULP |g| + U |logit + g|) / tau + U |z|
           + U |z - zmax|; the soft-max moves by <= 2 max|dz| p (1 - p) (+ second order) and adds its own roundings
           p (2 ULP + (log2 VP + 1) U).  Asserted to stay inside the 2e-5 the injected-draw golden test grants.
`[draws margin]` lines print err / bound per case."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import policy_oracle as PO  # noqa: E402  (checker)
from oracle import risvec_oracle as orc  # noqa: E402  (checker)
from oracle.replay_oracle import marshal_actions  # noqa: E402  (checker)
from tests.test_draws_oracle import (FADING_COUNTER, FADING_ONES, FADING_SEED, GUMBEL_CALL, GUMBEL_ONES,  # noqa: E402
                                     GUMBEL_SEED)
from tests.test_hip_parity import RT, check_step, cpu, make_vec, random_step_inputs, step_mask  # noqa: E402

DEV = "cuda:0"
DZ = 2e-6
U, ULP = 2.0 ** -24, 2.0 ** -23
FLT_MIN = float(np.finfo(np.float32).tiny)
SEED, OFFSET = 21, 1000


def margin(what, ratio):
    print("[draws margin] %s: max err / bound %.3f" % (what, float(ratio)))


# ------------------------------------------------------------------------------------------------ 3GPP fading
def make_env(E, V, M, model, K, seed=SEED, env_offset=OFFSET):
    env = make_vec(E, V, M, seed=seed, env_offset=env_offset, yaml=True)
    env.channel_model = model
    env.rician_K_dB = K
    env.make_new_game()
    env.renew_positions()
    rng = np.random.default_rng(99)
    env.tensors["data_buf"].copy_(torch.from_numpy(rng.uniform(0, 12, (E, V)).astype(np.float32)))
    env.tensors["mec_q"].copy_(torch.from_numpy(rng.uniform(0, 5e6, E).astype(np.float32)))
    return env


def oracle_gain(env, model, K, counter):
    """(gain, bound) of the env's float64 positions under the device draws of channel counter `counter`.  The LOS
    decision u < p_LOS is a discontinuity: no sample may sit within 1e-9 of it (u is a multiple of 2^-24, p_LOS is
    float64 on both sides and agrees to ~1e-16), asserted on the CPU values before anything is compared."""
    E, V = env.n_envs, env.n_veh
    pos = cpu(env.tensors["pos"]).astype(np.float64)
    p = orc.OracleParams.yaml_effective()
    ids = np.arange(env.env_offset, env.env_offset + E)
    u, z, sm = orc.philox_fading(ids, V, counter, env.seed, K)
    p_los = 0.7 * np.exp(-np.hypot(pos[..., 0], pos[..., 1]) / 200.0)
    assert (np.abs(u - p_los) >= 1e-9).all()
    g = orc.gain_3gpp(pos, model, u, z, sm, p)
    sd = np.where(u < p_los, p.shadow_std_los, p.shadow_std_nlos)
    bound = RT * g + g * (math.log(10.0) / 10.0) * sd * DZ
    if np.float32(K) > np.float32(1e-6):
        sg = 1.0 / math.sqrt(2.0 * (10 ** (K / 10.0) + 1.0))
        bound = bound + orc.gain_3gpp(pos, model, u, z, np.ones_like(sm), p) * (2 * math.sqrt(2.0) * np.sqrt(sm) * sg * DZ)
    return g, bound


def assert_gain(env, model, K, counter, what):
    got = cpu(env.tensors["gain"]).astype(np.float64)
    want, bound = oracle_gain(env, model, K, counter)
    err = np.abs(got - want)
    margin(what, (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), (what, np.argwhere(err > bound)[:5])
    return got


# (a) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,V", [(301, 8), (130, 5), (97, 16), (65, 4), (40, 33)])
@pytest.mark.parametrize("K", [0.0, 3.0, 6.0])
@pytest.mark.parametrize("model", ["3gpp_umi", "3gpp_uma", "something_else"])
def test_gain_3gpp_device_draws_vs_oracle(model, K, E, V):
    env = make_env(E, V, 16, model, K)
    assert env.seed == SEED and env.env_offset == OFFSET and env._chan == 0
    seen = []
    for call in range(3):
        env.update_channel_gains()
        assert env._chan == call + 1
        seen.append(assert_gain(env, model, K, env._chan, "gain %s K=%g (%d,%d) call %d" % (model, K, E, V, call + 1)))
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert (seen[0] > 0).all()


# (b) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,V,M,model,K", [(301, 8, 64, "3gpp_umi", 6.0), (130, 5, 21, "3gpp_uma", 0.0)])
def test_fused_3gpp_entries_draw_at_their_counter(E, V, M, model, K):
    from ris_vec_marl_amd import _native as N
    env = make_env(E, V, M, model, K)
    env.compute_parms()
    t, p = env.tensors, orc.OracleParams.yaml_effective()
    vp = 1 << (V - 1).bit_length()
    rng = np.random.default_rng(7 + E)
    action, partner, ng, arrivals = random_step_inputs(E, V, rng)
    action, partner32, ng32 = action.astype(np.float32), partner.astype(np.int32), ng.astype(np.int32)
    B0, Q0 = cpu(t["data_buf"]).astype(np.float64), cpu(t["mec_q"]).astype(np.float64)
    out = env.step(action, partner32, ng32, arrivals.astype(np.int32), fused=True)
    assert N.last_kernel() == "k_step_3gpp<%d>" % vp and env._chan == 1
    g_dev = assert_gain(env, model, K, env._chan, "fused step gain %s K=%g (%d,%d)" % (model, K, E, V))
    o = orc.step(B0, Q0, g_dev, action.astype(np.float64), partner, ng, arrivals, p)
    near_qos, near_other = step_mask(o, partner, g_dev, Q0)
    okr = check_step(env, out, o, B0, p, near_qos, near_other)
    assert okr.mean() > 0.9
    env.Random_phase()                          # shares the channel counter
    assert env._chan == 2
    T, start = 3, env._chan
    acts = np.stack([random_step_inputs(E, V, rng)[0] for _ in range(T)]).astype(np.float32)
    env.step_many(acts, partner32, ng32)
    assert N.last_kernel() == "k_step_3gpp<%d,MULTI>" % vp and env._chan == start + T and env._steps == 1 + T
    g_many = assert_gain(env, model, K, start + T, "step_many final gain %s K=%g (%d,%d)" % (model, K, E, V))
    assert not np.array_equal(g_many, g_dev)


# (c) ------------------------------------------------------------------------------------------------------------
def test_3gpp_exp1_edge_gives_a_zero_gain_and_finite_steps():
    """The Rayleigh power -ln(u) at u == 1 (all-ones top 24 bits of .w): a gain of exactly 0, which `thr + 1e-12f` and
    the NOMA eps must carry through step() without a division by zero -- alone and as either member of a pair."""
    env_id, veh = FADING_ONES
    E, V, M = 5, 8, 16
    mk = lambda: make_env(E, V, M, "3gpp_umi", 0.0, seed=FADING_SEED, env_offset=env_id - 2)   # noqa: E731
    a = mk()
    assert a._chan == FADING_COUNTER - 1
    a.update_channel_gains()
    g = assert_gain(a, "3gpp_umi", 0.0, FADING_COUNTER, "gain at the Exp(1) edge")
    assert g[2, veh] == 0.0 and (np.delete(g.ravel(), 2 * V + veh) > 0).all()
    mate = veh - 1
    for near, far in ((None, None), (veh, mate), (mate, veh)):
        b = mk()
        partner = np.full((E, V), -1, dtype=np.int32)
        if near is not None:
            partner[:, near], partner[:, far] = far, near + (1 << 16)
        ng = np.full(E, V - (near is not None), dtype=np.int32)
        action = np.random.default_rng(3).uniform(0.05, 1.0, (E, 2, V)).astype(np.float32)
        out = b.step(action, partner, ng, fused=True)
        assert b._chan == FADING_COUNTER
        t = b.tensors
        assert np.array_equal(cpu(t["gain"]), cpu(a.tensors["gain"]))
        for name in ("reward", "data_buf", "mec_q", "rate", "data_t", "data_p", "over_power", "over_data", "obs", "metrics",
                     "power_w"):
            assert np.isfinite(cpu(t[name])[2]).all(), (name, near)
        assert all(np.isfinite(cpu(x)[2]).all() for x in out)
        assert cpu(t["rate"])[2, veh] == 0.0


# ------------------------------------------------------------------------------------------------ policy epilogue
def T_(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def guarded(n):
    """n floats to be written (NaN until then) and 64 behind them that must stay as they are."""
    buf = torch.full((n + 64,), float("nan"), device=DEV)
    buf[n:] = 12345.0
    return buf


def sample_native(heads, mask, tau, hard, seed, counter, env_offset, floor=0.1):
    """risvec_policy_sample on host-made float32 heads [V,E,4+V], draws from the device."""
    from ris_vec_marl_amd import _native as N
    V, E, H = heads.shape
    assert H == 4 + V and heads.dtype == np.float32
    lib, st = N.load(), torch.cuda.current_stream().cuda_stream
    h, tt, hd = T_(heads), T_(np.asarray(tau, np.float32)), T_(np.asarray(hard, np.uint8))
    mk = None if mask is None else T_(mask.astype(np.uint8))
    shapes = dict(power=(E, V, 2), probs=(E, V, V), onehot=(E, V, V), action_env=(E, 2, V), p_off01=(E, V),
                  action_store=(E, V, V + 2))
    bufs = {k: guarded(int(np.prod(s))) for k, s in shapes.items()}
    N.check(lib.risvec_policy_sample(E, V, env_offset, h.data_ptr(), N.ptr(mk), tt.data_ptr(), hd.data_ptr(), None, None,
                                     seed, counter, floor, *(bufs[k].data_ptr() for k in shapes), st))
    torch.cuda.synchronize()
    out = {}
    for k, s in shapes.items():
        n = int(np.prod(s))
        assert bool((bufs[k][n:] == 12345.0).all()), "%s: written past its end" % k
        out[k] = cpu(bufs[k][:n]).reshape(s)
    return out


def oracle_sample(heads, mask, tau, hard, ids, call, seed, floor=0.1):
    """The epilogue on the same float32 heads with `philox_draws`: outputs and their bounds, [E,V,...]."""
    V, E, _ = heads.shape
    h = heads.astype(np.float64)
    eps, expo = PO.philox_draws(ids, V, call, seed)
    lvp = max(0, (V - 1).bit_length())
    r = {k: np.empty((E, V, n)) for k, n in (("power", 2), ("b_power", 2), ("probs", V), ("b_probs", V), ("onehot", V))}
    r["clear"] = np.empty((E, V), bool)
    for a in range(V):
        mu, ls, lg = h[a][:, 0:2], h[a][:, 2:4], h[a][:, 4:]
        m = None if mask is None else mask[:, a].astype(np.float64)
        t = float(np.float32(tau[a]))
        power, soft, onehot = PO.sample_heads(mu, ls, lg, m, t, eps[:, a], expo[:, a])
        r["power"][:, a], r["onehot"][:, a] = power, onehot
        r["probs"][:, a] = PO.sample_heads(mu, ls, lg, m, t, eps[:, a], expo[:, a], hard=True)[1] if hard[a] else soft
        r["clear"][:, a] = PO.top2_gap(soft) > 1e-4
        std = np.exp(np.clip(ls, -20.0, 2.0))
        r["b_power"][:, a] = std * DZ + 4 * U * (np.abs(eps[:, a]) * std + np.abs(mu)) + 2 * ULP
        ml = PO.mask_logits(lg, m)
        blocked = ml < -1e30
        g = -np.log(expo[:, a])
        z = (ml + g) / t
        dz = (ULP + ULP * np.abs(g) + U * np.abs(ml + g)) / t + U * np.abs(z) + U * np.abs(z - z.max(-1, keepdims=True))
        D = np.where(blocked, 0.0, dz).max(-1, keepdims=True)
        r["b_probs"][:, a] = 2 * D * soft * (1 - soft) + 4 * D * D + soft * (2 * ULP + (lvp + 1) * U) + 2 * FLT_MIN
        if hard[a]:                              # (1 - y) + y of the winner: two float32 roundings at <= 1
            r["b_probs"][:, a] = np.where(onehot > 0, ULP + U, 0.0)
    assert r["b_probs"].max() <= 2e-5, r["b_probs"].max()      # no wider than what the injected-draw golden test grants
    r["action_env"], r["p_off01"], store = marshal_actions(r["power"].astype(np.float32), r["probs"].astype(np.float32), floor)
    r["action_store"] = store.reshape(E, V, V + 2).astype(np.float64)
    b_env = (r["b_power"] + U) / 2 + U + 2e-9                  # cast, clip (1-Lipschitz), (x + 1) / 2; float32(floor)
    r["b_action_env"] = np.ascontiguousarray(b_env.transpose(0, 2, 1))
    r["b_p_off01"] = b_env[:, :, 0]
    r["b_action_store"] = np.concatenate([r["b_probs"] + U, r["b_power"] + U], axis=2)
    return r


def assert_sample(got, want, hard, what):
    """Values within their bounds on every row; one-hot (and with it the hard rows' winner) exact on the clear rows."""
    for k in got:
        assert np.isfinite(got[k]).all(), (what, k)
    clear = want["clear"]
    left_out = int((~clear).sum())
    print("[draws margin] %s: unclear rows left out %d of %d" % (what, left_out, clear.size))
    assert left_out <= 0.01 * clear.size
    hard_rows = np.broadcast_to(np.asarray(hard, bool)[None, :], clear.shape)
    judged = clear | ~hard_rows                                # a hard row is its arg-max: judged where that is clear
    worst = {}
    for k in ("power", "probs", "p_off01", "action_env", "action_store"):
        err, bound = np.abs(got[k].astype(np.float64) - want[k]), want["b_" + k]
        sel = np.ones(err.shape, bool)
        if k == "probs" or k == "action_store":
            sel[~judged] = False
        worst[k] = (err[sel] / np.maximum(bound[sel], 1e-300)).max()
        assert (err[sel] <= bound[sel]).all(), (what, k, np.argwhere(sel & (err > bound))[:5])
    print("[draws margin] %s: max err / bound %s" % (what, ", ".join("%s %.3f" % kv for kv in worst.items())))
    assert np.array_equal(got["onehot"][clear], want["onehot"][clear])
    assert np.array_equal(np.round(got["probs"])[clear & hard_rows], want["onehot"][clear & hard_rows])
    assert ((got["onehot"] == 0) | (got["onehot"] == 1)).all() and (got["onehot"].sum(-1) == 1).all()
    np.testing.assert_allclose(got["probs"].astype(np.float64).sum(-1), 1.0, atol=1e-5)
    # the marshalled outputs are those of the kernel's own power / probs, bit for bit (float32(floor) aside)
    m_env, m_p01, m_store = marshal_actions(got["power"], got["probs"], 0.1)
    assert np.array_equal(got["p_off01"].astype(np.float64), m_p01)
    assert np.array_equal(got["action_env"][:, 0].astype(np.float64), m_env[:, 0])
    np.testing.assert_allclose(got["action_env"][:, 1], m_env[:, 1], rtol=0, atol=2e-9)
    assert np.array_equal(got["action_store"].reshape(m_store.shape), m_store)


def policy_inputs(V, E, seed, masked=True):
    rng = np.random.default_rng(seed)
    heads = np.empty((V, E, 4 + V), np.float32)
    heads[..., 0:2] = rng.uniform(-1.5, 1.5, (V, E, 2))
    heads[..., 2:4] = rng.uniform(-3.0, 1.0, (V, E, 2))
    heads[..., 4:] = rng.uniform(-3.0, 3.0, (V, E, V))
    mask = None
    if masked:
        mask = (rng.uniform(size=(E, V, V)) < 0.7).astype(np.uint8)
        mask[:3] = 0                                           # all-zero rows are opened up
        mask[rng.integers(0, E, 5), rng.integers(0, V, 5)] = 0
    tau = rng.uniform(0.3, 2.0, V).astype(np.float32)
    hard = (np.arange(V) % 3 == 1).astype(np.uint8)
    return heads, mask, tau, hard


# (d) ------------------------------------------------------------------------------------------------------------
# E V ~ 2 000 rows; V = 20 / 33 / 64 run the VP = 32 / 64 instantiations and sub-sites up to 15
POLICY_SHAPES = [(1, 2001), (3, 667), (8, 251), (16, 125), (20, 101), (33, 63), (64, 63)]
NO_MASK = {(8, 7), (33, 1)}


@pytest.mark.parametrize("counter", [1, 7])
@pytest.mark.parametrize("V,E", POLICY_SHAPES)
def test_policy_sample_device_draws_vs_oracle(V, E, counter):
    heads, mask, tau, hard = policy_inputs(V, E, 100 * V + counter, masked=(V, counter) not in NO_MASK)
    got = sample_native(heads, mask, tau, hard, 77, counter, 4096)
    want = oracle_sample(heads, mask, tau, hard, np.arange(4096, 4096 + E), counter, 77)
    assert_sample(got, want, hard, "policy_sample V=%d E=%d call %d%s" % (V, E, counter, "" if mask is not None else " no mask"))
    if mask is not None:
        blocked = (mask == 0) & (mask.sum(-1, keepdims=True) > 0)
        assert (got["probs"][blocked] == 0.0).all()
        soft_agents = hard == 0                                 # an opened-up row gives every partner some probability
        assert ((got["probs"][:3] > 0) | (want["probs"][:3] < 1e-30))[:, soft_agents].all()


# (e) ------------------------------------------------------------------------------------------------------------
def test_batched_policy_owns_the_call_counter_and_the_env_offset():
    from ris_vec_marl_amd import BatchedPolicy
    V, E, cut, off = 8, 777, 300, 4096
    _, mask, tau, hard = policy_inputs(V, E, 5)
    obs = np.random.default_rng(6).uniform(0, 1.2, (E, V, 5)).astype(np.float32)

    def build(env_offset):
        pol = BatchedPolicy(V, 5, 64, 128, device=DEV, seed=13, env_offset=env_offset)
        with torch.no_grad():
            pol.Wh.mul_(100.0)
            pol.tau.copy_(T_(tau)); pol.gumbel_hard.copy_(T_(hard))
        return pol

    whole, lo, hi = build(off), build(off), build(off + cut)
    heads = cpu(whole.forward_heads(T_(obs)))
    for call in (1, 2):
        outs = [tuple(cpu(x) for x in pol.choose_action(T_(obs[s]), T_(mask[s]), cpu_share_floor=0.1))
                for pol, s in ((whole, slice(None)), (lo, slice(0, cut)), (hi, slice(cut, None)))]
        assert whole._calls == lo._calls == hi._calls == call
        names = ("power", "probs", "onehot", "action_env", "p_off01", "action_store")
        got = dict(zip(names, outs[0]))
        got["action_store"] = got["action_store"].reshape(E, V, V + 2)
        want = oracle_sample(heads, mask, tau, hard, np.arange(off, off + E), call, 13)
        assert_sample(got, want, hard, "BatchedPolicy.choose_action call %d" % call)
        for name, w, a, b in zip(names, *outs):                  # shards == the whole batch, bit for bit
            assert np.array_equal(w[:cut].view(np.uint32), a.view(np.uint32)), (name, call)
            assert np.array_equal(w[cut:].view(np.uint32), b.view(np.uint32)), (name, call)
        if call == 1:
            first = got["probs"].copy()
    assert not np.array_equal(first, got["probs"])


# (f) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocked", [False, True], ids=["open", "blocked"])
@pytest.mark.parametrize("env_id,agent,k", GUMBEL_ONES)
def test_gumbel_draw_with_u_equal_one(env_id, agent, k, blocked):
    """The Gumbel word with all-ones top 24 bits: Exp(1) = -ln(1) = 0 would be a Gumbel of +inf and a NaN row
    (inf - inf).  With torch's rule (2^-24 instead of 0) the lane wins at a Gumbel of 16.6 -- or, blocked, gets 0."""
    V, E = 8, 5
    heads, _, tau, hard = policy_inputs(V, E, 9, masked=False)
    hard[:] = 0
    mask = np.ones((E, V, V), np.uint8)
    if blocked:
        mask[2, agent, k] = 0
    ids = np.arange(env_id - 2, env_id + 3)
    want = oracle_sample(heads, mask, tau, hard, ids, GUMBEL_CALL, GUMBEL_SEED)
    assert PO.philox_draws(ids, V, GUMBEL_CALL, GUMBEL_SEED)[1][2, agent, k] == 2.0 ** -24
    if blocked:
        assert want["probs"][2, agent, k] == 0.0
    else:
        assert want["onehot"][2, agent, k] == 1.0 and want["clear"][2, agent]
    got = sample_native(heads, mask, tau, hard, GUMBEL_SEED, GUMBEL_CALL, env_id - 2)
    row = got["probs"][2, agent]
    assert np.isfinite(row).all(), row
    assert abs(float(row.astype(np.float64).sum()) - 1.0) <= 1e-5
    assert_sample(got, want, hard, "gumbel u == 1 at env %d agent %d k %d %s" % (env_id, agent, k, "blocked" if blocked else "open"))
    if blocked:
        assert row[k] == 0.0
    else:
        assert got["onehot"][2, agent, k] == 1.0
