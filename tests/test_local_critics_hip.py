"""GPU tests of every agent's local twin critics and local TD target (`BatchedLocalCritics`, `risvec_local_critics`,
csrc/k_local_critics.hip): `Agent.local_learn`'s target (Simulation-MARL-BCD/sac_agent.py:269-284) for all agents in one
MFMA launch, against vectors captured from the reference's own networks and target statements, against the global
kernel on the same weights (bit for bit: the net walk is the same code) and against a float64 restatement.

Error measure and bars are those of tests/marl_critic_ref.py: err = max over rows |q - q64| / max(max |q64|, 1e-3); err <
2e-5 in every mode; fused <= max(8 x the library mode's err on the same inputs, 1e-7).  The epilogue, against the q the
same launch wrote: |y - y64| <= 2^-22 (|r| + |gamma| (|m| + |c0 lp| + |c1 li|)) -- four float32 roundings (c0 lp, c1 li +
that, m - ent, live t + r; the product by live = (1 - done) gamma is exact on live rows up to gamma's own rounding, which
y64 shares) on terms no larger than that sum; a done row with a finite t equals the reward bit for bit.  Both modes also
equal the reference's statements evaluated in float32 operation by operation on the same q, bit for bit: the kernel's
epilogue contracts nothing into a fused multiply-add.
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import marl_critic_ref as R  # noqa: E402

DEV = "cuda:0"
SMALL = (96, 128, 128)                  # 3 fc1 groups over 4 wavefronts: one wavefront has none
DRIVER = (1024, 512, 256)
FIXTURES = ("local_critic_8", "local_critic_4")
NAN = float("nan")
FMIN2 = float(np.finfo(np.float32).min) / 2


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def agent_nets(V, hidden, seed, n_nets=2, A=None):
    """[agent][net] weight sets under the reference's key names."""
    dims = (5, V + 2 if A is None else A) + tuple(hidden)
    return [[R.random_net(dims, seed + 10 * j + c) for c in range(n_nets)] for j in range(V)]


def make(V, hidden, sds, gemm=None, n_nets=2, A=None):
    from ris_vec_marl_amd import BatchedLocalCritics
    c = BatchedLocalCritics(V, 5, A, *hidden, n_nets=n_nets, device=DEV, gemm=gemm)
    for j in range(V):
        c.load_agent_state_dict(j, *sds[j])
    return c


def explicit_batch(V, n, seed, A=None):
    A = V + 2 if A is None else A
    rng = np.random.default_rng(seed)
    obs = rng.uniform(0, 1.2, (n, V, 5)).astype(np.float32)
    act = rng.uniform(0, 1, (n, V, A)).astype(np.float32)
    return obs, act


def td_inputs(V, n, seed):
    rng = np.random.default_rng(seed)
    reward = rng.uniform(-6, 1, (n, V)).astype(np.float32)
    done = rng.uniform(size=n) < 0.25
    done[0] = True
    if n > 1:
        done[1] = False
    lp = rng.uniform(-8, 4, (n, V)).astype(np.float32)
    li = rng.uniform(-12, 0, (n, V)).astype(np.float32)
    coef = np.array([0.15, 0.06], np.float32)
    return reward, done, lp, li, coef


def target32(reward, q1, q2, done, gamma, coef=None, lp=None, li=None):
    """sac_agent.py:281-284 in float32, operation by operation as torch evaluates the statements (no fused multiply-add)"""
    f = np.float32
    m = q1.astype(f) if q2 is None else np.minimum(q1.astype(f), q2.astype(f))
    if lp is not None and li is not None:
        m = m - (f(coef[0]) * lp + f(coef[1]) * li)
    elif lp is not None:
        m = m - f(coef[0]) * lp
    elif li is not None:
        m = m - f(coef[1]) * li
    live = (f(1) - np.asarray(done, f)) * f(gamma)
    return (reward + live * m).astype(f)


def check_epilogue(y, q1, q2, reward, done, gamma, what, coef=None, lp=None, li=None):
    """y [V, n] against the float64 target per agent, built from the q [V, n] the same launch wrote."""
    g32 = float(np.float32(gamma))
    live = ~np.asarray(done, bool)
    worst = -np.inf
    for j in range(y.shape[0]):
        a = (None if lp is None else lp[:, j], None if li is None else li[:, j])
        q2j = None if q2 is None else q2[j]
        y64 = R.td_target64(reward[:, j], q1[j], q2j, done, g32, coef, *a)
        excess = np.abs(y[j].astype(np.float64) - y64) - R.y_bound(reward[:, j], q1[j], q2j, g32, coef, *a)
        assert np.isfinite(y[j][live]).all()
        if live.any():
            worst = max(worst, excess[live].max())
        assert np.array_equal(y[j][~live], reward[:, j][~live]), "%s: agent %d: a done row is not the reward" % (what, j)
        assert np.array_equal(y[j], target32(reward[:, j], q1[j], q2j, done, gamma, coef, *a)), \
            "%s: agent %d: y is not the reference's float32 statement on the q of the same launch" % (what, j)
    print("%s: epilogue, worst |y - y64| - bound = %.3g over %d live rows x %d agents" % (what, worst, live.sum(), y.shape[0]))
    assert worst <= 0


# ---------------------------------------------------------------------------------------------------- 1: the fixtures
def fixture_sds(fx):
    V = int(fx["V"])
    keys = R.KEYS
    return [[{k: fx["a%d.n%d.%s" % (j, c, k)] for k in keys} for c in (1, 2)] for j in range(V)]


@functools.lru_cache(maxsize=None)
def golden_run(name, mode):
    """(q1, q2, y) [V, B] of one fixture in one mode, from-policy form, as numpy; computed once and never modified."""
    fx = R.fixture(name)
    V, B = int(fx["V"]), int(fx["B"])
    hidden = tuple(int(fx[k]) for k in ("fc1", "fc2", "fc3"))
    critic = make(V, hidden, fixture_sds(fx), gemm=mode)
    assert critic.gemm == mode and critic.action_dims == int(fx["A"]) == V + 2
    q = tuple(torch.full((V, B, 1), NAN, device=DEV) for _ in range(2))
    y = critic.td_target(T(fx["reward_l"]), T(fx["obs_"]), T(fx["done"]), float(fx["gamma"]), heads=T(fx["heads"]),
                         power=T(fx["power"]), logp_power=T(fx["logp_power"]), logp_intent=T(fx["logp_intent"]),
                         coef=T(fx["coef"]), q=q)
    assert tuple(y.shape) == (V, B)
    if mode == "fused":
        from ris_vec_marl_amd import _native as N
        assert N.last_kernel().startswith("k_local_critics<1,1>x%d" % V)
    return tuple(t.cpu().numpy().reshape(V, B) for t in q) + (y.cpu().numpy(),)


@pytest.mark.parametrize("mode", ["fused", "library"])
@pytest.mark.parametrize("name", FIXTURES)
def test_vs_golden(name, mode):
    fx = R.fixture(name)
    V, B, done = int(fx["V"]), int(fx["B"]), fx["done"]
    q1, q2, y = golden_run(name, mode)
    l1, l2, _ = golden_run(name, "library")
    for j in range(V):
        for c, (got, lib) in enumerate(((q1, l1), (q2, l2))):
            want = fx["q%d" % (c + 1)][j]
            e, e_l = R.err(got[j], want), R.err(lib[j], want)
            print("%s %s: agent %d q%d vs the reference's float32 %.3g (library %.3g)" % (name, mode, j, c + 1, e, e_l))
            assert e < R.BAR
            if mode == "fused":
                assert e <= R.fused_bar(e_l)
    g32, coef = float(np.float32(fx["gamma"])), fx["coef"]
    worst = -np.inf
    for j in range(V):
        bound = R.y_bound(fx["reward_l"][:, j], fx["q1"][j], fx["q2"][j], g32, coef, fx["logp_power"][:, j], fx["logp_intent"][:, j])
        excess = np.abs(y[j].astype(np.float64) - fx["target"][j].astype(np.float64)) - bound
        worst = max(worst, excess[~done].max())
        assert np.array_equal(y[j][done], fx["reward_l"][:, j][done])          # bit for bit
    print("%s %s: target vs the reference's, worst |y - target| - bound = %.3g" % (name, mode, worst))
    assert worst <= 0
    check_epilogue(y, q1, q2, fx["reward_l"], done, float(fx["gamma"]), "%s %s" % (name, mode), coef, fx["logp_power"],
                   fx["logp_intent"])


# ---------------------------------------------------------------------------------------------------- 2: the global kernel
@functools.lru_cache(maxsize=None)
def pair_of_paths(V, hidden):
    """(local critics, [one BatchedTwinCritic(5, V + 2) per agent]) on the same weights, both fused; never modified."""
    from ris_vec_marl_amd import BatchedTwinCritic
    sds = agent_nets(V, hidden, 1000 * V)
    local = make(V, hidden, sds, gemm="fused")
    twins = []
    for j in range(V):
        t = BatchedTwinCritic(5, V + 2, *hidden, device=DEV, gemm="fused")
        t.load_state_dict(*sds[j])
        twins.append(t)
    return local, twins


def same_as_global(V, n, hidden):
    local, twins = pair_of_paths(V, hidden)
    obs, act = explicit_batch(V, n, 7 * V + n)
    obs_t, act_t = T(obs), T(act)
    q = local.forward(obs_t, act_t)
    assert len(q) == 2 and all(tuple(t.shape) == (V, n, 1) for t in q)
    for j, twin in enumerate(twins):
        want = twin.forward(obs_t[:, j].contiguous(), act_t[:, j].contiguous())
        for c in (0, 1):
            assert torch.isfinite(q[c][j]).all()
            assert torch.equal(bits(q[c][j]), bits(want[c])), "V=%d n=%d agent %d net %d differs from the global kernel" % (V, n, j, c + 1)
    return q


@pytest.mark.parametrize("n", [1, 33, 65])
@pytest.mark.parametrize("V", [2, 8, 9, 10, 16])
def test_same_arithmetic_as_the_global_kernel(V, n):
    """S + A = 7, 15 (one padded k-step), 16 (a full k-step), 17 (two k-steps), 23."""
    same_as_global(V, n, SMALL)
    from ris_vec_marl_amd import _native as N
    assert N.last_kernel().startswith("k_marl_critic<1,1>")


def test_same_arithmetic_at_the_drivers_sizes():
    from ris_vec_marl_amd import _native as N
    local, _ = pair_of_paths(8, DRIVER)
    same_as_global(8, 33, DRIVER)
    obs, act = explicit_batch(8, 33, 3)
    local.forward(T(obs), T(act))
    assert N.last_kernel() == "k_local_critics<4,2>x8x2"


# ---------------------------------------------------------------------------------------------------- 3: from the policy
def planted_heads(V, n, seed):
    """heads [V, n, 4 + V] with, per agent, row 0: the own logit is the largest; row 1: a tie between two other agents at
    the top; row 2: every other logit below finfo.min / 2, so the replaced own entry is the maximum."""
    rng = np.random.default_rng(seed)
    heads = rng.normal(0, 1.5, (V, n, 4 + V)).astype(np.float32)
    for j in range(V):
        lg = heads[j, :, 4:]
        lg[0, j] = lg[0].max() + 2.0
        a, b = [i for i in range(V) if i != j][1:3]           # two other agents, a < b, neither the first candidate
        lg[1, a] = lg[1, b] = np.float32(lg[1].max() + 1.0)
        lg[2, :] = np.float32(-3.0e38)
        lg[2, j] = 0.5
    return heads


def numpy_next_action(heads, power):
    """`sac_agent.py:270-274` in NumPy -> ([n, V, V + 2], idx [V, n])"""
    V, n = heads.shape[0], heads.shape[1]
    act = np.zeros((n, V, V + 2), np.float32)
    idx = np.zeros((V, n), np.int64)
    for j in range(V):
        lg = heads[j, :, 4:].copy()
        lg[:, j] = np.float32(FMIN2)
        idx[j] = lg.argmax(-1)                                # the first maximum
        act[np.arange(n), j, idx[j]] = 1.0
        act[:, j, V:] = power[:, j]
    return act, idx


@pytest.mark.parametrize("V", [4, 8, 16])
def test_from_policy_staging_equals_the_explicit_form(V):
    n = 35
    heads = planted_heads(V, n, V)
    rng = np.random.default_rng(V + 1)
    obs = rng.uniform(0, 1.2, (n, V, 5)).astype(np.float32)
    power = np.tanh(rng.normal(0, 1, (n, V, 2))).astype(np.float32)
    act, idx = numpy_next_action(heads, power)
    for j in range(V):
        a, b = [i for i in range(V) if i != j][1:3]
        assert idx[j, 0] != j and idx[j, 1] == a and idx[j, 2] == j
    reward, done, _, _, _ = td_inputs(V, n, 5)
    sds = agent_nets(V, SMALL, 300 + V)
    for mode in ("fused", "library"):
        critic = make(V, SMALL, sds, gemm=mode)
        q_pol = tuple(torch.full((V, n, 1), NAN, device=DEV) for _ in range(2))
        q_exp = tuple(torch.full((V, n, 1), NAN, device=DEV) for _ in range(2))
        y_pol = critic.td_target(T(reward), T(obs), T(done), 0.99, heads=T(heads), power=T(power), q=q_pol)
        y_exp = critic.td_target(T(reward), T(obs), T(done), 0.99, action_=T(act), q=q_exp)
        for c in (0, 1):
            assert torch.isfinite(q_pol[c]).all()
            assert torch.equal(bits(q_pol[c]), bits(q_exp[c])), "%s: net %d" % (mode, c + 1)
        assert torch.equal(bits(y_pol), bits(y_exp))


# ---------------------------------------------------------------------------------------------------- 4: the epilogue
@functools.lru_cache(maxsize=None)
def epilogue_critics(n_nets):
    V = 8
    sds = agent_nets(V, SMALL, 500, n_nets)
    return {mode: make(V, SMALL, sds, gemm=mode, n_nets=n_nets) for mode in ("fused", "library")}


@pytest.mark.parametrize("terms", ["both", "power", "intent", "none"])
@pytest.mark.parametrize("n_nets", [2, 1])
def test_epilogue_terms_and_caller_owned_outputs(n_nets, terms):
    V, n = 8, 37
    obs, act = explicit_batch(V, n, 11)
    reward, done, lp, li, coef = td_inputs(V, n, 12)
    lp = lp if terms in ("both", "power") else None
    li = li if terms in ("both", "intent") else None
    kw = dict(logp_power=None if lp is None else T(lp), logp_intent=None if li is None else T(li),
              coef=None if terms == "none" else T(coef))
    ys = {}
    for mode, critic in epilogue_critics(n_nets).items():
        # one guard row behind every output: nothing beyond [V, n] may be touched
        ybuf = torch.full((V + 1, n), NAN, device=DEV)
        qbuf = [torch.full((V + 1, n, 1), NAN, device=DEV) for _ in range(n_nets)]
        q = tuple(b[:V] for b in qbuf)
        y = critic.td_target(T(reward), T(obs), T(done), 0.99, action_=T(act), out=ybuf[:V], q=q if n_nets == 2 else q[0], **kw)
        assert y.data_ptr() == ybuf.data_ptr()
        for b in qbuf + [ybuf]:
            assert torch.isnan(b[V]).all() and torch.isfinite(b[:V]).all()
        qn = [b[:V].cpu().numpy().reshape(V, n) for b in qbuf]
        ys[mode] = y.cpu().numpy()
        check_epilogue(ys[mode], qn[0], qn[1] if n_nets == 2 else None, reward, done, 0.99, "%d nets %s %s" % (n_nets, terms, mode),
                       None if terms == "none" else coef, lp, li)
        fw = critic.forward(T(obs), T(act))
        fw = fw if n_nets == 2 else (fw,)
        assert all(torch.equal(bits(fw[c]), bits(qbuf[c][:V])) for c in range(n_nets))
    e = R.err(ys["fused"], ys["library"])
    print("%d nets %s: fused y vs library y %.3g" % (n_nets, terms, e))
    assert e < R.BAR


def test_done_row_with_infinite_logp_is_nan_in_both_modes():
    """The reference multiplies by (1 - done): 0 * inf is NaN (sac_agent.py:284), unlike the global target's select."""
    V, n = 8, 33
    obs, act = explicit_batch(V, n, 21)
    reward, done, lp, li, coef = td_inputs(V, n, 22)
    assert done[0] and not done[1]
    lp[0, 3] = np.inf                                         # a done row, agent 3
    lp[1, 5] = np.inf                                         # a live row, agent 5: t = -inf
    for mode, critic in epilogue_critics(2).items():
        y = critic.td_target(T(reward), T(obs), T(done), 0.99, action_=T(act), logp_power=T(lp), logp_intent=T(li),
                             coef=T(coef)).cpu().numpy()
        assert np.isnan(y[3, 0]), mode
        assert y[5, 1] == -np.inf, mode
        rest = np.ones_like(y, bool)
        rest[3, 0] = rest[5, 1] = False
        assert np.isfinite(y[rest]).all(), mode
        assert np.array_equal(y[:, done][rest[:, done]], reward.T[:, done][rest[:, done]]), mode


# ---------------------------------------------------------------------------------------------------- 5: weights in the loop
def device_sds(V, hidden, seed):
    return [[{k: T(v) for k, v in sd.items()} for sd in pair] for pair in agent_nets(V, hidden, seed)]


def test_shared_weights_rebuild_only_the_updated_agents_streams():
    from ris_vec_marl_amd import BatchedLocalCritics
    V, n, changed = 4, 33, 2
    sds = device_sds(V, SMALL, 700)
    obs, act = explicit_batch(V, n, 31)
    obs_t, act_t = T(obs), T(act)

    def shared(pack):
        critic = BatchedLocalCritics(V, 5, None, *SMALL, device=DEV, gemm="fused")
        critic.pack = pack
        for j in range(V):
            critic.share_agent_state_dict(j, *sds[j])
        assert critic.nets[1][0].W2.data_ptr() == sds[1][0]["fc2.weight"].data_ptr()
        return critic

    def streams_of(critic):
        return [[(bits(ws), bits(sc)) for ws, sc in pair] for pair in critic._fused_weights()]
    critic = shared("host")
    q0 = [t.clone() for t in critic.forward(obs_t, act_t)]
    assert critic.packs == 2 * V
    critic.forward(obs_t, act_t)
    assert critic.packs == 2 * V                              # nothing is stale
    before = streams_of(critic)
    for sd in sds[changed]:
        sd["fc2.weight"].mul_(1.01)                           # in place: seen through the version counter
    q1 = critic.forward(obs_t, act_t)
    assert critic.packs == 2 * V + 2                          # that agent's two streams, nobody else's
    after = streams_of(critic)
    for j in range(V):
        assert all(torch.equal(bits(q1[c][j]), bits(q0[c][j])) for c in (0, 1)) == (j != changed), j
        for c in (0, 1):
            assert torch.equal(after[j][c][0], before[j][c][0]) == (j != changed), (j, c)
    # pack="device": one two-launch pack per agent, the same bits as the host pack of the same tensors
    device = shared("device")
    qd = device.forward(obs_t, act_t)
    assert device.packs == 2 * V
    got = streams_of(device)
    for j in range(V):
        for c in (0, 1):
            assert torch.equal(got[j][c][0], after[j][c][0]) and torch.equal(got[j][c][1], after[j][c][1]), (j, c)
            assert torch.equal(bits(qd[c][j]), bits(q1[c][j]))
    buffers = [[ws.data_ptr() for ws, _ in pair] for pair in device._fused_weights()]
    sds[0][1]["fc3.weight"].mul_(0.99)
    device.forward(obs_t, act_t)
    assert device.packs == 2 * V + 1                          # one net of agent 0, into the buffer of its first rebuild
    assert buffers == [[ws.data_ptr() for ws, _ in pair] for pair in device._fused_weights()]


@pytest.mark.parametrize("agents", [None, 1])
def test_soft_update_is_the_references_statement_bit_for_bit(agents):
    V, tau = 4, 0.005
    target = make(V, SMALL, agent_nets(V, SMALL, 800), gemm="fused")
    online = device_sds(V, SMALL, 900)
    before = target.state_dict()
    obs, act = explicit_batch(V, 5, 41)
    target.forward(T(obs), T(act))
    packs = target.packs
    if agents is None:
        target.soft_update_from(None, online, tau)
    else:
        target.soft_update_from(agents, online[agents], tau)
    after = target.state_dict()
    for j in range(V):
        for c in (0, 1):
            for k in R.KEYS:
                a, b = online[j][c][k].cpu(), before[j][c][k]
                want = tau * a.clone() + (1 - tau) * b.clone() if agents in (None, j) else b      # sac_agent.py:305-312, on the CPU
                assert torch.equal(bits(after[j][c][k]), bits(want)), (j, c, k)
    target.forward(T(obs), T(act))
    assert target.packs == packs + 2 * (V if agents is None else 1)       # the blended nets were marked stale


# ---------------------------------------------------------------------------------------------------- 6: what is refused
def test_class_refuses_what_it_would_have_to_copy_or_convert():
    V, n = 8, 9
    critic = epilogue_critics(2)["fused"]
    obs, act = explicit_batch(V, n, 51)
    reward, done, lp, li, coef = td_inputs(V, n, 52)
    heads = T(np.zeros((V, n, 4 + V), np.float32))
    power = T(np.zeros((n, V, 2), np.float32))
    ok = dict(reward_l=T(reward), obs_=T(obs), done=T(done), gamma=0.99, action_=T(act), logp_power=T(lp), logp_intent=T(li),
              coef=T(coef))
    critic.td_target(**ok)
    wide = T(np.zeros((n, V, 10), np.float32))
    for bad in (dict(obs_=wide[:, :, :5]),                                     # a strided view
                dict(obs_=T(obs).double()), dict(obs_=T(obs).cpu()), dict(obs_=T(obs)[:, :4].contiguous()),
                dict(reward_l=T(reward).t().contiguous().t()), dict(reward_l=T(reward)[:, 0].contiguous()),
                dict(done=T(done).float()), dict(done=T(done)[:-1]),
                dict(action_=None), dict(heads=heads, power=power),            # neither form, both forms
                dict(action_=None, heads=heads), dict(power=power),            # heads without power, power without heads
                dict(action_=None, heads=heads[:, :, :-1].contiguous(), power=power),
                dict(logp_power=T(lp)[:, :1].contiguous()), dict(coef=None), dict(coef=T(coef).double()),
                dict(out=torch.empty(n, V, device=DEV)), dict(q=(torch.empty(V, n, 1, device=DEV),)),
                dict(gamma=float("inf"))):
        with pytest.raises(ValueError):
            critic.td_target(**dict(ok, **bad))
    with pytest.raises(ValueError):
        critic.forward(T(obs), T(act)[:, :, :-1].contiguous())
    from ris_vec_marl_amd import BatchedLocalCritics
    with pytest.raises(ValueError):
        BatchedLocalCritics(17, 5, None, *SMALL, device=DEV, gemm="fused")     # no fused kernel beyond 16 agents
    many = BatchedLocalCritics(17, 5, None, *SMALL, device=DEV)
    assert many.gemm == "library"
    odd = BatchedLocalCritics(V, 5, V + 3, *SMALL, device=DEV, gemm="fused")   # an explicit action of another width
    with pytest.raises(ValueError):
        odd.td_target(T(reward), T(obs), T(done), 0.99, heads=heads, power=power)      # heads needs action_dims == V + 2
    for call in (lambda: critic.load_agent_state_dict(V, {}, {}), lambda: critic.load_agent_state_dict(0, {}),
                 lambda: critic.soft_update_from(0, [{}], 0.5), lambda: critic.soft_update_from(None, [], 0.5)):
        with pytest.raises((ValueError, KeyError)):
            call()


def test_seeded_constructor_draws_the_same_weights_as_before():
    """`BatchedLocalCritics(seed=7)`: the draw loop as it stood in the constructor, restated literally on a CPU generator
    -- agent 0 net 1, agent 0 net 2, agent 1 net 1, ...; W1 b1 W2 b2 W3 b3 Wq bq inside a net -- bit for bit."""
    import math
    from ris_vec_marl_amd import BatchedLocalCritics
    V, S, A, F1, F2, F3 = 2, 3, 2, 32, 128, 128
    g = torch.Generator(device="cpu").manual_seed(7)

    def uni(*shape, r):
        return (torch.rand(*shape, generator=g) * 2 - 1) * r
    want = []
    for _ in range(V):
        pair = []
        for _ in range(2):
            sd = {}
            for name, fan_out, fan_in in (("fc1", F1, S + A), ("fc2", F2, F1), ("fc3", F3, F2), ("q", 1, F3)):
                r = 1.0 / math.sqrt(fan_in)
                sd[name + ".weight"] = uni(fan_out, fan_in, r=r)
                sd[name + ".bias"] = uni(fan_out, r=r)
            pair.append(sd)
        want.append(pair)
    got = BatchedLocalCritics(V, S, A, F1, F2, F3, seed=7).state_dict()
    assert [len(pair) for pair in got] == [2, 2]
    for pair, refs in zip(got, want):
        for sd, ref in zip(pair, refs):
            assert list(sd) == list(ref)
            for k in ref:
                assert sd[k].dtype == torch.float32 and torch.equal(sd[k], ref[k]), k
