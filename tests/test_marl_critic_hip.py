"""GPU tests of the SAC twin global critic and its TD target (`BatchedTwinCritic`, `risvec_marl_critic`,
csrc/k_marl_critic.hip): the reference's two `CriticNetwork.forward` (Simulation-MARL-BCD/networks.py:38-49), the minimum,
the entropy term and the target of `global_learn` (global_sac_critic.py:339-352) in one MFMA launch, against vectors
captured from the reference's own networks and target statements and against a float64 restatement
(tests/marl_critic_ref.py).

Error measure: err = max over rows |q - q64| / max(max over the batch |q64|, 1e-3) -- batch-wide, because a single q can
cancel to near zero.  Bars (the project's, tests/sarl_critic_ref.py):
  * err < 2e-5 in every mode;
  * fused: err <= max(8 x the library mode's err on the same inputs, 1e-7).
The epilogue, against the q1 / q2 the same launch wrote: |y - y64| <= 2^-22 (|r| + |gamma| (|m| + |c0 lp| + |c1 li|)) --
at most four float32 roundings (c0 lp, the fused c1 li + that, m - ent, the fused gamma . + r) on terms no larger than
that sum; rows with `done` equal the reward bit for bit.
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import marl_critic_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DRIVER = {4: (20, 24, 1024, 512, 256), 8: (40, 80, 1024, 512, 256)}
SMALL = (40, 80, 96, 256, 256)          # 3 fc1 groups over 4 wavefronts, 2 tiles per wavefront in fc2 and fc3
NAN = float("nan")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def make(dims, sds=None, gemm=None, n_nets=2, seed=0):
    from ris_vec_marl_amd import BatchedTwinCritic
    S, A, F1, F2, F3 = dims
    c = BatchedTwinCritic(S, A, F1, F2, F3, n_nets=n_nets, device=DEV, seed=seed, gemm=gemm)
    if sds is not None:
        c.load_state_dict(*sds)
    return c


def np_sds(critic):
    return [{k: v.numpy() for k, v in sd.items()} for sd in critic.state_dict()]


def run(critic, x, a, mode):
    """(q1, q2) [n] of `critic` in `mode` on device tensors, as numpy; one array in a list when n_nets == 1."""
    was, critic.gemm = critic.gemm, mode
    try:
        out = tuple(torch.full((x.shape[0], 1), NAN, device=DEV) for _ in range(critic.n_nets))
        q = critic.forward(x, a, out=out if critic.n_nets == 2 else out[0])
        q = q if critic.n_nets == 2 else (q,)
        assert all(t.data_ptr() == o.data_ptr() for t, o in zip(q, out))
    finally:
        critic.gemm = was
    return [t.cpu().numpy().reshape(-1) for t in q]


def check_bars(critic, x, a, what):
    """Both modes against the float64 restatement on the same inputs, both bars of the module docstring."""
    sds = np_sds(critic)
    q_f, q_l = run(critic, x, a, "fused"), run(critic, x, a, "library")
    refs = []
    for c, sd in enumerate(sds):
        ref64 = R.critic_q64(sd, x.cpu().numpy(), a.cpu().numpy())
        e_f, e_l = R.err(q_f[c], ref64), R.err(q_l[c], ref64)
        print("%s: q%d err fused %.3g library %.3g (ratio %.2f), max |q64| %.3g"
              % (what, c + 1, e_f, e_l, e_f / max(e_l, 1e-30), np.abs(ref64).max()))
        assert e_l < R.BAR and e_f < R.BAR
        assert e_f <= R.fused_bar(e_l)
        refs.append(ref64)
    return q_f, refs


def check_epilogue(y, q1, q2, reward, done, gamma, what, coef=None, lp=None, li=None):
    """y against the float64 target built from the q1 / q2 the same launch wrote (gamma and coef as the float32 values the
    kernel receives)"""
    g32 = float(np.float32(gamma))
    y = np.asarray(y, np.float64).reshape(-1)
    y64 = R.td_target64(reward, q1, q2, done, g32, coef, lp, li)
    live = ~np.asarray(done, bool)
    excess = np.abs(y - y64) - R.y_bound(reward, q1, q2, g32, coef, lp, li)
    print("%s: epilogue, worst |y - y64| - bound = %.3g over %d live rows" % (what, excess[live].max() if live.any() else NAN, live.sum()))
    assert np.isfinite(y[live]).all() and (excess[live] <= 0).all()
    assert np.array_equal(y[~live], np.asarray(reward, np.float64)[~live])


@functools.lru_cache(maxsize=None)
def driver_critic(V):
    """The driver's sizes with weights in the reference's initialisation ranges, q widened to +-0.4.  Shared and never
    modified: tests that update weights build their own."""
    return make(DRIVER[V], [R.random_net(DRIVER[V], 41), R.random_net(DRIVER[V], 42)], gemm="fused")


@functools.lru_cache(maxsize=None)
def small_critic():
    return make(SMALL, [R.random_net(SMALL, 51), R.random_net(SMALL, 52)], gemm="fused")


def batch(dims, n, seed, V=None, zero_row0=True):
    s, a = R.random_batch(dims, n, seed, V, zero_row0)
    return T(s), T(a)


def td_inputs(n, seed, inf_on_done=False):
    rng = np.random.default_rng(seed)
    reward = rng.uniform(-6, 1, n).astype(np.float32)
    done = rng.uniform(size=n) < 0.25
    done[0] = True
    done[1:2] = False
    lp = rng.uniform(-8, 4, n).astype(np.float32)
    li = rng.uniform(-12, 0, n).astype(np.float32)
    if inf_on_done:
        lp[0] = np.inf
    coef = np.array([0.15, 0.06], np.float32)
    return reward, done, lp, li, coef


# ---------------------------------------------------------------------------------------------------- 1: the fixtures
@pytest.mark.parametrize("mode", ["fused", "library"])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_vs_golden(name, mode):
    fx = R.fixture(name)
    V, B = int(fx["V"]), int(fx["B"])
    dims = tuple(int(fx[k]) for k in ("S", "A", "fc1", "fc2", "fc3"))
    sds = [R.weights_of(fx, 1), R.weights_of(fx, 2)]
    critic = make(dims, sds, gemm=mode)
    assert critic.gemm == mode
    x, a = T(fx["state_"].reshape(B, V, 5)), T(fx["action_"].reshape(B, V, V + 2))     # the learner's views: read in place
    q64 = [R.critic_q64(sd, fx["state_"], fx["action_"]) for sd in sds]
    q = critic.forward(x, a)
    assert len(q) == 2 and all(tuple(t.shape) == (B, 1) for t in q)
    for c in (0, 1):
        e_gold, e_64 = R.err(q[c].cpu().numpy(), fx["q%d" % (c + 1)]), R.err(q[c].cpu().numpy(), q64[c])
        print("%s %s: q%d vs the reference's float32 %.3g, vs float64 %.3g" % (name, mode, c + 1, e_gold, e_64))
        assert e_gold < R.BAR and e_64 < R.BAR
    gamma, done, reward = float(fx["gamma"]), T(fx["done"]), T(fx["reward"])
    for branch in ("single", "separate"):
        coef = fx["coef_" + branch]
        q_own = (torch.full((B, 1), NAN, device=DEV), torch.full((B, 1), NAN, device=DEV))
        y = critic.td_target(reward, x, a, done, gamma, logp_power=T(fx["logp_power"]), logp_intent=T(fx["logp_intent"]),
                             coef=T(coef), q=q_own)
        y64 = R.td_target64(fx["reward"], q64[0], q64[1], fx["done"], gamma, coef, fx["logp_power"], fx["logp_intent"])
        e_y, e_y64 = R.err(y.cpu().numpy(), fx["target_" + branch]), R.err(y.cpu().numpy(), y64)
        e_q = [R.err(q_own[c].cpu().numpy(), fx["q%d" % (c + 1)]) for c in (0, 1)]
        print("%s %s %s-alpha: target vs the reference's %.3g, vs float64 %.3g; Q_c(s', a') vs the reference's %.3g %.3g"
              % (name, mode, branch, e_y, e_y64, e_q[0], e_q[1]))
        assert tuple(y.shape) == (B,) and e_y < R.BAR and e_y64 < R.BAR and max(e_q) < R.BAR
        assert torch.equal(y[done], reward[done])                 # bit for bit
        assert all(torch.equal(q_own[c], q[c]) for c in (0, 1))
        if mode == "fused":
            check_epilogue(y.cpu().numpy(), q_own[0].cpu().numpy(), q_own[1].cpu().numpy(), fx["reward"], fx["done"], gamma,
                           "%s %s" % (name, branch), coef, fx["logp_power"], fx["logp_intent"])
    if mode == "fused":
        check_bars(critic, x, a, name)


# ---------------------------------------------------------------------------------------------------- 2: driver sizes
@pytest.mark.parametrize("V", sorted(DRIVER))
def test_driver_sizes_vs_float64(V):
    critic = driver_critic(V)
    x, a = batch(DRIVER[V], 257, 7, V)
    _, refs = check_bars(critic, x, a, "driver V=%d x 257" % V)
    for ref in refs:
        assert np.abs(ref).max() > 0.3
    from ris_vec_marl_amd import _native as N
    assert N.last_kernel().startswith("k_marl_critic<4,2>")


# ---------------------------------------------------------------------------------------------------- 3: row counts
@pytest.mark.parametrize("n", [1, 33, 65, 129, 257])
def test_row_counts_and_sentinels(n):
    """Partly filled tiles and more than one workgroup; row 0 all zero; rows beyond n keep their NaN sentinel."""
    critic = small_critic()
    x, a = batch(SMALL, n, 100 + n, 8)
    assert not x[0].any() and not a[0].any()
    q_f, refs = check_bars(critic, x, a, "small x %d" % n)
    pad = 40
    buf = [torch.full((n + pad, 1), NAN, device=DEV) for _ in range(3)]
    ybuf = torch.full((n + pad,), NAN, device=DEV)
    out = critic.forward(x, a, out=(buf[0][:n], buf[1][:n]))
    reward, done, lp, li, coef = td_inputs(n, n)
    y = critic.td_target(T(reward), x, a, T(done), 0.99, T(lp), T(li), T(coef), out=ybuf[:n], q=(buf[2][:n], buf[0][:n]))
    assert y.data_ptr() == ybuf.data_ptr()
    for b in buf + [ybuf]:
        assert torch.isnan(b[n:]).all() and torch.isfinite(b[:n]).all()
    assert np.array_equal(out[1].cpu().numpy().reshape(-1), q_f[1]) and np.array_equal(buf[2][:n].cpu().numpy().reshape(-1), q_f[0])
    assert np.array_equal(buf[0][:n].cpu().numpy().reshape(-1), q_f[1])        # the second td_target buffer holds q2
    y64 = R.td_target64(reward, refs[0], refs[1], done, 0.99, coef, lp, li)
    e_y = R.err(y.cpu().numpy(), y64)
    print("small x %d: target vs float64 %.3g" % (n, e_y))
    assert e_y < R.BAR


# ---------------------------------------------------------------------------------------------------- 4: net isolation
@pytest.mark.parametrize("dims", [SMALL, DRIVER[4]])
def test_each_net_is_computed_on_its_own(dims):
    sds = [R.random_net(dims, 61), R.random_net(dims, 62)]
    x, a = batch(dims, 70, 9, None)
    singles = [run(make(dims, [sd], gemm="fused", n_nets=1), x, a, "fused")[0] for sd in sds]
    for order in ((0, 1), (1, 0)):
        q = run(make(dims, [sds[order[0]], sds[order[1]]], gemm="fused"), x, a, "fused")
        assert np.array_equal(q[0], singles[order[0]]) and np.array_equal(q[1], singles[order[1]]), order
    assert not np.array_equal(singles[0], singles[1])


# ---------------------------------------------------------------------------------------------------- 5: the epilogue
def test_epilogue_forms():
    n = 97
    x, a = batch(SMALL, n, 21, 8)
    # at the initialisation ranges the q biases make one net the minimum almost everywhere (as the fixtures' capture found):
    # net 2's q bias is set so that the median of q1 - q2 over these rows is 0, and min() has both outcomes
    sds = np_sds(small_critic())
    q0 = run(small_critic(), x, a, "fused")
    sds[1]["q.bias"] = sds[1]["q.bias"] + np.float32(np.median(q0[0] - q0[1]))
    critic = make(SMALL, sds, gemm="fused")
    reward, done, lp, li, coef = td_inputs(n, 5, inf_on_done=True)
    assert done[0] and np.isinf(lp[0])
    tr, td, tlp, tli, tc = T(reward), T(done), T(lp), T(li), T(coef)

    def q_pair():
        return (torch.full((n, 1), NAN, device=DEV), torch.full((n, 1), NAN, device=DEV))
    # reward = 0, gamma = 1, no entropy: y is min(q1, q2) bit for bit on live rows
    q = q_pair()
    y = critic.td_target(torch.zeros(n, device=DEV), x, a, td, 1.0, q=q)
    live = ~td
    assert torch.equal(y[live], torch.minimum(q[0], q[1]).view(n)[live]) and not y[td].any()
    both = (torch.minimum(q[0], q[1]) == q[0]).float().mean()
    print("epilogue: q1 is the minimum on %.0f %% of %d rows" % (100 * float(both), n))
    assert 0.3 < float(both) < 0.7
    # the general form, each logp present or absent; done as uint8 and logp as [n, 1]
    for what, kw, ref in (("both", dict(logp_power=tlp, logp_intent=tli, coef=tc), dict(coef=coef, lp=lp, li=li)),
                          ("power only", dict(logp_power=tlp.view(n, 1), coef=tc), dict(coef=coef, lp=lp)),
                          ("intent only", dict(logp_intent=tli, coef=tc.view(1, 2)), dict(coef=coef, li=li)),
                          ("neither", dict(), dict()), ("neither, coef given", dict(coef=tc), dict())):
        q = q_pair()
        y = critic.td_target(tr, x, a, td.to(torch.uint8), 0.97, q=q, **kw)
        check_epilogue(y.cpu().numpy(), q[0].cpu().numpy(), q[1].cpu().numpy(), reward, done, 0.97, "epilogue " + what, **ref)
        assert float(y[0]) == float(reward[0])                # the done row with logp = +inf
    # one net: m = q1
    one = make(SMALL, [R.random_net(SMALL, 51)], gemm="fused", n_nets=1)
    q1 = torch.full((n, 1), NAN, device=DEV)
    y = one.td_target(tr, x, a, td, 0.97, tlp, tli, tc, q=q1)
    check_epilogue(y.cpu().numpy(), q1.cpu().numpy(), None, reward, done, 0.97, "epilogue one net", coef=coef, lp=lp, li=li)
    y0 = one.td_target(torch.zeros(n, device=DEV), x, a, td, 1.0, q=q1)
    assert torch.equal(y0[live], q1.view(n)[live])
    assert isinstance(one.forward(x, a), torch.Tensor)
    # the library mode computes the same target to the bar
    q = q_pair()
    yf = critic.td_target(tr, x, a, td, 0.97, tlp, tli, tc, q=q)
    lib = make(SMALL, np_sds(critic), gemm="library")
    yl = lib.td_target(tr, x, a, td, 0.97, tlp, tli, tc)
    e = R.err(yl.cpu().numpy()[~done], yf.cpu().numpy()[~done])
    print("epilogue: library against fused target %.3g" % e)
    assert e < R.BAR and torch.equal(yl[td], tr[td])


# ---------------------------------------------------------------------------------------------------- 6: refused shapes
def test_sixteen_vehicles_take_the_library_path():
    from ris_vec_marl_amd import BatchedTwinCritic
    dims = (80, 288, 1024, 512, 256)
    with pytest.raises(ValueError):
        BatchedTwinCritic(*dims, device=DEV, gemm="fused")
    critic = make(dims, [R.random_net(dims, 71), R.random_net(dims, 72)])
    assert critic.gemm == "library"
    x, a = batch(dims, 65, 3, 16)
    q = critic.forward(x, a)
    for c, sd in enumerate(np_sds(critic)):
        e = R.err(q[c].cpu().numpy(), R.critic_q64(sd, x.cpu().numpy(), a.cpu().numpy()))
        print("16 vehicles, library: q%d err %.3g" % (c + 1, e))
        assert e < R.BAR
    reward, done, lp, li, coef = td_inputs(65, 8)
    y = critic.td_target(T(reward), x, a, T(done), 0.99, T(lp), T(li), T(coef))
    assert torch.equal(y[T(done)], T(reward)[T(done)]) and torch.isfinite(y).all()


# ---------------------------------------------------------------------------------------------------- 7: weights in the loop
def test_shared_weights_repack_on_update():
    dims = SMALL
    sds = [{k: T(v) for k, v in R.random_net(dims, s).items()} for s in (81, 82)]
    critic = make(dims, gemm="fused")
    critic.share_state_dict(*sds)
    x, a = batch(dims, 70, 4, 8)
    critic.forward(x, a)
    critic.forward(x, a)
    assert critic.packs == 2                                  # one pack per net, reused
    sds[1]["fc2.weight"].add_(0.01)
    q = critic.forward(x, a)
    assert critic.packs == 3                                  # only the net that changed
    for c in (0, 1):
        ref = R.critic_q64({k: v.cpu().numpy() for k, v in sds[c].items()}, x.cpu().numpy(), a.cpu().numpy())
        e = R.err(q[c].cpu().numpy(), ref)
        print("after add_: q%d err %.3g" % (c + 1, e))
        assert e < R.BAR
    sds[0]["q.bias"].add_(1.0)                                # not part of the stream: read in place, no repack
    q2 = critic.forward(x, a)
    assert critic.packs == 3 and torch.allclose(q2[0], q[0] + 1.0, atol=1e-5)
    critic.mark_stale()
    critic.forward(x, a)
    assert critic.packs == 5


@pytest.mark.parametrize("tau", [0.005, 1.0])
def test_soft_update_is_the_references_statement(tau):
    dims = (20, 24, 64, 128, 128)
    target = make(dims, [R.random_net(dims, 91), R.random_net(dims, 92)], gemm="fused")
    online = [{k: T(v) for k, v in R.random_net(dims, s).items()} for s in (93, 94)]
    x, a = batch(dims, 33, 6, 4)
    target.forward(x, a)
    packs = target.packs
    before = target.state_dict()
    target.soft_update_from(*online, tau=tau)
    after = target.state_dict()
    n_checked = 0
    for c in (0, 1):
        for k in R.KEYS:
            want = tau * online[c][k].cpu() + (1 - tau) * before[c][k]         # global_sac_critic.py:398, on the CPU
            assert torch.equal(after[c][k], want), (c, k)
            n_checked += 1
    assert n_checked == 16
    q = target.forward(x, a)                                  # marked stale: both streams are rebuilt
    assert target.packs == packs + 2
    for c in (0, 1):
        e = R.err(q[c].cpu().numpy(), R.critic_q64({k: v.numpy() for k, v in after[c].items()}, x.cpu().numpy(), a.cpu().numpy()))
        print("after soft update tau=%g: q%d err %.3g" % (tau, c + 1, e))
        assert e < R.BAR
    # a refused argument changes nothing
    bad = dict(online[1])
    bad["fc3.weight"] = online[1]["fc3.weight"].double()
    for args, kw, exc in (((online[0], bad), dict(tau=0.5), ValueError), ((online[0],), dict(tau=0.5), ValueError),
                          ((online[0], online[1]), dict(tau=1.5), ValueError),
                          ((online[0], {k: v for k, v in online[1].items() if k != "q.bias"}), dict(tau=0.5), KeyError)):
        with pytest.raises(exc):
            target.soft_update_from(*args, **kw)
    again = target.state_dict()
    assert all(torch.equal(again[c][k], after[c][k]) for c in (0, 1) for k in R.KEYS)
    other = make(dims, [R.random_net(dims, 95), R.random_net(dims, 96)], gemm="fused")
    target.soft_update_from(other, tau=1.0)                   # another BatchedTwinCritic as the online pair
    assert all(torch.equal(target.state_dict()[c][k], other.state_dict()[c][k]) for c in (0, 1) for k in R.KEYS)


# ---------------------------------------------------------------------------------------------------- 8: inputs in place
def test_inputs_are_read_in_place_or_refused():
    from ris_vec_marl_amd import VecReplayBuffer
    V, n = 8, 64
    critic = driver_critic(V)
    memory = VecReplayBuffer(256, 5, V + 2, V, device=DEV, seed=3)
    s, a = R.random_batch(DRIVER[V], 200, 13, V, zero_row0=False)
    s2, _ = R.random_batch(DRIVER[V], 200, 14, V, zero_row0=False)
    rng = np.random.default_rng(2)
    memory.store_batch(T(s), T(a), T(rng.uniform(-6, 1, 200).astype(np.float32)), T(rng.uniform(-6, 1, (200, V)).astype(np.float32)),
                       T(s2), False, torch.ones(200, V, V, dtype=torch.bool, device=DEV))
    states, actions, rewards_g, _, states_, dones, _ = memory.sample_buffer(n)
    q_flat = critic.forward(states_, actions)
    q_view = critic.forward(states_.view(n, V, 5), actions.view(n, V, V + 2))
    assert all(torch.equal(q_flat[c], q_view[c]) for c in (0, 1))
    y1 = critic.td_target(rewards_g, states_.view(n, V, 5), actions.view(n, V, V + 2), dones, 0.99)
    y2 = critic.td_target(rewards_g, states_, actions, dones, 0.99)
    assert torch.equal(y1, y2)                                # two identical calls give identical bits
    reward, done, lp, li, coef = td_inputs(n, 1)
    ok = dict(reward=rewards_g, state_=states_, action_=actions, done=dones, gamma=0.99, logp_power=T(lp), logp_intent=T(li), coef=T(coef))
    wide = torch.zeros(n, 2 * DRIVER[V][0], device=DEV)
    for k, v in (("state_", states_.double()), ("state_", wide[:, ::2]), ("action_", actions.double()),
                 ("action_", actions[:, :-1]), ("action_", actions.t().contiguous().t()), ("reward", rewards_g.double()),
                 ("reward", rewards_g[:-1]), ("done", dones.float()), ("logp_power", T(lp).double()),
                 ("logp_intent", torch.zeros(n, 2, device=DEV)[:, 0]), ("coef", None), ("coef", T(coef).double()),
                 ("coef", T(coef).cpu()), ("gamma", float("nan")), ("out", torch.zeros(n, 1, device=DEV)),
                 ("q", (torch.zeros(n, 1, device=DEV),)), ("q", (torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)))):
        with pytest.raises(ValueError):
            critic.td_target(**dict(ok, **{k: v}))
    with pytest.raises(ValueError):
        critic.forward(states_, actions, out=torch.zeros(n, 1, device=DEV))
    y3 = critic.td_target(**ok)
    assert torch.isfinite(y3).all() and torch.equal(y3, critic.td_target(**ok))


# ---------------------------------------------------------------------------------------------------- 9: the example
def test_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "marl_td_target.py"), "256", "1"], capture_output=True,
                         text=True, timeout=240, cwd=ROOT)
    print(out.stdout[-1500:], out.stderr[-1500:])
    assert out.returncode == 0
    assert "mean target" in out.stdout


def test_seeded_constructor_draws_the_same_weights_as_before():
    """`BatchedTwinCritic(seed=7)`: the draw loop as it stood in the constructor, restated literally on a CPU generator --
    net 1 then net 2, W1 b1 W2 b2 W3 b3 Wq bq inside a net -- bit for bit."""
    import math
    from ris_vec_marl_amd import BatchedTwinCritic
    S, A, F1, F2, F3 = 3, 2, 32, 128, 128
    g = torch.Generator(device="cpu").manual_seed(7)

    def uni(*shape, r):
        return (torch.rand(*shape, generator=g) * 2 - 1) * r
    want = []
    for _ in range(2):
        sd = {}
        for name, fan_out, fan_in in (("fc1", F1, S + A), ("fc2", F2, F1), ("fc3", F3, F2), ("q", 1, F3)):
            r = 1.0 / math.sqrt(fan_in)
            sd[name + ".weight"] = uni(fan_out, fan_in, r=r)
            sd[name + ".bias"] = uni(fan_out, r=r)
        want.append(sd)
    got = BatchedTwinCritic(S, A, F1, F2, F3, seed=7).state_dict()
    assert len(got) == 2
    for sd, ref in zip(got, want):
        assert list(sd) == list(ref)
        for k in ref:
            assert sd[k].dtype == torch.float32 and torch.equal(sd[k], ref[k]), k
