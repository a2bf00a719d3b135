"""GPU tests of step() ON its branch edges (tests/step_edge_cases.py), with nothing masked out.

(a) the cached step `k_step<VP>` against the float64 oracle on the whole table, V in {3, 5, 8, 16}: `check_step` and the
    metrics / power / observation checks of test_step_golden with their tolerances and all-False masks, and on top bit
    equality wherever the table says exact;
(b) `log2_1p` against log2(1 + x), relative only, over 2^-40 ... 2^40 and the 17 floats around its switch at 0.0625;
(c) every launch form of the fused step carries the same edge states: the form runs, the gain it wrote goes into a twin env
    and the cached step on the twin must leave the same bits in everything a step writes -- (a) ties the cached side to
    the oracle.  Gains of exactly 0 (a zero theta, a zero fading power) and exact ties (two paired vehicles at one
    position) are made by construction inside every form;
(d) the SARL step on its own edges (Bn > 0, over_data > 2, the all-zero row) through `sarl_step` and the rollout launch.

The dyadic parameter set of the table makes the device (float32) and the oracle (float64) decide every comparison from
the same numbers; tests/test_step_edges_host.py checks the table itself."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import risvec_oracle as orc  # noqa: E402  (checker)
from tests import step_edge_cases as T  # noqa: E402
from tests.test_hip_parity import (RT, check_step, check_step_outputs, cpu, make_vec, record, set_params,  # noqa: E402
                                   step_mask)
from tests.test_step_edges_host import step_mask as host_step_mask  # noqa: E402
from tests.test_theta_index_step_hip import STEP_KEYS  # noqa: E402

DEV = "cuda:0"
VS = [3, 5, 8, 16]


def _N():
    from ris_vec_marl_amd import _native as N
    return N


def apply_params(env, p):
    set_params(env, p)
    env.time_fast = p.time_fast


def tolerance_params(p):
    """The parameter set `check_step` takes its scales from.  It divides by cpu_share_floor (the delay scale
    B 1000 Cpb / (floor f_local_max)), so a floor that is NaN, infinite or outside [0, 0.95] is replaced by the one in
    force (ENV:574-577); where that is 0 the base floor 0.125 stands in: every vehicle of those cases has a share of at
    least 0.25 but vehicle 0, whose reward is the clip's and asserted exactly."""
    fl = orc.effective_floor(p.cpu_share_floor)
    return dataclasses.replace(p, cpu_share_floor=fl if fl > 0 else T.BASE["cpu_share_floor"])


def dev(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x).astype(dt)).to(DEV)


def run_cached(b, V, policy_action=False, action=None):
    """one cached-gain step of batch `b` on a fresh env -> (env, out)"""
    env = make_vec(b.E, V, 16)
    apply_params(env, b.params)
    t = env.tensors
    t["data_buf"].copy_(dev(b.data_buf0, np.float32)); t["mec_q"].copy_(dev(b.mec_q0, np.float32))
    t["gain"].copy_(dev(b.gain, np.float32))
    out = env.step(dev(b.action if action is None else action, np.float32), dev(b.partner, np.int32),
                   dev(b.n_groups, np.int32), dev(b.arrivals, np.int32), fused=False, policy_action=policy_action)
    assert _N().last_kernel() == "k_step<%d>" % (1 << (V - 1).bit_length()), _N().last_kernel()
    return env, out


def same_bits(got, want):
    """float32 device values equal the float32 image of the oracle's, compared as values (-0 == +0)"""
    return np.array_equal(np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float64).astype(np.float32))


# ---------------------------------------------------------------------------- (a) the cached step against the oracle
@pytest.mark.parametrize("V", VS)
def test_cached_step_on_the_edges_vs_oracle(V):
    ratios, runs = {}, []
    # ---- every batch runs and every figure (error / asserted tolerance per output) is printed before anything is asserted
    for b in T.batches(V):
        pt = tolerance_params(b.params)
        env, out = run_cached(b, V)
        t = env.tensors
        o = b.oracle()
        runs.append((b, pt, env, out, o))
        B0 = b.data_buf0
        kb = np.maximum(B0, 1.0)
        d_scale = B0 * 1000 * pt.cycles_per_bit / (pt.cpu_share_floor * pt.f_local_max)
        for key, got, ref, tol in (
                ("rate", cpu(t["rate"]), o["vehicle_rate"], 1e-7 + RT * np.abs(o["vehicle_rate"])),
                ("data_t", cpu(t["data_t"]), o["data_t"], 1e-7 + RT * np.abs(o["data_t"])),
                ("data_p", cpu(t["data_p"]), o["data_p"], 1e-7 + RT * np.abs(o["data_p"])),
                ("data_buf", cpu(out[2]), o["data_buf"], RT * o["data_buf"] + 4e-7 * kb),
                ("over_power", cpu(t["over_power"]), o["over_power"], 1e-6 + RT * np.abs(o["over_power"])),
                ("reward", cpu(out[0]), o["reward"], RT * np.abs(o["reward"]) + 4e-7 * pt.w_d * d_scale + 1e-9),
                ("mec_q", cpu(t["mec_q"]), o["mec_q"], RT * o["mec_q"] + 1e-6 * pt.f_edge_max * pt.time_fast)):
            r = np.abs(got - ref) / tol
            ratios[key] = max(ratios.get(key, 0.0), float(r.max()))
            for at in np.argwhere(r > 1)[:4]:
                name = [c.name for c, sl in zip(b.cases, b.slices) if sl.start <= at[0] < sl.stop][0]
                print("[edge] V=%d %s %r: %s at %s is %r, the oracle has %r (%.3g of its tolerance)"
                      % (V, name, b.over, key, at, got[tuple(at)], ref[tuple(at)], r[tuple(at)]))
    for key, r in ratios.items():
        record("edges (a) V=%d %s: worst error / asserted tolerance" % (V, key), r)
    worst_metrics = 0.0
    for b, pt, env, out, o in runs:
        t = env.tensors
        B0 = b.data_buf0
        for mine, theirs in zip(host_step_mask(o, b.partner, b.gain, b.mec_q0), step_mask(o, b.partner, b.gain, b.mec_q0)):
            assert np.array_equal(mine, theirs)                 # the host test judged the table with the same mask
        none = np.zeros((b.E, V), dtype=bool)
        what = [c.name for c in b.cases]
        okr = check_step(env, out, o, B0, pt, none, none)
        assert okr.all(), what
        worst_metrics = max(worst_metrics, float(check_step_outputs(env, out, o["metrics"][:, :14], o["last_power_W"], B0, pt, okr)))
        # ---- bit for bit wherever the table says exact
        for key, got, ref in (("data_p", cpu(t["data_p"]), o["data_p"]), ("data_buf", cpu(out[2]), o["data_buf"]),
                              ("reward", cpu(out[0]), o["reward"]), ("rate", cpu(t["rate"]), o["vehicle_rate"]),
                              ("mec_q", cpu(t["mec_q"]), o["mec_q"])):
            m = b.mask(key)
            assert same_bits(got[m], ref[m]), (what, key, got[m], ref[m])
        # the violation slot: count / V, the count exact (v_rcp_f32 and the product: 1.5 ulp of the quotient)
        m = b.mask("viol")
        n_viol = o["viol"].sum(axis=1).astype(np.float64)
        slot = cpu(t["metrics"])[:, 11].astype(np.float64)
        assert np.array_equal(np.rint(slot * V)[m], n_viol[m]), (what, slot * V, n_viol)
        assert (np.abs(slot * V - n_viol) <= 2.0 ** -22 * n_viol)[m].all()
        if V in (8, 16):
            assert np.array_equal(slot[m], (n_viol / V)[m])
    record("edges (a) V=%d metrics: worst error above the floor / 1e-5" % V, worst_metrics / RT)


@pytest.mark.parametrize("V", [5, 8])
def test_facade_passes_every_floor_to_the_kernel(V):
    """The Python facade refuses no cpu_share_floor: NaN, +inf, -1 and 2 reach the kernel as they are (params.to_c), and
    ENV:574-577 runs there -- asserted by (a); here: the C struct holds the value given."""
    env = make_vec(2, V, 16)
    for fl in (float("nan"), float("inf"), -1.0, 0.0, 0.95, 2.0):
        env.cpu_share_floor = fl
        got = float(env._p().cpu_share_floor)
        assert (np.isnan(got) and np.isnan(fl)) or got == float(np.float32(fl))


# ---------------------------------------------------------------------------- (b) log2_1p
def test_log2_1p_relative_error():
    """|rate - log2(1 + x)| <= 1e-5 log2(1 + x), no absolute floor: pw0 == 1, gain = x 2^-46 and n_groups = 1 make the rate
    log2_1p(x) itself.  The worst ratio overall and among the 17 floats around the switch of formula are recorded."""
    V = 8
    c = [x for x in T.cases(V) if x.name == "log2_1p"][0]
    b = T.batches(V, [c])[0]
    env, _ = run_cached(b, V)
    x = c.meta["x"]
    ref = np.log1p(x) / np.log(2.0)
    rate = cpu(env.tensors["rate"]).astype(np.float64)
    rel = np.abs(rate - ref) / ref
    sw = c.meta["at_switch"]
    record("log2_1p: worst relative error, x = 2^-40 ... 2^40 and the switch", rel.max())
    record("log2_1p: worst relative error among the 17 floats around x = 0.0625", rel[sw].max())
    record("log2_1p: worst relative error below the switch (series)", rel[x < 0.0625].max())
    record("log2_1p: worst relative error from the switch on (v_log_f32)", rel[x >= 0.0625].max())
    assert (np.abs(rate - ref) <= RT * ref).all(), (x[rel > RT], rel[rel > RT])
    # what the two formulas can give.  The series: its first dropped term x^5 / 6 <= 1.6e-7 and five fused steps.
    assert rel[x < 0.0625].max() < 1e-6
    # v_log_f32(1 + x): the sum is rounded to float32 first, an error of up to 2^-24 (1 + x) in the argument and so of
    # 2^-24 / ln(1 + x) relative to the result -- 9.8e-7 at the switch -- plus the instruction's own ulp and the
    # result's rounding (2^-22 together)
    assert (rel <= 2.0 ** -24 / np.log1p(x) + 2.0 ** -22)[x >= 0.0625].all()


# ---------------------------------------------------------------------------- (c) every launch form
def edge_state(V, with_zero_theta=True):
    """The base-parameter cases of the table as the state of a real env: (inputs dict, tie envs, zero-gain envs).  The
    table's own gains are not used -- a fused form computes them; two extra copies of the first envs get a zero theta."""
    b = T.batches(V)[0]
    assert b.over == {}
    tie = [sl for c, sl in zip(b.cases, b.slices) if c.name == "noma/tie"][0]
    keys = ("data_buf0", "mec_q0", "action", "partner", "n_groups", "arrivals")
    inp = {k: getattr(b, k) for k in keys}
    zero = []
    if with_zero_theta:
        pick = [tie.start, tie.start + 1, 0]                     # the two tie listings and the local-clear env, at gain 0
        inp = {k: np.concatenate([v, v[pick]]) for k, v in inp.items()}
        zero = list(range(b.E, b.E + len(pick)))
    return inp, list(range(tie.start, tie.stop)), zero


def real_env(V, M, inp, tie, zero, seed=9, model=None):
    E = inp["data_buf0"].shape[0]
    env = make_vec(E, V, M, seed=seed)
    apply_params(env, T.dyadic_params())
    if model:
        env.channel_model = model
    env.make_new_game(); env.renew_positions()
    pos = env.tensors["pos"]
    pos[tie, 1, :] = pos[tie, 0, :]                              # the paired vehicles 0 and 1 at one position
    env.compute_parms()
    env.Random_phase()
    if zero:
        env.tensors["theta"][zero] = 0.0                         # a write through torch: the step reads the tensor
    load_state(env, inp)
    return env


def load_state(env, inp):
    env.tensors["data_buf"].copy_(dev(inp["data_buf0"], np.float32))
    env.tensors["mec_q"].copy_(dev(inp["mec_q0"], np.float32))


def step_args(inp):
    return (dev(inp["action"], np.float32), dev(inp["partner"], np.int32), dev(inp["n_groups"], np.int32),
            dev(inp["arrivals"], np.int32))


def check_gains(env, tie, zero, what):
    g = env.tensors["gain"]
    gi = g.contiguous().view(torch.int32)
    assert torch.equal(gi[tie, 0], gi[tie, 1]), (what, "the co-located vehicles' gains differ")
    assert bool((g[tie, 0] > 0).all()), what
    if zero:
        assert bool((g[zero] == 0).all()), (what, "a zero theta gives a gain of exactly 0")


def twin_of(env, V, M, inp, gain, n_steps=1, actions=None, arrivals=None, policy_action=False, power_w=True):
    """the cached step on a fresh env holding `gain`: what every form must equal bit for bit"""
    N = _N()
    twin = make_vec(inp["data_buf0"].shape[0], V, M, seed=9)
    apply_params(twin, T.dyadic_params())
    load_state(twin, inp)
    twin.tensors["gain"].copy_(gain)
    a, pt, ng, ar = step_args(inp)
    snaps = []
    for k in range(n_steps):
        twin.step(a if actions is None else actions[k], pt, ng, ar if arrivals is None else arrivals[k], fused=False,
                  metrics=True, obs=True, power_w=power_w, policy_action=policy_action)
        assert N.last_kernel() == "k_step<%d>" % (1 << (V - 1).bit_length()), N.last_kernel()
        snaps.append({k2: twin.tensors[k2].clone() for k2 in ("reward", "obs", "metrics")})
    return twin, snaps


def assert_same(a, b, what, keys=STEP_KEYS):
    for k in keys:
        x, y = a.tensors[k], b.tensors[k]
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), \
            (what, k, int((x != y).sum()), "words differ")


LAUNCHED = {}


def note(form, shape, name):
    LAUNCHED.setdefault(form, set()).add(name)
    print("[edge forms] %-24s %-10s %s" % (form, shape, name))


# form -> (forced fields, touch h_r, heads, expected name (prefix, suffix), rebuilt, groups per wave > 1)
SINGLE_FORMS = [
    ("lat by rule", (8, 64), {}, False, True, ("k_step_fused_lat<8,64,", ">"), None),
    ("lat by rule", (4, 16), {}, False, True, ("k_step_fused_lat<4,16,", ">"), None),
    ("pipe", (8, 64), dict(lat=False, pipe_nt=False), True, True, ("k_step_fused_pipe<8,64,", "MarlCore>"), 0),
    ("pipe", (16, 256), dict(lat=False, pipe_nt=False), True, True, ("k_step_fused_pipe<16,256,", "MarlCore>"), 0),
    ("pipe NT", (8, 64), dict(lat=False, pipe_nt=True), True, True, ("k_step_fused_pipe<8,64,", "MarlCore,NT>"), 0),
    ("pipe NT", (16, 256), dict(lat=False, pipe_nt=True), True, True, ("k_step_fused_pipe<16,256,", "MarlCore,NT>"), 0),
    ("GEN one-group, heads", (8, 64), dict(lat=False, pipe_nt=False), False, True, ("k_step_fused_pipe<8,64,", "MarlCore>"), 1),
    ("GEN one-group, sincospi", (8, 64), dict(lat=False, pipe_nt=False), False, False, ("k_step_fused_pipe<8,64,", "MarlCore>"), 1),
    ("GEN loop, heads", (8, 64), dict(lat=False, pipe_nt=False, pipe_waves=2), False, True, ("k_step_fused_pipe<8,64,", "MarlCore>"), 2),
    ("GEN loop, sincospi", (8, 64), dict(lat=False, pipe_nt=False, pipe_waves=2), False, False, ("k_step_fused_pipe<8,64,", "MarlCore>"), 2),
    ("GEN one-group, heads", (16, 64), dict(lat=False, pipe_nt=False), False, True, ("k_step_fused_pipe<16,64,", "MarlCore>"), 1),
    ("GEN one-group, sincospi", (16, 64), dict(lat=False, pipe_nt=False), False, False, ("k_step_fused_pipe<16,64,", "MarlCore>"), 1),
    ("GEN loop, heads", (16, 64), dict(lat=False, pipe_nt=False, pipe_waves=2), False, True, ("k_step_fused_pipe<16,64,", "MarlCore>"), 2),
    ("GEN loop, sincospi", (16, 64), dict(lat=False, pipe_nt=False, pipe_waves=2), False, False, ("k_step_fused_pipe<16,64,", "MarlCore>"), 2),
    ("generic k_step_fused", (5, 21), {}, False, True, ("k_step_fused<", ">"), None),
]


@pytest.mark.parametrize("form,shape,force,touch,heads,name,gen", SINGLE_FORMS,
                         ids=["%s-%dx%d" % (f[0].replace(" ", "_"), f[1][0], f[1][1]) for f in SINGLE_FORMS])
def test_single_step_forms_carry_the_edges(form, shape, force, touch, heads, name, gen):
    N = _N()
    V, M = shape
    inp, tie, zero = edge_state(V)
    env = real_env(V, M, inp, tie, zero)
    if touch:
        env.tensors["h_r"].mul_(1)                               # ends the permission to rebuild the rows: the reading form
    if not heads:
        env.steer_heads = False
    with N.forced(**force):
        env.step(*step_args(inp), fused=True, metrics=True, obs=True, power_w=True)
        kern = N.last_kernel()
        rebuilt, hd, gpw = N.last_h_r_rebuilt(), N.last_h_r_heads(), N.last_gen_groups_per_wave()
    note(form, shape, kern)
    assert kern.startswith(name[0]) and kern.endswith(name[1]), kern
    assert N.last_theta_by_index() == 0
    if gen is not None:
        assert rebuilt == (1 if gen else 0), (form, rebuilt)
        if gen:
            assert hd == (1 if heads else 0), (form, hd)
            assert (gpw == 1) if gen == 1 else (gpw > 1), (form, gpw)
    check_gains(env, tie, zero, form)
    twin, _ = twin_of(env, V, M, inp, env.tensors["gain"])
    assert_same(env, twin, (form, shape))


@pytest.mark.parametrize("V,M", [(8, 64), (16, 64)])
def test_theta_by_index_form_carries_the_edges(V, M):
    """Random_phase() leaves the indices current and the pipeline reads them (no zero theta here: an index has none)."""
    N = _N()
    inp, tie, _ = edge_state(V, with_zero_theta=False)
    env = real_env(V, M, inp, tie, [])
    with N.forced(lat=False, pipe_nt=False):
        env.step(*step_args(inp), fused=True, metrics=True, obs=True, power_w=True)
        kern, by_index = N.last_kernel(), N.last_theta_by_index()
    note("theta by index", (V, M), kern)
    assert by_index == 1 and kern.startswith("k_step_fused_pipe<%d,%d," % (V, M)) and kern.endswith("MarlCore>"), kern
    check_gains(env, tie, [], "theta by index")
    twin, _ = twin_of(env, V, M, inp, env.tensors["gain"])
    assert_same(env, twin, ("theta by index", V, M))


@pytest.mark.parametrize("V,M,fused", [(8, 64, True), (4, 16, True), (5, 21, True), (8, 64, False), (5, 21, False)])
def test_t_step_launches_carry_the_edges(V, M, fused):
    """step_many, T = 2: the first step's records and the state after the second against two cached steps of the twin (the
    second step starts from the first's state, on the same edges' partners and parameters)."""
    N = _N()
    inp, tie, zero = edge_state(V)
    env = real_env(V, M, inp, tie, zero)
    a, pt, ng, ar = step_args(inp)
    actions = torch.stack([a, (a * 0.75).contiguous()])
    arrivals = torch.stack([ar, (ar + 1) % 3])
    if not fused:
        env.update_channel_gains()
    want = N.step_kernel(env._cstate, 0, N.FORM_FUSED_MULTI) if fused else None
    rec = env.step_many(actions, pt, ng, arrivals, metrics=True, obs=True, fused=fused)
    kern = N.last_kernel()
    note("step_fused_multi" if fused else "step_multi", (V, M), kern)
    assert kern == (want if want is not None else "k_step_multi<%d>" % (1 << (V - 1).bit_length())), (kern, want)
    check_gains(env, tie, zero, kern)
    twin, snaps = twin_of(env, V, M, inp, env.tensors["gain"], n_steps=2, actions=[actions[0].clone(), actions[1].clone()],
                          arrivals=[arrivals[0].clone(), arrivals[1].clone()], power_w=False)
    for t in range(2):
        for k in ("reward", "obs", "metrics"):
            assert torch.equal(rec[k][t].contiguous().view(torch.int32), snaps[t][k].contiguous().view(torch.int32)), (t, k)
    assert_same(env, twin, kern, [k for k in STEP_KEYS if k != "power_w"])


@pytest.mark.parametrize("V,M", [(8, 64), (4, 16)])
def test_ring_form_carries_the_edges(V, M):
    """bind_step_store(fused=True) takes the raw policy output: power_raw = 2 a - 1 maps back onto the table's action
    wherever that lies inside the policy's range (the clip and the floor move the rest: still valid states)."""
    from ris_vec_marl_amd import VecReplayBuffer
    N = _N()
    inp, tie, zero = edge_state(V)
    E = inp["data_buf0"].shape[0]
    env = real_env(V, M, inp, tie, zero)
    raw = dev(np.transpose(2.0 * inp["action"] - 1.0, (0, 2, 1)), np.float32)
    _, pt, ng, ar = step_args(inp)
    probs = torch.softmax(torch.randn(E, V, V, device=DEV, generator=torch.Generator(DEV).manual_seed(3)), -1)
    buf = VecReplayBuffer(2 * E, 5, V + 2, V, device=DEV)
    launch = env.bind_step_store(buf, raw, pt, ng, probs, None, ar, fused=True, power_w=True)
    with N.forced(pipe_nt=False):
        launch(done=False, use_mask=False)
        kern = N.last_kernel()
    note("ring", (V, M), kern)
    assert kern.startswith("k_step_fused_pipe<%d,%d," % (V, M)) and kern.endswith("MarlCore+ring>"), kern
    check_gains(env, tie, zero, kern)
    twin, _ = twin_of(env, V, M, inp, env.tensors["gain"], actions=[raw], policy_action=True)
    assert_same(env, twin, kern)
    # the ring's row of this step holds the step's own rewards and observation
    assert torch.equal(buf.reward_local_memory[:E].reshape(E, V), env.tensors["reward"])
    assert torch.equal(buf.reward_global_memory[:E].reshape(E), env.tensors["metrics"][:, 0])
    assert torch.equal(buf.new_state_memory[:E].reshape(E, V, 5), env.tensors["obs"])


@pytest.mark.parametrize("V,M", [(8, 16), (5, 21)])
def test_fused_3gpp_form_carries_the_edges(V, M):
    """Injected fading: the co-located pair gets the same three draws (an exact tie), a small-scale power of 0 a gain of
    exactly 0."""
    N = _N()
    inp, tie, zero = edge_state(V)
    E = inp["data_buf0"].shape[0]
    env = real_env(V, M, inp, tie, zero, model="3gpp_umi")
    g = torch.Generator(DEV).manual_seed(17)
    u, z = torch.rand(E, V, device=DEV, generator=g), torch.randn(E, V, device=DEV, generator=g)
    sm = -torch.log1p(-torch.rand(E, V, device=DEV, generator=g))
    for x in (u, z, sm):
        x[tie, 1] = x[tie, 0]
    sm[zero] = 0.0
    env.step(*step_args(inp), fused=True, metrics=True, obs=True, power_w=True, fading=(u, z, sm))
    kern = N.last_kernel()
    note("fused 3GPP", (V, M), kern)
    assert kern == "k_step_3gpp<%d>" % (1 << (V - 1).bit_length()), kern
    check_gains(env, tie, zero, kern)
    twin, _ = twin_of(env, V, M, inp, env.tensors["gain"])
    assert_same(env, twin, kern)


@pytest.mark.parametrize("V,M", [(8, 64), (5, 21)])
def test_step_fused_bcd_carries_the_edges(V, M):
    """step(bcd=True): the sweep replaces theta (the zero-theta envs included), so only the ties are made by construction."""
    N = _N()
    inp, tie, _ = edge_state(V, with_zero_theta=False)
    env = real_env(V, M, inp, tie, [])
    env.step(*step_args(inp), fused=True, bcd=True, metrics=True, obs=True, power_w=True)
    kern = N.last_kernel()
    note("step_fused_bcd", (V, M), kern)
    assert kern.startswith("k_step_fused"), kern
    check_gains(env, tie, [], kern)
    twin, _ = twin_of(env, V, M, inp, env.tensors["gain"])
    assert_same(env, twin, kern)


# ---------------------------------------------------------------------------- (d) SARL
def _sarl_env(E, V, M):
    env = make_vec(E, V, M, seed=21)
    env.make_new_game()
    env.compute_parms()
    return env


def _sarl_check(t, o, B0, power, E):
    """tolerances of test_sarl_step_golden, nothing left out"""
    np.testing.assert_allclose(cpu(t["rate"]), o["vehicle_rate"], rtol=RT, atol=1e-7)
    np.testing.assert_allclose(cpu(t["data_t"]), o["data_t"], rtol=RT, atol=1e-7)
    np.testing.assert_allclose(cpu(t["data_p"]), o["data_p"], rtol=RT, atol=1e-7)
    kb = np.maximum(B0, 1.0)
    assert (np.abs(cpu(t["data_buf"]) - o["data_buf"]) <= RT * o["data_buf"] + 4e-7 * kb).all()
    assert (np.abs(cpu(t["over_data"]) - o["over_data"]) <= RT * o["over_data"] + 4e-7 * kb).all()
    p1 = power[:, 1, :]
    proc = np.where(o["over_data"] > 0, p1 - o["over_power"], 0.0)
    assert (np.abs(cpu(t["over_power"]) - o["over_power"]) <= RT * np.maximum(p1, proc) + 3e-6 * proc + 1e-7).all()
    sp = orc.SarlParams()
    assert (np.abs(cpu(t["reward"]) - o["reward"]) <= RT * np.abs(o["reward"]) + sp.t_factor2 * 4e-7 * kb + 1e-7).all()
    r_floor = sp.t_factor2 * (4e-7 * kb).mean(axis=1) + 1e-7
    assert (np.abs(cpu(t["metrics"][:, 0]) - o["reward_mean"]) <= RT * np.abs(o["reward_mean"]) + r_floor).all()


OFFSETS = (2.0, 0.5, -1.0, -2.75)


def _sarl_rows(env, phase, power, sp):
    """Backlogs around the two branches of SENV:344-352 for envs 1 ... 4 (env 0 keeps B = 0): with `spent` = data_t +
    data_p of a vehicle -- from the gains the device computes for `phase` ahead of the step, in float64 -- B = spent + 2
    and spent + 0.5 (Bn > 0: penalty 1), spent - 1 (no penalty: over_data = 1 <= 2), spent - 2.75 (over_data = 2.75 > 2:
    penalty 2; every vehicle processes 3.4 kbit or more locally, so B stays positive).  Margins of 0.5 kbit, against a gain that may move in its last bits between the two launches."""
    env.get_next_phase(phase)
    env.update_channel_gains()
    g = cpu(env.tensors["gain"]).astype(np.float64)
    rate = np.log(1 + power[:, 0, :] * g / orc.SIGMA ** 2)
    spent = rate * sp.time_fast * sp.bandwidth * 1000 + np.cbrt(power[:, 1, :] / sp.k) * sp.time_fast / sp.L / 1000
    B0 = np.zeros_like(spent)
    for e, off in enumerate(OFFSETS, start=1):
        B0[e] = spent[e] + off
    assert (B0 >= 0).all()
    return B0.astype(np.float32).astype(np.float64)


def _sarl_margins(o):
    assert (np.abs(o["margin"]["buf"][1:]) > 0.4).all() and (np.abs(o["margin"]["over"][1:]) > 0.4).all()
    assert (o["margin"]["buf"][1:3] > 0).all() and (o["margin"]["buf"][3:] < 0).all()
    assert (o["over_data"][3] < 2).all() and (o["over_data"][4] > 2).all()


@pytest.mark.parametrize("V,M", [(8, 40), (4, 16), (5, 21)])
def test_sarl_step_on_its_edges(V, M):
    sp = orc.SarlParams()
    E = 5
    env = _sarl_env(E, V, M)
    t = env.tensors
    power = np.zeros((E, 2, V))
    power[1:, 0, :] = 0.25
    power[1:, 1, :] = 1.0                                       # data_p = 4.31 kbit
    power[1:, 1, 0] = 0.5
    phase = np.linspace(0.1, 6.0, E * M, dtype=np.float32).reshape(E, M)
    B0 = _sarl_rows(env, phase, power, sp)
    t["data_buf"].copy_(dev(B0, np.float32))
    arr = np.zeros((E, V), dtype=np.int32)
    arr[1:] = np.arange(V) % 3
    env.sarl_step(power.astype(np.float32), phase, arr)
    o = orc.sarl_step(B0, cpu(t["gain"]).astype(np.float64), power, arr, sp)
    _sarl_margins(o)
    _sarl_check(t, o, B0, power, E)
    # the all-zero row: Bn == 0 is neither branch
    for k in ("reward", "over_power", "over_data", "rate", "data_t", "data_p", "data_buf"):
        assert bool((t[k][0] == 0).all()), k
    assert float(t["metrics"][0, 0]) == 0.0
    # row 3 pays no penalty, row 4 penalty 2 and both leave an empty buffer: the reward is the powers' sum exactly
    rew = cpu(t["reward"]).astype(np.float64)
    assert np.array_equal(rew[3], -power[3].sum(axis=0)) and np.array_equal(rew[4], -power[4].sum(axis=0) - sp.penalty2)


@pytest.mark.parametrize("V,M", [(8, 40), (4, 16)])
def test_sarl_rollout_on_its_edges(V, M):
    """The rollout launch maps mu through clip(+-0.999) and (a + 1) / 2, so its lowest power is 0.0005, not 0: row 0 is the
    lowest the launch can reach (B = 0, more processed than there was), the other rows are placed as for `sarl_step`."""
    from ris_vec_marl_amd import sarl_action_map
    N = _N()
    sp = orc.SarlParams()
    E = 5
    env = _sarl_env(E, V, M)
    t = env.tensors
    mu = np.zeros((E, 2 * V + M), dtype=np.float32)
    mu[0, :2 * V] = -1.0                                         # p0 = p1 = 0.0005
    mu[1:, :V] = -0.5                                            # p0 = 0.25
    mu[1:, V:2 * V] = 0.5                                        # p1 = 0.75: data_p = 3.9 kbit
    mu[:, 2 * V:] = np.linspace(-0.9, 0.9, E * M, dtype=np.float32).reshape(E, M)
    pw, ph = sarl_action_map(dev(mu, np.float32), V, M)
    power = cpu(pw).astype(np.float64)
    B0 = _sarl_rows(env, ph, power, sp)
    t["data_buf"].copy_(dev(B0, np.float32))
    arr = np.zeros((E, V), dtype=np.int32)
    arr[1:] = np.arange(V) % 3
    action, phase, _ = env.sarl_rollout(mu, arrivals=arr)
    assert N.last_kernel().startswith("k_sarl_rollout"), N.last_kernel()
    assert torch.equal(phase, ph) and np.array_equal(cpu(action), np.clip(mu, np.float32(-0.999), np.float32(0.999)))
    o = orc.sarl_step(B0, cpu(t["gain"]).astype(np.float64), power, arr, sp)
    _sarl_margins(o)
    assert (o["margin"]["buf"][0] < 0).all() and (o["over_data"][0] < 1.5).all()
    _sarl_check(t, o, B0, power, E)
    assert bool((t["data_buf"][0] == 0).all())                   # more processed than there was: an empty buffer


def test_forms_that_ran():
    """Printed last: every form of (c) and the kernels it launched (when the whole module ran)."""
    for form in sorted(LAUNCHED):
        print("[edge forms] %s: %s" % (form, ", ".join(sorted(LAUNCHED[form]))))
