"""GPU sweep of the five learner-side MFMA kernels -- `k_marl_critic<MT2,MT3>` (BatchedTwinCritic), `k_sarl_critic<MT2,MT3>`
(BatchedCritic), `k_sarl_actor<MT,KS>` (BatchedActor), `k_marl_critic_wide<MT2,MT3>` (BatchedTwinCritic(gemm="wide")) and
`k_local_critics<MT2,MT3>` (BatchedLocalCritics) -- over every template instantiation and every edge of their
run-time parameters (tests/mlp_sweep_shapes.py names the edge each case is there for): clamped prefetch, wavefronts
without work, all-zero k-steps, the bias row at a k-step boundary, partly filled head tiles, the > 64 KiB dynamic-LDS
attribute path; for the wide kernel the chunk walk (a last chunk below, on and past a prefetch block, uneven groups per
wavefront, the state / action boundary on and inside a chunk); for the local critics the agent count's limits, the
per-agent net table and the one-hot built from the policy's heads.  The other test_*_hip.py files of these kernels stay
at the driver's sizes and the fixtures.

Per case, against the float64 restatement of the reference's network (tests/marl_critic_ref.py, tests/sarl_critic_ref.py,
`forward64` of test_sarl_actor_hip.py) and with the bars of those files, imported and not restated (BAR = 2e-5 in both
modes, fused <= max(8 x library, 1e-7), the actor's sigmoid check):
  * the library dispatches to the instantiation the table names (`_native.last_kernel()`);
  * 70 rows (critics: two full 32-row tiles and one of 6) or 161 rows (actor: a full 128-row workgroup, a full
    wavefront and one row), row 0 all zero, both modes under the bars;
  * outputs written into buffers 40 rows longer keep their sentinel beyond n and hold the same bits as before;
  * the same call on row 0 alone writes the bits that row 0 of the long call got (rows are independent; the launch
    with one mostly empty tile);
  * a second object with pack="device" and the same weights returns the bits pack="host" returned (the `k_*_pack`
    kernels at the same edges);
  * critics: one `td_target` through the epilogue check of the kernel's own test file;
  * wide: each net of the twin launch is, bit for bit, a one-net launch holding its weights (the second net restages
    the input and reuses the accumulators); the device pack's stream and scales are the host pack's; the shape inside
    the fused rule gives `k_marl_critic`'s bits;
  * local: every agent has its own weights and is judged against float64 on its own columns, and equals, bit for bit, a
    fused `BatchedTwinCritic(S, A)` holding its weights; the target also equals the reference's float32 statements;
    with A = V + 2 the from-policy form equals the explicit form of the action NumPy builds from the same heads.
Weights in the reference's initialisation ranges; every shape's float32-against-float64 error and, where fc1 <= 160,
the NumPy walk of the packed stream are checked at these very inputs without a GPU by test_mlp_sweep_host.py.
Every figure is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import marl_critic_ref as MR  # noqa: E402
from tests import mlp_sweep_shapes as SW  # noqa: E402
from tests import sarl_critic_ref as R  # noqa: E402
from tests import test_local_critics_hip as TL  # noqa: E402
from tests import test_marl_critic_hip as TM  # noqa: E402
from tests import test_marl_critic_wide_hip as TW  # noqa: E402
from tests import test_sarl_actor_hip as TA  # noqa: E402
from tests import test_sarl_critic_hip as TC  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = -7.0
T = TM.T


def last_kernel():
    from ris_vec_marl_amd import _native as N
    return N.last_kernel()


def bits(t):
    """A float32 tensor or array as int32 bit patterns (numpy): equality that tells -0 from 0 and compares NaN."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def sentinel_buffers(n, *tails):
    return [torch.full((n + SW.PAD,) + tail, SENTINEL, device=DEV) for tail in tails]


def kept(buf, n):
    return bool((buf[n:] == SENTINEL).all()) and bool(torch.isfinite(buf[:n]).all())


# ------------------------------------------------------------------------------------------------------- MARL critic
@pytest.mark.parametrize("index,n_nets", SW.MARL_CRITIC_RUNS,
                         ids=["%s-x%d" % (SW.case_id(SW.MARL_CRITIC[i]), k) for i, k in SW.MARL_CRITIC_RUNS])
def test_marl_critic(index, n_nets):
    case = SW.MARL_CRITIC[index]
    dims, n = case.dims, SW.CRITIC_ROWS
    w_seed, b_seed = SW.seeds("marl", index)
    sds = [MR.random_net(dims, w_seed + c) for c in range(n_nets)]
    what = "marl %s x%d" % (SW.case_id(case), n_nets)
    critic = TM.make(dims, sds, gemm="fused", n_nets=n_nets)
    assert critic.gemm == "fused" and critic.pack == "host"
    x, a = TM.batch(dims, n, b_seed)
    assert tuple(x.shape) == (n, dims[0]) and tuple(a.shape) == (n, dims[1]) and not x[0].any() and not a[0].any()
    q_f, refs = TM.check_bars(critic, x, a, what)             # both modes, both bars; prints fused and library err
    assert all(np.abs(ref).max() > 0.05 for ref in refs)      # a q layer of +-0.4 on live features: not a zero output

    # the long call into longer buffers: the instantiation, the same bits, the tail untouched
    big = sentinel_buffers(n, *((1,),) * n_nets)
    out = critic.forward(x, a, out=tuple(b[:n] for b in big) if n_nets == 2 else big[0][:n])
    assert last_kernel().startswith(case.kernel + "x%d" % n_nets), last_kernel()
    out = out if n_nets == 2 else (out,)
    for c in range(n_nets):
        assert out[c].data_ptr() == big[c].data_ptr() and kept(big[c], n)
        assert np.array_equal(bits(big[c][:n, 0]), bits(q_f[c])), c

    # row 0 alone
    one = critic.forward(x[:1], a[:1])
    assert last_kernel().startswith(case.kernel + "x%d" % n_nets), last_kernel()
    one = one if n_nets == 2 else (one,)
    for c in range(n_nets):
        assert tuple(one[c].shape) == (1, 1) and np.array_equal(bits(one[c]).reshape(-1), bits(q_f[c][:1])), c

    # the device pack of the same weights
    dev = TM.make(dims, sds, gemm="fused", n_nets=n_nets)
    dev.pack = "device"
    q_d = TM.run(dev, x, a, "fused")
    assert dev.pack == "device" and dev.packs == n_nets
    assert last_kernel().startswith(case.kernel), last_kernel()
    for c in range(n_nets):
        n_diff = int((bits(q_d[c]) != bits(q_f[c])).sum())
        print("%s: q%d of pack=device differs from pack=host in %d of %d rows" % (what, c + 1, n_diff, n))
        assert n_diff == 0

    # one TD target: the argument marshalling reaches the epilogue at this instantiation
    reward, done, lp, li, coef = TM.td_inputs(n, b_seed + 1)
    ybuf, *qbuf = sentinel_buffers(n, (), *((1,),) * n_nets)
    y = critic.td_target(T(reward), x, a, T(done), 0.99, T(lp), T(li), T(coef), out=ybuf[:n],
                         q=tuple(b[:n] for b in qbuf) if n_nets == 2 else qbuf[0][:n])
    assert y.data_ptr() == ybuf.data_ptr() and kept(ybuf, n) and all(kept(b, n) for b in qbuf)
    for c in range(n_nets):
        assert np.array_equal(bits(qbuf[c][:n, 0]), bits(q_f[c])), c
    TM.check_epilogue(y.cpu().numpy(), q_f[0], q_f[1] if n_nets == 2 else None, reward, done, 0.99, what, coef, lp, li)
    e_y = MR.err(y.cpu().numpy(), MR.td_target64(reward, refs[0], refs[1] if n_nets == 2 else None, done, 0.99, coef, lp, li))
    print("%s: target vs float64 %.3g" % (what, e_y))
    assert e_y < MR.BAR


# -------------------------------------------------------------------------------------------------- MARL critic, wide
def wide_bars(critic, x, a, what):
    """`check_bars` of test_marl_critic_hip.py with the chunked kernel in the fused kernel's place: gemm="wide" and the
    library mode against the float64 restatement on the same inputs, both bars as they stand in marl_critic_ref.py."""
    q_w, q_l = TW.run(critic, x, a, "wide"), TW.run(critic, x, a, "library")
    refs = []
    for c, sd in enumerate(TW.np_sds(critic)):
        ref64 = MR.critic_q64(sd, x.cpu().numpy(), a.cpu().numpy())
        e_w, e_l = MR.err(q_w[c], ref64), MR.err(q_l[c], ref64)
        print("%s: q%d err wide %.3g library %.3g (ratio %.2f), max |q64| %.3g"
              % (what, c + 1, e_w, e_l, e_w / max(e_l, 1e-30), np.abs(ref64).max()))
        assert np.isfinite(q_w[c]).all()
        assert e_l < MR.BAR and e_w < MR.BAR
        assert e_w <= MR.fused_bar(e_l)
        refs.append(ref64)
    return q_w, refs


@pytest.mark.parametrize("index,n_nets", SW.MARL_CRITIC_WIDE_RUNS,
                         ids=["%s-x%d" % (SW.case_id(SW.MARL_CRITIC_WIDE[i]), k) for i, k in SW.MARL_CRITIC_WIDE_RUNS])
def test_marl_critic_wide(index, n_nets):
    from ris_vec_marl_amd import marl_critic as MC
    case = SW.MARL_CRITIC_WIDE[index]
    dims, n = case.dims, SW.CRITIC_ROWS
    w_seed, b_seed = SW.seeds("wide", index)
    sds = [MR.random_net(dims, w_seed + c) for c in range(n_nets)]
    what = "wide %s x%d" % (SW.case_id(case), n_nets)
    kernel = case.kernel + "x%d" % n_nets
    critic = TW.make(dims, sds, gemm="wide", n_nets=n_nets)
    assert critic.gemm == "wide" and critic.pack == "host"
    x, a = TW.batch(dims, n, b_seed)
    assert tuple(x.shape) == (n, dims[0]) and tuple(a.shape) == (n, dims[1]) and not x[0].any() and not a[0].any()
    q_w, refs = wide_bars(critic, x, a, what)                 # both modes, both bars; prints wide and library err
    assert all(np.abs(ref).max() > 0.05 for ref in refs)

    # the long call into longer buffers: the instantiation, the same bits, the tail untouched
    big = sentinel_buffers(n, *((1,),) * n_nets)
    out = critic.forward(x, a, out=tuple(b[:n] for b in big) if n_nets == 2 else big[0][:n])
    assert last_kernel().startswith(kernel), last_kernel()
    out = out if n_nets == 2 else (out,)
    for c in range(n_nets):
        assert out[c].data_ptr() == big[c].data_ptr() and kept(big[c], n)
        assert np.array_equal(bits(big[c][:n, 0]), bits(q_w[c])), c

    # row 0 alone
    one = critic.forward(x[:1], a[:1])
    assert last_kernel().startswith(kernel), last_kernel()
    one = one if n_nets == 2 else (one,)
    for c in range(n_nets):
        assert tuple(one[c].shape) == (1, 1) and np.array_equal(bits(one[c]).reshape(-1), bits(q_w[c][:1])), c

    # each net of the twin launch against a one-net launch that holds its weights: the second net restages the input from
    # its first chunk and starts from zeroed accumulators
    if n_nets == 2:
        for c in range(2):
            single = TW.make(dims, [sds[c]], gemm="wide", n_nets=1)
            q_1 = TW.run(single, x, a, "wide")
            assert last_kernel().startswith(case.kernel + "x1"), last_kernel()
            n_diff = int((bits(q_1[0]) != bits(q_w[c])).sum())
            print("%s: q%d of the twin launch differs from a one-net launch in %d of %d rows" % (what, c + 1, n_diff, n))
            assert n_diff == 0
        assert not np.array_equal(q_w[0], q_w[1])

    # the device pack of the same weights: the same streams and scales, padding included, and so the same q
    dev = TW.make(dims, sds, gemm="wide", n_nets=n_nets)
    dev.pack = "device"
    q_d = TW.run(dev, x, a, "wide")
    assert dev.pack == "device" and dev.packs == n_nets == critic.packs
    assert last_kernel().startswith(kernel), last_kernel()
    rows = MC.marl_critic_geom(*dims).rows
    for c in range(n_nets):
        (s_h, u_h), (s_d, u_d) = critic.nets[c].packed[1], dev.nets[c].packed[1]
        assert tuple(s_d.shape) == tuple(s_h.shape) == (rows, 64, 8) and s_d.dtype == s_h.dtype == torch.float16
        assert torch.equal(s_h.view(torch.int16), s_d.view(torch.int16)) and np.array_equal(bits(u_h), bits(u_d)), c
        n_diff = int((bits(q_d[c]) != bits(q_w[c])).sum())
        print("%s: q%d of pack=device differs from pack=host in %d of %d rows" % (what, c + 1, n_diff, n))
        assert n_diff == 0

    # one TD target: the argument marshalling reaches the epilogue at this instantiation
    reward, done, lp, li, coef = TW.td_inputs(n, b_seed + 1)
    ybuf, *qbuf = sentinel_buffers(n, (), *((1,),) * n_nets)
    y = critic.td_target(T(reward), x, a, T(done), 0.99, T(lp), T(li), T(coef), out=ybuf[:n],
                         q=tuple(b[:n] for b in qbuf) if n_nets == 2 else qbuf[0][:n])
    assert last_kernel().startswith(kernel), last_kernel()
    assert y.data_ptr() == ybuf.data_ptr() and kept(ybuf, n) and all(kept(b, n) for b in qbuf)
    for c in range(n_nets):
        assert np.array_equal(bits(qbuf[c][:n, 0]), bits(q_w[c])), c
    TW.check_epilogue(y.cpu().numpy(), q_w[0], q_w[1] if n_nets == 2 else None, reward, done, 0.99, what, coef, lp, li)
    e_y = MR.err(y.cpu().numpy(), MR.td_target64(reward, refs[0], refs[1] if n_nets == 2 else None, done, 0.99, coef, lp, li))
    print("%s: target vs float64 %.3g" % (what, e_y))
    assert e_y < MR.BAR

    # where the fused rule holds too: one chunk, and the fused kernel's bits
    assert MC._supported(*dims) == (index == 0)
    if MC._supported(*dims):
        fused = TW.make(dims, sds, gemm="fused", n_nets=n_nets)
        assert fused.gemm == "fused"
        q_f = TW.run(fused, x, a, "fused")
        assert last_kernel().startswith("k_marl_critic<"), last_kernel()
        y_f = fused.td_target(T(reward), x, a, T(done), 0.99, T(lp), T(li), T(coef))
        for c in range(n_nets):
            assert np.array_equal(bits(q_f[c]), bits(q_w[c])), c
        assert np.array_equal(bits(y_f), bits(y))


# ------------------------------------------------------------------------------------------------------ local critics
def local_make(dims, sds, n_nets, gemm="fused", pack=None):
    from ris_vec_marl_amd import BatchedLocalCritics
    critic = BatchedLocalCritics(*dims, n_nets=n_nets, device=DEV, gemm=gemm)
    if pack is not None:
        critic.pack = pack
    for j, pair in enumerate(sds):
        critic.load_agent_state_dict(j, *pair)
    return critic


def local_run(critic, mode, obs, n_out, **form):
    """q [n_nets][V, n] and y [V, n] (None without `reward`) of `critic` in `mode`, as numpy, through one flat buffer per
    output that is PAD values longer than [V, n]: the tail keeps its sentinel.  form: action= (forward, or td_target's
    action_ with reward=, done=, ...) or heads=, power= (td_target only)."""
    V, n, k = critic.n_agents, obs.shape[0], critic.n_nets
    flat = [torch.full((V * n + SW.PAD,), SENTINEL, device=DEV) for _ in range(n_out)]
    qs = tuple(b[:V * n].view(V, n, 1) for b in flat[:k])
    was, critic.gemm = critic.gemm, mode
    try:
        if "reward" in form:
            kw = {key: (None if v is None else T(v)) for key, v in form.items() if key not in ("reward", "done", "gamma")}
            if "action" in kw:
                kw["action_"] = kw.pop("action")
            y = critic.td_target(T(form["reward"]), obs, T(form["done"]), form["gamma"], out=flat[k][:V * n].view(V, n),
                                 q=qs if k == 2 else qs[0], **kw)
            assert y.data_ptr() == flat[k].data_ptr()
        else:
            out = critic.forward(obs, T(form["action"]), out=qs if k == 2 else qs[0])
            assert (out if k == 2 else (out,))[0].data_ptr() == flat[0].data_ptr()
    finally:
        critic.gemm = was
    for b in flat:
        assert bool((b[V * n:] == SENTINEL).all()) and bool(torch.isfinite(b[:V * n]).all())
    got = [b[:V * n].cpu().numpy().reshape(V, n) for b in flat]
    return got[:k], (got[k] if n_out > k else None)


def local_bars(q_f, q_l, sds, obs, act, what):
    """Every agent's q of both modes against `critic_q64` with THAT agent's weights on that agent's columns; both bars."""
    worst_f = worst_l = 0.0
    least = np.inf
    for j, pair in enumerate(sds):
        for c, sd in enumerate(pair):
            ref64 = MR.critic_q64(sd, obs[:, j], act[:, j])
            e_f, e_l = MR.err(q_f[c][j], ref64), MR.err(q_l[c][j], ref64)
            worst_f, worst_l, least = max(worst_f, e_f), max(worst_l, e_l), min(least, np.abs(ref64).max())
            assert e_l < MR.BAR and e_f < MR.BAR, (what, j, c, e_f, e_l)
            assert e_f <= MR.fused_bar(e_l), (what, j, c, e_f, e_l)
            assert np.abs(ref64).max() > 0.05, (what, j, c)
    print("%s: over %d agents x %d nets: largest err fused %.3g library %.3g, smallest max |q64| %.3g"
          % (what, len(sds), len(sds[0]), worst_f, worst_l, least))


@pytest.mark.parametrize("index,n_nets", SW.LOCAL_CRITICS_RUNS,
                         ids=["%s-x%d" % (SW.case_id(SW.LOCAL_CRITICS[i]), k) for i, k in SW.LOCAL_CRITICS_RUNS])
def test_local_critics(index, n_nets):
    from ris_vec_marl_amd import BatchedTwinCritic
    case = SW.LOCAL_CRITICS[index]
    dims, n = case.dims, SW.CRITIC_ROWS
    V, S, A = dims[:3]
    w_seed, b_seed = SW.seeds("local", index)
    sds = SW.local_nets(dims, w_seed, n_nets)
    what = "local %s x%d" % (SW.case_id(case), n_nets)
    kernel = case.kernel + "x%d" % n_nets
    critic = local_make(dims, sds, n_nets)
    assert critic.gemm == "fused" and critic.pack == "host" and critic.action_dims == A
    obs, act = SW.local_batch(dims, n, b_seed)
    assert obs.shape == (n, V, S) and act.shape == (n, V, A) and not obs[0].any() and not act[0].any()
    obs_t, act_t = T(obs), T(act)

    # the long call, sentinel tails; every agent against float64 with its own weights
    q_f, _ = local_run(critic, "fused", obs_t, n_nets, action=act)
    assert last_kernel() == kernel, last_kernel()
    q_l, _ = local_run(critic, "library", obs_t, n_nets, action=act)
    local_bars(q_f, q_l, sds, obs, act, what)

    # every agent against the global kernel holding that agent's weights, bit for bit
    for j in range(V):
        twin = BatchedTwinCritic(S, A, *dims[3:], n_nets=n_nets, device=DEV, gemm="fused")
        twin.load_state_dict(*sds[j])
        want = twin.forward(obs_t[:, j].contiguous(), act_t[:, j].contiguous())
        assert last_kernel().startswith("k_marl_critic<"), last_kernel()
        want = want if n_nets == 2 else (want,)
        for c in range(n_nets):
            assert np.array_equal(bits(want[c]).reshape(-1), bits(q_f[c][j])), "%s: agent %d net %d differs from the global kernel" % (what, j, c + 1)

    # row 0 alone
    one = critic.forward(obs_t[:1], act_t[:1])
    assert last_kernel() == kernel, last_kernel()
    one = one if n_nets == 2 else (one,)
    for c in range(n_nets):
        assert tuple(one[c].shape) == (V, 1, 1) and np.array_equal(bits(one[c]).reshape(-1), bits(q_f[c][:, 0])), c

    # the device pack of the same weights: the same streams and scales, and so the same q
    dev = local_make(dims, sds, n_nets, pack="device")
    q_d, _ = local_run(dev, "fused", obs_t, n_nets, action=act)
    assert dev.pack == "device" and dev.packs == V * n_nets == critic.packs
    assert last_kernel() == kernel, last_kernel()
    for j in range(V):
        for c in range(n_nets):
            (s_h, u_h), (s_d, u_d) = critic.nets[j][c].packed[1], dev.nets[j][c].packed[1]
            assert torch.equal(s_h.view(torch.int16), s_d.view(torch.int16)) and np.array_equal(bits(u_h), bits(u_d)), (j, c)
    for c in range(n_nets):
        n_diff = int((bits(q_d[c]) != bits(q_f[c])).sum())
        print("%s: q%d of pack=device differs from pack=host in %d of %d values" % (what, c + 1, n_diff, V * n))
        assert n_diff == 0

    # one TD target in the explicit form: the float64 bound and the reference's float32 statements, operation by operation
    reward, done, lp, li, coef = TL.td_inputs(V, n, b_seed + 1)
    td = dict(reward=reward, done=done, gamma=0.99, logp_power=lp, logp_intent=li, coef=coef)
    q_t, y = local_run(critic, "fused", obs_t, n_nets + 1, action=act, **td)
    assert last_kernel() == kernel, last_kernel()
    for c in range(n_nets):
        assert np.array_equal(bits(q_t[c]), bits(q_f[c])), c
    TL.check_epilogue(y, q_t[0], q_t[1] if n_nets == 2 else None, reward, done, 0.99, what, coef, lp, li)

    # A = V + 2: the action built from the policy's heads, against the action NumPy builds from them
    if A == V + 2:
        heads, power, act_p, idx = SW.local_policy_inputs(dims, n, b_seed + 2)
        for j in range(V):
            lo, _ = [i for i in range(V) if i != j][1:3]
            assert idx[j, 0] != j and idx[j, 1] == lo and idx[j, 2] == j              # the planted rows
        q_p, y_p = local_run(critic, "fused", obs_t, n_nets + 1, heads=heads, power=power, **td)
        assert last_kernel() == kernel, last_kernel()
        q_e, y_e = local_run(critic, "fused", obs_t, n_nets + 1, action=act_p, **td)
        q_pl, y_pl = local_run(critic, "library", obs_t, n_nets + 1, heads=heads, power=power, **td)
        local_bars(q_p, q_pl, sds, obs, act_p, what + " from the policy")
        for c in range(n_nets):
            n_diff = int((bits(q_p[c]) != bits(q_e[c])).sum())
            print("%s: q%d from the policy differs from the explicit form in %d of %d values" % (what, c + 1, n_diff, V * n))
            assert n_diff == 0
        assert np.array_equal(bits(y_p), bits(y_e))
        TL.check_epilogue(y_p, q_p[0], q_p[1] if n_nets == 2 else None, reward, done, 0.99, what + " from the policy", coef, lp, li)
        TL.check_epilogue(y_pl, q_pl[0], q_pl[1] if n_nets == 2 else None, reward, done, 0.99, what + " from the policy, library",
                          coef, lp, li)


# ------------------------------------------------------------------------------------------------------- SARL critic
@pytest.mark.parametrize("index", range(len(SW.SARL_CRITIC)), ids=[SW.case_id(c) for c in SW.SARL_CRITIC])
def test_sarl_critic(index):
    from ris_vec_marl_amd import BatchedCritic
    case = SW.SARL_CRITIC[index]
    dims, n = case.dims, SW.CRITIC_ROWS
    IN, F1, F2, F3, A = dims
    w_seed, b_seed = SW.seeds("critic", index)
    sd = R.random_critic(dims, w_seed)
    what = "critic %s" % SW.case_id(case)
    critic = TC.make_critic(dims, sd, gemm="fused")
    assert critic.gemm == "fused" and critic.pack == "host"
    x, a = TC.batch(dims, n, b_seed)
    assert tuple(x.shape) == (n, IN) and tuple(a.shape) == (n, A) and not x[0].any() and not a[0].any()
    q_f, ref = TC.check_bars(critic, x, a, what)              # both modes, both bars; prints fused and library err
    assert np.abs(ref).max() > 0.05

    big, big_q, big_y = sentinel_buffers(n, (1,), (1,), ())
    assert critic.forward(x, a, out=big[:n]).data_ptr() == big.data_ptr()
    assert last_kernel().startswith(case.kernel), last_kernel()
    assert kept(big, n) and np.array_equal(bits(big[:n, 0]), bits(q_f))

    one = critic.forward(x[:1], a[:1])
    assert last_kernel().startswith(case.kernel), last_kernel()
    assert tuple(one.shape) == (1, 1) and np.array_equal(bits(one).reshape(-1), bits(q_f[:1]))

    dev = BatchedCritic(IN, A, F1, F2, F3, device=DEV, seed=1, gemm="fused", pack="device")
    dev.load_state_dict(sd)
    q_d = TC.run(dev, x, a, "fused")
    assert dev.pack == "device" and dev.packs == 1
    assert last_kernel().startswith(case.kernel), last_kernel()
    n_diff = int((bits(q_d) != bits(q_f)).sum())
    print("%s: q of pack=device differs from pack=host in %d of %d rows (largest |difference| %.3g)"
          % (what, n_diff, n, float(np.abs(q_d - q_f).max())))
    assert n_diff == 0

    rng = np.random.default_rng(b_seed + 1)
    reward, done = rng.uniform(-6, 1, n).astype(np.float32), rng.uniform(size=n) < 0.3
    done[0], done[1] = True, False
    y = critic.td_target(T(reward), x, a, T(done), 0.99, out=big_y[:n], q=big_q[:n])
    assert y.data_ptr() == big_y.data_ptr() and kept(big_y, n) and kept(big_q, n)
    assert np.array_equal(bits(big_q[:n, 0]), bits(q_f))
    TC.check_epilogue(y.cpu().numpy(), q_f, reward, done, 0.99, what)
    e_y = R.err(y.cpu().numpy(), R.td_target64(reward, ref, done, 0.99))
    print("%s: target vs float64 %.3g" % (what, e_y))
    assert e_y < R.BAR


# ------------------------------------------------------------------------------------------------------------- actor
@pytest.mark.parametrize("index", range(len(SW.SARL_ACTOR)), ids=[SW.case_id(c) for c in SW.SARL_ACTOR])
def test_sarl_actor(index):
    from ris_vec_marl_amd import BatchedActor
    case = SW.SARL_ACTOR[index]
    dims, n = case.dims, SW.ACTOR_ROWS
    IN, F1, F2, A = dims
    V, tn = case.obs
    assert V * (tn + 5) == IN
    w_seed, b_seed = SW.seeds("actor", index)
    sd = SW.actor_weights(dims, w_seed)
    what = "actor %s" % SW.case_id(case)
    actor = BatchedActor(IN, A, F1, F2, device=DEV, seed=1)
    assert actor.gemm == "fused" and actor.pack == "host"
    actor.load_state_dict(sd)
    o = TA.obs_like(np.random.default_rng(b_seed), n, V, tn)
    o[0] = 0.0
    x = T(o)
    lg_f, mu_f, ref = TA.check_bars(actor, x, what)           # both modes, every bar; prints fused and library err
    mu64 = TA.sigmoid64(ref)
    print("%s: mu64 spans [%.3g, %.3g]" % (what, mu64.min(), mu64.max()))
    assert np.abs(mu64 - 0.5).max() > 0.1                       # the widened head: the sigmoid is not stuck at 1/2

    big, big_l = sentinel_buffers(n, (A,), (A,))
    assert actor.forward(x, out=big[:n], logits=big_l[:n]).data_ptr() == big.data_ptr()
    assert last_kernel().startswith(case.kernel), last_kernel()
    assert kept(big, n) and kept(big_l, n)
    assert np.array_equal(bits(big[:n]), bits(mu_f)) and np.array_equal(bits(big_l[:n]), bits(lg_f))

    one_l = torch.full((1, A), NAN, device=DEV)
    one = actor.forward(x[:1], logits=one_l)
    assert last_kernel().startswith(case.kernel), last_kernel()
    assert np.array_equal(bits(one), bits(mu_f[:1])) and np.array_equal(bits(one_l), bits(lg_f[:1]))

    dev = BatchedActor(IN, A, F1, F2, device=DEV, seed=2, pack="device")
    dev.load_state_dict(sd)
    lg_d, mu_d = TA.run(dev, x, "fused")
    assert dev.pack == "device" and last_kernel().startswith(case.kernel), last_kernel()
    n_diff = int((bits(lg_d) != bits(lg_f)).sum())
    print("%s: logits of pack=device differ from pack=host in %d of %d values (largest |difference| %.3g)"
          % (what, n_diff, lg_f.size, float(np.abs(lg_d - lg_f).max())))
    assert n_diff == 0 and np.array_equal(bits(mu_d), bits(mu_f))
