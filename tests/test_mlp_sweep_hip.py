"""GPU sweep of the three learner-side MFMA kernels -- `k_marl_critic<MT2,MT3>` (BatchedTwinCritic), `k_sarl_critic<MT2,MT3>`
(BatchedCritic) and `k_sarl_actor<MT,KS>` (BatchedActor) -- over every template instantiation and every edge of their
run-time parameters (tests/mlp_sweep_shapes.py names the edge each case is there for): clamped prefetch, wavefronts
without work, all-zero k-steps, the bias row at a k-step boundary, partly filled head tiles, the > 64 KiB dynamic-LDS
attribute path.  The other test_*_hip.py files of these kernels stay at the driver's sizes and the fixtures.

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
  * critics: one `td_target` through the epilogue check of the kernel's own test file.
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
from tests import test_marl_critic_hip as TM  # noqa: E402
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
