"""GPU tests of the chunked twin critic (`BatchedTwinCritic(gemm="wide")`, `risvec_marl_critic_wide`, k_marl_critic_wide in
csrc/k_marl_critic.hip): the launch of `risvec_marl_critic` with fc1 walking the input 8 k-steps at a time, which covers
the driver's 16 vehicles (80 + 288 inputs).  Measured against the float64 restatement of tests/marl_critic_ref.py and,
where the fused kernel is built too, against that kernel bit for bit.

The shapes are the smallest at which the chunk walk can go wrong: 96-256-256 gives 3 fc1 groups over 4 wavefronts (one
wavefront has none) and two output tiles per wavefront in fc2 and fc3; 130 inputs are chunks of 8 + 1 k-steps, the last
with 2 live columns; 256 inputs two full chunks; the driver's 368 three chunks with 8 groups per wavefront.

Error measure and bars are those of test_marl_critic_hip.py: err = max over rows |q - q64| / max(max over the batch |q64|,
1e-3); err < 2e-5 in every mode; wide <= max(8 x the library mode's err on the same inputs, 1e-7).  The epilogue, against
the q1 / q2 the same launch wrote: |y - y64| <= 2^-22 (|r| + |gamma| (|m| + |c0 lp| + |c1 li|)); rows with `done` equal the
reward bit for bit.  Every figure is printed before it is asserted (pytest -s shows them)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import marl_critic_ref as R  # noqa: E402

DEV = "cuda:0"
DRIVER16 = (80, 288, 1024, 512, 256)    # 16 vehicles: 23 k-steps = chunks 8 + 8 + 7, 8 fc1 groups per wavefront
SMALL9 = (40, 90, 96, 256, 256)         # 9 k-steps = chunks 8 + 1, the last k-step with 2 live columns
SMALL16 = (64, 192, 96, 256, 256)       # 16 k-steps = two full chunks
IDLE = (80, 288, 32, 128, 128)          # one fc1 group: three wavefronts idle in fc1
ORACLE = (SMALL9, SMALL16, DRIVER16, IDLE)
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
    """(q1, q2) [n] of `critic` in `mode` on device tensors, as numpy, through caller-owned buffers."""
    was, critic.gemm = critic.gemm, mode
    try:
        out = tuple(torch.full((x.shape[0], 1), NAN, device=DEV) for _ in range(critic.n_nets))
        q = critic.forward(x, a, out=out if critic.n_nets == 2 else out[0])
        q = q if critic.n_nets == 2 else (q,)
        assert all(t.data_ptr() == o.data_ptr() for t, o in zip(q, out))
    finally:
        critic.gemm = was
    return [t.cpu().numpy().reshape(-1) for t in q]


def check_epilogue(y, q1, q2, reward, done, gamma, what, coef=None, lp=None, li=None):
    """y against the float64 target built from the q1 / q2 the same launch wrote (gamma and coef as the float32 values the
    kernel receives): test_marl_critic_hip.py's check, restated"""
    g32 = float(np.float32(gamma))
    y = np.asarray(y, np.float64).reshape(-1)
    y64 = R.td_target64(reward, q1, q2, done, g32, coef, lp, li)
    live = ~np.asarray(done, bool)
    excess = np.abs(y - y64) - R.y_bound(reward, q1, q2, g32, coef, lp, li)
    print("%s: epilogue, worst |y - y64| - bound = %.3g over %d live rows" % (what, excess[live].max() if live.any() else NAN, live.sum()))
    assert np.isfinite(y[live]).all() and (excess[live] <= 0).all()
    assert np.array_equal(y[~live], np.asarray(reward, np.float64)[~live])


@functools.lru_cache(maxsize=None)
def wide_critic(dims):
    """Two nets in the reference's initialisation ranges, q widened to +-0.4.  Shared and never modified: tests that update
    weights build their own."""
    return make(dims, [R.random_net(dims, 41), R.random_net(dims, 42)], gemm="wide")


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


# ---------------------------------------------------------------------------------------------------- 1: float64 oracle
@pytest.mark.parametrize("n", [1, 33, 65])
@pytest.mark.parametrize("dims", ORACLE)
def test_wide_and_library_vs_float64(dims, n):
    """Partly filled tiles and more than one workgroup.  Both bars of the module docstring, as they stand in
    tests/marl_critic_ref.py.  Row 0 of the 33- and 65-row batches is all zero.  The one-row batch is a drawn row: err is
    relative to the batch's largest |q64|, and a batch that is only the all-zero row has nothing but the bias path, whose
    single q can cancel to almost nothing (the float64 reference gives 3.5e-4 for net 2 at the driver's shape, from terms
    of 0.05), which would measure that cancellation and not the kernel -- in either mode."""
    from ris_vec_marl_amd import _native as N
    critic = wide_critic(dims)
    assert critic.gemm == "wide"
    x, a = batch(dims, n, 100 + n, 16 if dims[:2] == (80, 288) else None, zero_row0=n > 1)
    assert n == 1 or (not x[0].any() and not a[0].any())
    q_w = run(critic, x, a, "wide")
    assert N.last_kernel() == "k_marl_critic_wide<%d,%d>x2" % (dims[3] // 128, dims[4] // 128)
    q_l = run(critic, x, a, "library")
    for c, sd in enumerate(np_sds(critic)):
        ref64 = R.critic_q64(sd, x.cpu().numpy(), a.cpu().numpy())
        e_w, e_l = R.err(q_w[c], ref64), R.err(q_l[c], ref64)
        print("%s x %d: q%d err wide %.3g library %.3g (ratio %.2f), max |q64| %.3g"
              % (dims, n, c + 1, e_w, e_l, e_w / max(e_l, 1e-30), np.abs(ref64).max()))
        assert np.isfinite(q_w[c]).all()
        assert e_l < R.BAR and e_w < R.BAR
        assert e_w <= R.fused_bar(e_l)


# ---------------------------------------------------------------------------------------------------- 2: against the fused kernel
@pytest.mark.parametrize("dims", [(40, 80, 96, 256, 256), (20, 24, 1024, 512, 256)])
def test_one_chunk_is_the_fused_kernel_bit_for_bit(dims):
    sds = [R.random_net(dims, 61), R.random_net(dims, 62)]
    n = 70
    x, a = batch(dims, n, 9, None)
    reward, done, lp, li, coef = td_inputs(n, 3)
    got = {}
    for mode in ("wide", "fused"):
        critic = make(dims, sds, gemm=mode)
        assert critic.gemm == mode
        q = critic.forward(x, a)
        qs = tuple(torch.full((n, 1), NAN, device=DEV) for _ in range(2))
        y = critic.td_target(T(reward), x, a, T(done), 0.99, T(lp), T(li), T(coef), q=qs)
        assert all(torch.equal(u, v) for u, v in zip(q, qs))
        got[mode] = (q[0], q[1], y)
    for name, w, f in zip(("q1", "q2", "y"), got["wide"], got["fused"]):
        d = float((w - f).abs().max())
        print("%s: %s wide - fused, largest difference %.3g" % (dims, name, d))
        assert torch.isfinite(w).all() and torch.equal(w, f), name


def test_a_chunk_edge_with_zero_weights_beyond_is_the_fused_kernel_bit_for_bit():
    """A (40, 80) net embedded into (40, 200): W1 gets 120 all-zero columns, the action rows 120 more values in (-1, 1).
    Zero weights add exact zeros in the same k order and the pack scale ignores zeros, so the wide kernel over chunks of
    8 + 7 k-steps equals the fused kernel over its 8."""
    small, big, n = (40, 80, 96, 256, 256), (40, 200, 96, 256, 256), 70
    sds = [R.random_net(small, 71), R.random_net(small, 72)]
    emb = [dict(sd, **{"fc1.weight": np.concatenate([sd["fc1.weight"], np.zeros((96, 120), np.float32)], 1)}) for sd in sds]
    s, a = R.random_batch(small, n, 5, None, zero_row0=False)
    extra = np.random.default_rng(6).uniform(-1, 1, (n, 120)).astype(np.float32)
    assert np.isfinite(extra).all() and np.abs(extra).max() < 1 and np.abs(extra).min() > 0
    reward, done, lp, li, coef = td_inputs(n, 4)
    fused, wide = make(small, sds, gemm="fused"), make(big, emb, gemm="wide")
    qf, qw = fused.forward(T(s), T(a)), wide.forward(T(s), T(np.concatenate([a, extra], 1)))
    yf = fused.td_target(T(reward), T(s), T(a), T(done), 0.99, T(lp), T(li), T(coef))
    yw = wide.td_target(T(reward), T(s), T(np.concatenate([a, extra], 1)), T(done), 0.99, T(lp), T(li), T(coef))
    for name, w, f in (("q1", qw[0], qf[0]), ("q2", qw[1], qf[1]), ("y", yw, yf)):
        print("embedded: %s wide - fused, largest difference %.3g" % (name, float((w - f).abs().max())))
        assert torch.isfinite(w).all() and bool((w == f).all()), name
    assert float(qw[0].abs().max()) > 0.05


# ---------------------------------------------------------------------------------------------------- 3: the epilogue
def test_epilogue_forms():
    dims, n = SMALL9, 97
    x, a = batch(dims, n, 21, None)
    # net 2's q bias is set so that the median of q1 - q2 over these rows is 0, and min() has both outcomes
    sds = np_sds(wide_critic(dims))
    q0 = run(wide_critic(dims), x, a, "wide")
    sds[1]["q.bias"] = sds[1]["q.bias"] + np.float32(np.median(q0[0] - q0[1]))
    critic = make(dims, sds, gemm="wide")
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
        assert torch.equal(y[td], tr[td])
    # one net: m = q1; and a twin launch gives each net the bits of a one-net launch holding its weights
    twin = run(critic, x, a, "wide")
    for c in (0, 1):
        one = make(dims, [sds[c]], gemm="wide", n_nets=1)
        q1 = torch.full((n, 1), NAN, device=DEV)
        y = one.td_target(tr, x, a, td, 0.97, tlp, tli, tc, q=q1)
        check_epilogue(y.cpu().numpy(), q1.cpu().numpy(), None, reward, done, 0.97, "epilogue one net (%d)" % (c + 1), coef=coef, lp=lp, li=li)
        y0 = one.td_target(torch.zeros(n, device=DEV), x, a, td, 1.0, q=q1)
        assert torch.equal(y0[live], q1.view(n)[live])
        assert isinstance(one.forward(x, a), torch.Tensor)
        assert np.array_equal(q1.cpu().numpy().reshape(-1), twin[c]), c
    assert not np.array_equal(twin[0], twin[1])


# ---------------------------------------------------------------------------------------------------- 4: weights in the loop
def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def test_shared_weights_repack_once_per_net_at_sixteen_vehicles():
    dims = DRIVER16
    sds = [{k: T(v) for k, v in R.random_net(dims, s).items()} for s in (81, 82)]
    critic = make(dims, gemm="wide")
    critic.share_state_dict(*sds)
    x, a = batch(dims, 33, 4, 16)
    critic.forward(x, a)
    critic.forward(x, a)
    assert critic.packs == 2                                  # one pack per net, reused
    sds[1]["fc2.weight"].add_(0.01)
    q = critic.forward(x, a)
    assert critic.packs == 3                                  # only the net that changed
    for sd in sds:
        for k in ("fc1.weight", "fc2.weight", "fc3.weight"):
            sd[k].mul_(1.01)
    q = critic.forward(x, a)
    assert critic.packs == 5                                  # exactly one rebuild per net
    for c in (0, 1):
        ref = R.critic_q64({k: v.cpu().numpy() for k, v in sds[c].items()}, x.cpu().numpy(), a.cpu().numpy())
        e = R.err(q[c].cpu().numpy(), ref)
        print("after the in-place update: q%d err %.3g" % (c + 1, e))
        assert e < R.BAR
    critic.forward(x, a)
    assert critic.packs == 5
    critic.mark_stale()
    critic.forward(x, a)
    assert critic.packs == 7


def test_device_pack_and_the_blend_at_sixteen_vehicles():
    from ris_vec_marl_amd import _native as N
    from ris_vec_marl_amd import marl_critic as MC
    dims, n = DRIVER16, 33
    nets = [R.random_net(dims, 91 + c) for c in (0, 1)]
    online = [{k: T(v) for k, v in R.random_net(dims, 95 + c).items()} for c in (0, 1)]
    x, a = batch(dims, n, 9, 16)
    host, dev = make(dims, nets, gemm="wide"), make(dims, nets, gemm="wide")
    dev.pack = "device"
    assert (host.pack, dev.pack) == ("host", "device")
    qh, qd = host.forward(x, a), dev.forward(x, a)
    assert N.last_kernel().startswith("k_marl_critic_wide<4,2>x2")
    assert host.packs == dev.packs == 2
    for c in (0, 1):                                          # the same streams and scales, padding included, and so the same q
        (sh, uh), (sd, ud) = host.nets[c].packed[1], dev.nets[c].packed[1]
        assert tuple(sd.shape) == (MC.marl_critic_geom(*dims).rows, 64, 8)
        assert torch.equal(bits(sh), bits(sd)) and torch.equal(bits(uh), bits(ud)), c
        assert torch.equal(qh[c], qd[c])
    streams = [net.packed[1][0].data_ptr() for net in dev.nets]
    # the blend, then the target: 1 + 2 + 1 launches
    packs = dev.packs
    dev.soft_update_from(*online, tau=0.005)
    assert N.last_kernel() == "k_soft_update"
    host.soft_update_from(*online, tau=0.005)
    reward, done, lp, li, coef = td_inputs(n, 7)
    qs = tuple(torch.full((n, 1), NAN, device=DEV) for _ in range(2))
    y = dev.td_target(T(reward), x, a, T(done), 0.99, T(lp), T(li), T(coef), q=qs)
    assert N.last_kernel().startswith("k_marl_critic_wide<")
    assert dev.packs == packs + 2 and [net.packed[1][0].data_ptr() for net in dev.nets] == streams
    yh = host.td_target(T(reward), x, a, T(done), 0.99, T(lp), T(li), T(coef))
    assert torch.equal(y, yh)                                 # the blended weights through either pack
    check_epilogue(y.cpu().numpy(), qs[0].cpu().numpy(), qs[1].cpu().numpy(), reward, done, 0.99, "after the blend", coef, lp, li)
    for c, sd in enumerate(dev.state_dict()):                 # q against the blended weights
        e = R.err(qs[c].cpu().numpy(), R.critic_q64({k: v.numpy() for k, v in sd.items()}, x.cpu().numpy(), a.cpu().numpy()))
        print("after the blend: q%d err %.3g" % (c + 1, e))
        assert e < R.BAR
    # the pack kernels are what rebuilt the streams: a stale critic names them when the rebuild is run on its own
    dev.mark_stale()
    dev._fused_weights()
    assert N.last_kernel() == "k_marl_critic_pack x2" and dev.packs == packs + 4
    with pytest.raises(ValueError):                           # the fused rule's pack still refuses the shape
        MC.pack_marl_critic_weights_device([tuple(getattr(dev.nets[0], k) for k in ("W1", "W2", "W3"))])


# ---------------------------------------------------------------------------------------------------- 5: caller buffers
def test_outputs_land_in_caller_buffers_and_padding_is_untouched():
    dims, n, pad = SMALL9, 33, 40
    critic = wide_critic(dims)
    x, a = batch(dims, n, 133, None)
    q_w = run(critic, x, a, "wide")
    buf = [torch.full((n + pad, 1), NAN, device=DEV) for _ in range(3)]
    ybuf = torch.full((n + pad,), NAN, device=DEV)
    out = critic.forward(x, a, out=(buf[0][:n], buf[1][:n]))
    assert out[0].data_ptr() == buf[0].data_ptr() and out[1].data_ptr() == buf[1].data_ptr()
    reward, done, lp, li, coef = td_inputs(n, n)
    y = critic.td_target(T(reward), x, a, T(done), 0.99, T(lp), T(li), T(coef), out=ybuf[:n], q=(buf[2][:n], buf[0][:n]))
    assert y.data_ptr() == ybuf.data_ptr()
    for b in buf + [ybuf]:
        assert torch.isnan(b[n:]).all() and torch.isfinite(b[:n]).all()
    assert np.array_equal(out[1].cpu().numpy().reshape(-1), q_w[1]) and np.array_equal(buf[2][:n].cpu().numpy().reshape(-1), q_w[0])
    assert np.array_equal(buf[0][:n].cpu().numpy().reshape(-1), q_w[1])        # the second td_target buffer holds q2
    # the learner's views are read in place: [n, V, S / V] and [n, V, A / V]
    q_view = critic.forward(x.view(n, 8, 5), a.view(n, 9, 10))
    assert np.array_equal(q_view[0].cpu().numpy().reshape(-1), q_w[0])


# ---------------------------------------------------------------------------------------------------- 6: the mode
def test_the_mode_is_opt_in_and_refused_outside_its_rule():
    from ris_vec_marl_amd import BatchedTwinCritic
    for dims in ((80, 433, 1024, 512, 256), (80, 288, 1000, 512, 256), (80, 288, 1024, 384, 256)):
        with pytest.raises(ValueError):
            BatchedTwinCritic(*dims, device=DEV, gemm="wide")
    with pytest.raises(ValueError):
        BatchedTwinCritic(*DRIVER16, device=DEV, gemm="fused")
    critic = BatchedTwinCritic(*DRIVER16, device=DEV)
    assert critic.gemm == "library" and critic.pack == "host"
    with pytest.raises(ValueError):
        critic.pack = "device"
    assert BatchedTwinCritic(40, 80, device=DEV).gemm == "fused"
