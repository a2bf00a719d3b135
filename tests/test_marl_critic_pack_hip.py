"""GPU tests of the device weight packing of the SAC twin critic (`risvec_marl_critic_pack`, csrc/k_marl_critic_pack.hip;
`pack_marl_critic_weights_device`, `BatchedTwinCritic.pack = "device"`).

The reference is the host function `pack_marl_critic_weights` on the same tensors.  Nothing is centred here and no sum is
taken: a maximum does not depend on its order, the scaling is a multiplication by a power of two in float64, the two
roundings are correctly rounded.  So the bar is equality: the scales and all three blocks are the same bits, zero padding
included.  The one place two correct implementations could disagree is floor(log2(64 / amax)) where the quotient sits
within a few ulp of a power of two; the header's float32 rule is the specification, and the weights here are drawn so
that log2(64 / amax) of every matrix is at least 1e-3 from an integer (asserted on the CPU copy): ranges of 0.9 /
sqrt(fan_in), because the reference's own 1 / sqrt(fan_in) is a power of two at fan_in = 1024, 256, 64 and a uniform
draw's largest entry then sits just under it.
The forward bars are those of test_marl_critic_hip.py: err < 2e-5 against the float64 restatement of
tests/marl_critic_ref.py, fused <= max(8 x library, 1e-7); y within `y_bound` of `td_target64`.
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import marl_critic_ref as R  # noqa: E402

DEV = "cuda:0"
# (S, A, fc1, fc2, fc3): the driver at 8 and at 4 vehicles; IN = 8: one k-step, half of it padding, one fc1 group for four
# wavefronts, one tile per wavefront; IN = 47: rows no multiple of 4 floats, NG = 3; IN = 17: the second k-step holds one
# column; IN = 128: no padding, every limit at once
SHAPES = [(40, 80, 1024, 512, 256), (20, 24, 1024, 512, 256), (5, 3, 32, 128, 128), (33, 14, 96, 256, 128),
          (16, 1, 64, 128, 256), (64, 64, 1024, 512, 256)]
CASES = [(d, s) for d in SHAPES for s in (1.0, 1e-3)]
NAMES = ("W1", "W2", "W3")
BLOCKS = ("fc1", "fc2", "fc3")
DRIVER = (40, 80, 1024, 512, 256)
SMALL = (33, 14, 96, 256, 128)


def make_weights(dims, scale=1.0, seed=43):
    """(W1, W2, W3) on the device, uniform in +-0.9 / sqrt(fan_in), everything times `scale`."""
    S, A, F1, F2, F3 = dims
    IN = S + A
    g = torch.Generator().manual_seed(seed)
    u = lambda *s, r: (torch.rand(*s, generator=g) * 2 - 1) * (0.9 * r)     # noqa: E731
    w = (u(F1, IN, r=IN ** -0.5), u(F2, F1, r=F1 ** -0.5), u(F3, F2, r=F2 ** -0.5))
    return tuple((v * scale).to(DEV).contiguous() for v in w)


def shift_margin(ws):
    """The smallest distance of log2(64 / amax) from an integer over the matrices, on the CPU copy in float64."""
    out = 1.0
    for t in ws:
        amax = float(t.detach().cpu().double().abs().max())
        if amax > 0:
            v = math.log2(64.0 / amax)
            out = min(out, abs(v - round(v)))
    return out


def poisoned(dims):
    """Output buffers with every byte 0xFF."""
    from ris_vec_marl_amd import marl_critic as MC
    g = MC.marl_critic_geom(*dims)
    return (torch.full((g.rows, 64, 8), -1, dtype=torch.int16, device=DEV).view(torch.float16),
            torch.full((3,), -1, dtype=torch.int32, device=DEV).view(torch.float32))


def device_pack(nets, dims):
    """[(stream, scales)] on the CPU of 1 or 2 nets packed in one call into poisoned buffers."""
    from ris_vec_marl_amd import marl_critic as MC
    out = [poisoned(dims) for _ in nets]
    got = MC.pack_marl_critic_weights_device(list(nets), out=out)
    assert len(got) == len(nets)
    for g, o in zip(got, out):
        assert g[0].data_ptr() == o[0].data_ptr() and g[1].data_ptr() == o[1].data_ptr()
    return [(g[0].cpu(), g[1].cpu()) for g in got]


def host_pack(ws):
    from ris_vec_marl_amd import marl_critic as MC
    hs, hc = MC.pack_marl_critic_weights(*ws)
    return hs.cpu(), hc.cpu()


@functools.lru_cache(maxsize=None)
def packed(dims, scale):
    """(weights, host pack, device pack) of one net of one case, computed once and never modified."""
    w = make_weights(dims, scale)
    return w, host_pack(w), device_pack([w], dims)[0]


def block_rows(dims):
    """{block: slice of the stream's fragment rows} (include/risvec.h); together the whole stream."""
    from ris_vec_marl_amd import marl_critic as MC
    g = MC.marl_critic_geom(*dims)
    return {"fc1": slice(g.fc1, g.fc2), "fc2": slice(g.fc2, g.fc3), "fc3": slice(g.fc3, g.rows)}


def bits(stream):
    return stream.contiguous().view(torch.int16)


def assert_same_bits(dev, host, dims, what):
    (ds, dc), (hs, hc) = dev, host
    rows = block_rows(dims)
    assert ds.shape == hs.shape and sum(r.stop - r.start for r in rows.values()) == ds.shape[0]
    print("%s: scales device %s host %s" % (what, dc.tolist(), hc.tolist()))
    differ = {}
    for part in BLOCKS:
        differ[part] = int((bits(ds)[rows[part]] != bits(hs)[rows[part]]).sum())
        print("%s %s: %d of %d halfs differ from the host pack" % (what, part, differ[part], bits(hs)[rows[part]].numel()))
    assert torch.equal(dc.view(torch.int32), hc.view(torch.int32))
    for part in BLOCKS:
        assert differ[part] == 0, part


@pytest.mark.parametrize("dims,scale", CASES)
def test_against_the_host_pack(dims, scale):
    from ris_vec_marl_amd import marl_critic as MC
    w, host, dev = packed(dims, scale)
    margin = shift_margin(w)
    print("%s x %g: log2(64 / amax) is at least %.3g from an integer" % (dims, scale, margin))
    assert margin >= 1e-3
    assert_same_bits(dev, host, dims, "%s x %g" % (dims, scale))
    # the zero padding of the fc1 block, on its own: inputs beyond state_dims + action_dims
    IN, F1 = dims[0] + dims[1], dims[2]
    g = MC.marl_critic_geom(*dims)
    f1 = bits(dev[0])[block_rows(dims)["fc1"]].reshape(g.ng, g.ks, 2, 2, 32, 8)                     # (g, s, t, h, r, j)
    k = 16 * torch.arange(g.ks)[:, None, None] + 8 * torch.arange(2)[None, :, None] + torch.arange(8)[None, None, :]   # (s, h, j)
    pad = (k >= IN)[None, :, None, :, None, :].expand(g.ng, g.ks, 2, 2, 32, 8)
    print("%s x %g: %d padded fc1 halfs, %d nonzero" % (dims, scale, int(pad.sum()), int((f1[pad] != 0).sum())))
    assert int(pad.sum()) == (16 * g.ks - IN) * F1 * 2 and int((f1[pad] != 0).sum()) == 0


@pytest.mark.parametrize("dims,scale", CASES)
def test_round_trip_against_float64(dims, scale):
    """The bound of test_packing_round_trip_and_stream_size (test_marl_critic_host.py)."""
    from ris_vec_marl_amd import marl_critic as MC
    w, _, (ds, dc) = packed(dims, scale)
    assert bool(torch.isfinite(dc).all()) and all(float(torch.log2(s)) == round(float(torch.log2(s))) for s in dc)   # powers of two
    un = MC._unpack(ds, dc, *dims)
    want = {"fc1": w[0].cpu().double().T, "fc2": w[1].cpu().double().T, "fc3": w[2].cpu().double().T}
    assert set(un) == set(want)
    for name in want:
        assert un[name].shape == want[name].shape
        e, bound = float((un[name] - want[name]).abs().max()), 2.0 ** -21 * float(want[name].abs().max())
        print("%s x %g %s: round trip %.3g (bound %.3g)" % (dims, scale, name, e, bound))
        assert e <= bound


@pytest.mark.parametrize("dims", [DRIVER, SMALL, (5, 3, 32, 128, 128)])
def test_two_nets_in_one_call(dims):
    """Net 2 is 37 x net 1: a workspace slot or a scale shared between the nets would show in either."""
    w1 = make_weights(dims, 1.0, seed=47)
    w2 = tuple((37.0 * t).contiguous() for t in w1)
    assert shift_margin(w1) >= 1e-3 and shift_margin(w2) >= 1e-3
    both = device_pack([w1, w2], dims)
    for c, w in enumerate((w1, w2)):
        assert_same_bits(both[c], host_pack(w), dims, "%s net %d of 2" % (dims, c + 1))
        alone = device_pack([w], dims)[0]
        assert torch.equal(bits(both[c][0]), bits(alone[0])) and torch.equal(both[c][1].view(torch.int32), alone[1].view(torch.int32))
    assert not torch.equal(both[0][1], both[1][1])            # 37 x moves every shift by 5 or 6
    swapped = device_pack([w2, w1], dims)                     # the order of the nets is the caller's
    assert torch.equal(bits(swapped[0][0]), bits(both[1][0])) and torch.equal(bits(swapped[1][0]), bits(both[0][0]))


def test_two_packs_are_byte_identical():
    w, _, (ds, dc) = packed(DRIVER, 1.0)
    es, ec = device_pack([w], DRIVER)[0]
    assert torch.equal(bits(es), bits(ds)) and torch.equal(ec.view(torch.int32), dc.view(torch.int32))


@pytest.mark.parametrize("dims", [SMALL, (20, 24, 1024, 512, 256)])
def test_weights_that_do_not_start_on_16_bytes(dims):
    """Views one float into a larger buffer: W2 and W3 are then read float by float, the result is the same bytes."""
    w, _, (ds, dc) = packed(dims, 1.0)
    off = []
    for v in w:
        buf = torch.zeros(v.numel() + 1, device=DEV)
        t = buf[1:].view(v.shape)
        t.copy_(v)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        off.append(t)
    es, ec = device_pack([tuple(off)], dims)[0]
    assert torch.equal(bits(es), bits(ds)) and torch.equal(ec.view(torch.int32), dc.view(torch.int32))
    # one aligned and one misaligned net in one call: the float-by-float read is chosen for the launch
    w2 = tuple((37.0 * t).contiguous() for t in w)
    mixed = device_pack([tuple(off), w2], dims)
    assert torch.equal(bits(mixed[0][0]), bits(ds))
    assert torch.equal(bits(mixed[1][0]), bits(host_pack(w2)[0]))


@pytest.mark.parametrize("dims", [DRIVER, SMALL])
def test_degenerate_inputs(dims):
    from ris_vec_marl_amd import marl_critic as MC
    rows = block_rows(dims)
    # an all-zero fc3: amax clamps at 1e-30, the shift at 40
    w = list(make_weights(dims))
    w[2] = torch.zeros_like(w[2])
    host = host_pack(w)
    ds, dc = device_pack([tuple(w)], dims)[0]
    print("%s, W3 = 0: scales %s" % (dims, dc.tolist()))
    assert bool(torch.isfinite(dc).all()) and float(dc[2]) == 2.0 ** -40
    assert int((bits(ds)[rows["fc3"]] != 0).sum()) == 0
    assert bool(torch.isfinite(ds.float()).all())
    assert_same_bits((ds, dc), host, dims, "%s, W3 = 0" % (dims,))
    # one huge fc2 entry: the shift turns negative, most lo halves land in the float16 subnormals
    w = list(make_weights(dims))
    w[1] = w[1].clone()
    w[1][3, 5] = 1e4
    host = host_pack(w)
    ds, dc = device_pack([tuple(w)], dims)[0]
    print("%s, W2[3, 5] = 1e4: scales %s" % (dims, dc.tolist()))
    assert float(dc[1]) == 2.0 ** 8
    g = MC.marl_critic_geom(*dims)
    f2 = ds[rows["fc2"]].reshape(4, 2 * g.ng, g.mt2, 2, 64, 8)                         # (w, k, m, t, lane, j)
    assert bool(torch.isfinite(f2[:, :, :, 1].float()).all())
    assert_same_bits((ds, dc), host, dims, "%s, W2[3, 5] = 1e4" % (dims,))
    assert float(MC._unpack(ds, dc, *dims)["fc2"][5, 3]) == 1e4 == float(w[1][3, 5].double())


# ---------------------------------------------------------------------------------------------- in the critic
def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def new_critic(dims=DRIVER, pack="device", n_nets=2, seed=0, gemm="fused"):
    from ris_vec_marl_amd import BatchedTwinCritic
    S, A, F1, F2, F3 = dims
    c = BatchedTwinCritic(S, A, F1, F2, F3, n_nets=n_nets, device=DEV, seed=seed, gemm=gemm)
    c.pack = pack
    return c


def run(critic, x, a, mode):
    """[q_c [n, 1]] of `critic` in `mode`, clones on the device."""
    was, critic.gemm = critic.gemm, mode
    try:
        out = tuple(torch.full((x.shape[0], 1), float("nan"), device=DEV) for _ in range(critic.n_nets))
        q = critic.forward(x, a, out=out if critic.n_nets == 2 else out[0])
        q = q if critic.n_nets == 2 else (q,)
    finally:
        critic.gemm = was
    return [t.clone() for t in q]


def meets_the_bars(critic, x, a, what):
    """Both bars of test_marl_critic_hip.py against the float64 restatement on the weights the critic holds now."""
    sds = [{k: v.numpy() for k, v in sd.items()} for sd in critic.state_dict()]
    q_f, q_l = run(critic, x, a, "fused"), run(critic, x, a, "library")
    refs = []
    for c, sd in enumerate(sds):
        ref64 = R.critic_q64(sd, x.cpu().numpy(), a.cpu().numpy())
        e_f, e_l = R.err(q_f[c].cpu().numpy().reshape(-1), ref64), R.err(q_l[c].cpu().numpy().reshape(-1), ref64)
        print("%s: q%d err fused %.3g library %.3g, max |q64| %.3g" % (what, c + 1, e_f, e_l, np.abs(ref64).max()))
        assert bool(torch.isfinite(q_f[c]).all())
        assert e_l < R.BAR and e_f < R.BAR
        assert e_f <= R.fused_bar(e_l)
        refs.append(ref64)
    return q_f, refs


def streams_of(critic):
    return [net.packed[1][0].data_ptr() for net in critic.nets]


@pytest.mark.parametrize("n_nets", [2, 1])
def test_in_the_loop(n_nets):
    from ris_vec_marl_amd import BatchedTwinCritic
    sds = [{k: T(v) for k, v in R.random_net(DRIVER, 41 + c).items()} for c in range(n_nets)]   # a learner's tensors
    critic = new_critic(n_nets=n_nets)
    assert critic.pack == "device" and critic.gemm == "fused"
    critic.share_state_dict(*sds)
    assert all(getattr(net, v).data_ptr() == sd[k].data_ptr() for net, sd in zip(critic.nets, sds)
               for k, v in BatchedTwinCritic._SD.items())
    x, a = (T(v) for v in R.random_batch(DRIVER, 257, 7, 8))
    q0 = run(critic, x, a, "fused")
    assert critic.packs == n_nets
    streams, workspace = streams_of(critic), critic._pack_workspace.data_ptr()
    run(critic, x, a, "fused")
    assert critic.packs == n_nets                             # nothing changed: nothing rebuilt
    g = torch.Generator(device="cpu").manual_seed(53)
    for sd in sds:                                            # the learner's step: every tensor, in place
        for t in sd.values():
            t.add_((torch.randn(t.shape, generator=g) * 1e-3 * float(t.abs().max())).to(DEV))
    packs = critic.packs
    q1, _ = meets_the_bars(critic, x, a, "n_nets=%d after the in-place update" % n_nets)
    assert critic.packs == packs + n_nets
    assert streams_of(critic) == streams and critic._pack_workspace.data_ptr() == workspace
    assert all(not torch.equal(u, v) for u, v in zip(q0, q1))
    fresh = new_critic(n_nets=n_nets, seed=99)
    fresh.load_state_dict(*[{k: v.cpu().clone() for k, v in sd.items()} for sd in sds])
    assert all(torch.equal(u, v) for u, v in zip(run(fresh, x, a, "fused"), q1))


def test_partial_staleness_and_the_blend():
    from ris_vec_marl_amd import _native as N
    from ris_vec_marl_amd import marl_critic as MC
    dims = DRIVER
    sds = [{k: T(v) for k, v in R.random_net(dims, 81 + c).items()} for c in (0, 1)]
    online = [{k: T(v) for k, v in R.random_net(dims, 91 + c).items()} for c in (0, 1)]
    critic = new_critic(dims)
    critic.share_state_dict(*sds)
    n = 257
    x, a = (T(v) for v in R.random_batch(dims, n, 9, 8))
    run(critic, x, a, "fused")
    streams, packs = streams_of(critic), critic.packs
    kept = critic.nets[0].packed[1][0].clone()
    for k in ("fc1.weight", "fc2.weight", "fc3.weight"):      # net 2 only
        sds[1][k].mul_(1.01)
    q, _ = meets_the_bars(critic, x, a, "after an update of net 2")
    assert critic.packs == packs + 1 and streams_of(critic) == streams
    assert torch.equal(bits(critic.nets[0].packed[1][0]), bits(kept))         # net 1's stream was not written
    want = host_pack(tuple(sds[1][k] for k in ("fc1.weight", "fc2.weight", "fc3.weight")))
    assert torch.equal(bits(critic.nets[1].packed[1][0].cpu()), bits(want[0]))
    # the blend, then the target: 1 + 2 + 1 launches
    packs = critic.packs
    critic.soft_update_from(*online, tau=0.005)
    assert N.last_kernel() == "k_soft_update"
    rng = np.random.default_rng(5)
    reward = rng.uniform(-6, 1, n).astype(np.float32)
    done = rng.uniform(size=n) < 0.25
    lp, li = rng.uniform(-8, 4, n).astype(np.float32), rng.uniform(-12, 0, n).astype(np.float32)
    coef = np.array([0.2, 0.05], np.float32)
    qs = tuple(torch.full((n, 1), float("nan"), device=DEV) for _ in range(2))
    y = critic.td_target(T(reward), x, a, T(done), 0.99, T(lp), T(li), T(coef), q=qs)
    assert critic.packs == packs + 2 and streams_of(critic) == streams
    assert N.last_kernel().startswith("k_marl_critic<")
    q1, q2 = (t.cpu().numpy().reshape(-1) for t in qs)
    g32 = float(np.float32(0.99))
    y64 = R.td_target64(reward, q1, q2, done, g32, coef, lp, li)
    excess = np.abs(y.cpu().numpy().astype(np.float64) - y64) - R.y_bound(reward, q1, q2, g32, coef, lp, li)
    print("after the blend: worst |y - y64| - bound = %.3g over %d live rows" % (excess[~done].max(), int((~done).sum())))
    assert np.isfinite(y.cpu().numpy()).all() and (excess[~done] <= 0).all()
    assert np.array_equal(y.cpu().numpy()[done], reward[done])
    for c, sd in enumerate(critic.state_dict()):              # q against the blended weights
        e = R.err((q1, q2)[c], R.critic_q64({k: v.numpy() for k, v in sd.items()}, x.cpu().numpy(), a.cpu().numpy()))
        print("after the blend: q%d err %.3g" % (c + 1, e))
        assert e < R.BAR
    # the pack kernels are what rebuilt the streams: a stale critic names them when the rebuild is run on its own
    critic.mark_stale()
    critic._fused_weights()
    assert N.last_kernel() == "k_marl_critic_pack x2"
    assert critic.packs == packs + 4
    MC.pack_marl_critic_weights_device([tuple(getattr(critic.nets[1], k) for k in NAMES)])
    assert N.last_kernel() == "k_marl_critic_pack x1"


def test_host_path_against_device_path():
    sds = [R.random_net(DRIVER, 61), R.random_net(DRIVER, 62)]
    x, a = (T(v) for v in R.random_batch(DRIVER, 257, 23, 8))
    out = {}
    for pack in ("host", "device"):
        c = new_critic(pack=pack)
        c.load_state_dict(*sds)
        out[pack], _ = meets_the_bars(c, x, a, "pack=%s" % pack)
    for c in (0, 1):
        d = float((out["host"][c] - out["device"][c]).abs().max())
        print("q%d: largest difference between the two packs %.3g" % (c + 1, d))
        assert torch.equal(out["host"][c], out["device"][c])
    # a change of mode on one critic: stale, rebuilt by the other path, the same q
    c = new_critic(pack="host")
    c.load_state_dict(*sds)
    q_h = run(c, x, a, "fused")
    packs = c.packs
    c.pack = "host"                                           # no change: nothing is marked stale
    run(c, x, a, "fused")
    assert c.packs == packs
    c.pack = "device"
    q_d = run(c, x, a, "fused")
    assert c.packs == packs + 2 and all(torch.equal(u, v) for u, v in zip(q_h, q_d))


def test_dispatch():
    from ris_vec_marl_amd import BatchedTwinCritic
    from ris_vec_marl_amd import marl_critic as MC
    assert BatchedTwinCritic(40, 80, device=DEV).pack == "host"
    for dims in ((40, 80, 1024, 384, 256), (80, 288, 1024, 512, 256)):        # no fused kernel: fc2 = 384; 16 vehicles
        c = BatchedTwinCritic(*dims, device=DEV)
        assert c.gemm == "library" and c.pack == "host"
        with pytest.raises(ValueError):
            c.pack = "device"
        assert c.pack == "host"
        c.pack = "host"
    c = new_critic(pack="device")
    for bad in ("gpu", None, 1):
        with pytest.raises(ValueError):
            c.pack = bad
        assert c.pack == "device"
    w = make_weights(DRIVER)
    for i, bad in ((1, w[1].cpu()), (0, w[0].double()), (2, w[2].T), (2, torch.zeros(256, 256, device=DEV))):
        ws = list(w)
        ws[i] = bad
        with pytest.raises(ValueError):
            MC.pack_marl_critic_weights_device([tuple(ws)])
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights_device([tuple(t.cpu() for t in w)])
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights_device([w, make_weights(SMALL)])          # two nets of different shapes
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights_device([w], out=[(torch.empty(4, device=DEV), torch.empty(3, device=DEV))])
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights_device([w, w], out=[poisoned(DRIVER)])    # one pair for two nets
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights_device([w, w, w])
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights_device([w], workspace=torch.zeros(8, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        out = poisoned(DRIVER)
        MC.pack_marl_critic_weights_device([w, w], out=[out, out])            # two nets into one buffer
