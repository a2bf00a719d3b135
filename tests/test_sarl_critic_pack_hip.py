"""GPU tests of the device weight packing of the DDPG critic (`risvec_sarl_critic_pack`, csrc/k_sarl_critic_pack.hip;
`pack_critic_weights_device`, `BatchedCritic(pack="device")`).

The reference is the host function `pack_critic_weights` on the same tensors.  The scales and the action_value, fc2 and
fc3 blocks must be the same bits, zero padding included.  The fc1 operand is centred with a float64 mean that the
kernel sums in another order than the library, which can move a value across a float32 rounding boundary, so there: at
least 99.9 % of the halfs bit-equal and the unpacked matrix within 2^-22 max|centred fc1| of the host's (the bars of
test_sarl_actor_pack_hip.py, for the same reason; the kernel's 16-way summation order emulated on the CPU at these
five shapes and both scales gave 0 differing halfs).  The forward bars are those of test_sarl_critic_hip.py: err < 2e-5
against the float64 restatement of tests/sarl_critic_ref.py, fused <= max(8 x library, 1e-7).
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import sarl_critic_ref as R  # noqa: E402

DEV = "cuda:0"
# (IN, F1, F2, F3, A): the driver's two shapes; fc1 < 128, so a wavefront of the forward has no fc1 group, one action
# k-step that is mostly padding; IN + 1 fills its k-steps exactly, NG = 3, A no multiple of 4 or 16; every limit at once
SHAPES = [(80, 1024, 512, 256, 56), (104, 1024, 512, 256, 80), (21, 64, 128, 128, 6), (47, 96, 256, 128, 33),
          (128, 1024, 512, 256, 96)]
CASES = [(d, s) for d in SHAPES for s in (1.0, 1e-3)]
NAMES = ("W1", "b1", "W2", "Wav", "W3")
BLOCKS = ("action_value", "fc1", "fc2", "fc3")


def make_weights(dims, scale=1.0, seed=43):
    """The five packed tensors on the device at the reference's init ranges (networks.py:40-58), everything times `scale`."""
    IN, F1, F2, F3, A = dims
    g = torch.Generator().manual_seed(seed)
    u = lambda *s, r: (torch.rand(*s, generator=g) * 2 - 1) * r     # noqa: E731
    w = dict(W1=u(F1, IN, r=F1 ** -0.5), b1=u(F1, r=F1 ** -0.5), W2=u(F2, F1, r=F2 ** -0.5), Wav=u(F2, A, r=F2 ** -0.5),
             W3=u(F3, F2, r=F3 ** -0.5))
    return {k: (v * scale).to(DEV).contiguous() for k, v in w.items()}


def poisoned(dims):
    """Output buffers with every byte 0xFF."""
    from ris_vec_marl_amd import critic as CR
    g = CR.critic_geom(*dims)
    return (torch.full((g.rows, 64, 8), -1, dtype=torch.int16, device=DEV).view(torch.float16),
            torch.full((4,), -1, dtype=torch.int32, device=DEV).view(torch.float32))


def device_pack(w, dims):
    from ris_vec_marl_amd import critic as CR
    out = poisoned(dims)
    got = CR.pack_critic_weights_device(*(w[k] for k in NAMES), out=out)
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    return got[0].cpu(), got[1].cpu()


@functools.lru_cache(maxsize=None)
def packed(dims, scale):
    """(weights, host pack, device pack, unpacked host, unpacked device) of one case, computed once and never modified."""
    from ris_vec_marl_amd import critic as CR
    w = make_weights(dims, scale)
    hs, hc = CR.pack_critic_weights(*(w[k] for k in NAMES))
    host = (hs.cpu(), hc.cpu())
    dev = device_pack(w, dims)
    return w, host, dev, CR.unpack_critic_weights(*host, *dims), CR.unpack_critic_weights(*dev, *dims)


def block_rows(dims):
    """{block: slice of the stream's fragment rows} (include/risvec.h); together the whole stream."""
    from ris_vec_marl_amd import critic as CR
    g = CR.critic_geom(*dims)
    return {"action_value": slice(g.av, g.fc1), "fc1": slice(g.fc1, g.fc2), "fc2": slice(g.fc2, g.fc3), "fc3": slice(g.fc3, g.rows)}


def bits(stream):
    return stream.contiguous().view(torch.int16)


@pytest.mark.parametrize("dims,scale", CASES)
def test_against_the_host_pack(dims, scale):
    from ris_vec_marl_amd import critic as CR
    w, (hs, hc), (ds, dc), uh, ud = packed(dims, scale)
    rows = block_rows(dims)
    assert ds.shape == hs.shape and sum(r.stop - r.start for r in rows.values()) == ds.shape[0]
    print("%s x %g: scales device %s host %s" % (dims, scale, dc.tolist(), hc.tolist()))
    assert torch.equal(dc.view(torch.int32), hc.view(torch.int32))
    for part in ("action_value", "fc2", "fc3"):
        n_diff = int((bits(ds)[rows[part]] != bits(hs)[rows[part]]).sum())
        print("%s x %g %s: %d of %d halfs differ from the host pack" % (dims, scale, part, n_diff, bits(hs)[rows[part]].numel()))
        assert n_diff == 0, part
    # the zero padding of the action_value block, on its own: actions beyond n_actions
    A = dims[4]
    g = CR.critic_geom(*dims)
    av = bits(ds)[rows["action_value"]].reshape(4, g.ksa, g.mt2, 2, 2, 32, 8)          # (w, s, m, t, h, r, j)
    k = (16 * torch.arange(g.ksa)[:, None, None] + 8 * torch.arange(2)[None, :, None] + torch.arange(8)[None, None, :])  # (s, h, j)
    pad = (k >= A)[None, :, None, None, :, None, :].expand(4, g.ksa, g.mt2, 2, 2, 32, 8)
    print("%s x %g: %d padded action halfs, %d nonzero" % (dims, scale, int(pad.sum()), int((av[pad] != 0).sum())))
    assert int(pad.sum()) == (16 * g.ksa - A) * dims[2] * 2 and int((av[pad] != 0).sum()) == 0
    a, b = bits(ds)[rows["fc1"]], bits(hs)[rows["fc1"]]
    differ = int((a != b).sum())
    centred = CR.centre_fc1(w["W1"].cpu(), w["b1"].cpu())
    d_un = float((ud["fc1"] - uh["fc1"]).abs().max())
    bound = 2.0 ** -22 * float(centred.abs().max())
    print("%s x %g: %d of %d fc1 halfs differ from the host pack; unpacked fc1 differs by %.3g (bound %.3g)"
          % (dims, scale, differ, a.numel(), d_un, bound))
    assert differ <= 1e-3 * a.numel()
    assert d_un <= bound


@pytest.mark.parametrize("dims,scale", CASES)
def test_round_trip_against_float64(dims, scale):
    """The bounds of test_packing_round_trip_and_stream_size and test_fc1_operand_columns_sum_to_zero
    (test_sarl_critic_host.py)."""
    from ris_vec_marl_amd import critic as CR
    w, _, (ds, dc), _, ud = packed(dims, scale)
    cw = {k: v.cpu() for k, v in w.items()}
    c = CR.centre_fc1(cw["W1"], cw["b1"])
    assert bool(torch.isfinite(dc).all()) and all(float(torch.log2(s)) == round(float(torch.log2(s))) for s in dc)   # powers of two
    want = {"fc1": c, "fc2": cw["W2"].double().T, "action_value": cw["Wav"].double().T, "fc3": cw["W3"].double().T}
    assert set(ud) == set(want)
    for name in want:
        assert ud[name].shape == want[name].shape
        e, bound = float((ud[name] - want[name]).abs().max()), 2.0 ** -21 * float(want[name].abs().max())
        print("%s x %g %s: round trip %.3g (bound %.3g)" % (dims, scale, name, e, bound))
        assert e <= bound
    rs, bound = float(ud["fc1"].sum(-1).abs().max()), dims[1] * 2.0 ** -22 * float(c.abs().max())
    print("%s x %g: largest fc1 column sum %.3g (bound %.3g)" % (dims, scale, rs, bound))
    assert rs <= bound


@pytest.mark.parametrize("dims", [(80, 1024, 512, 256, 56), (47, 96, 256, 128, 33)])
def test_degenerate_inputs(dims):
    from ris_vec_marl_amd import critic as CR
    rows = block_rows(dims)
    # an all-zero action_value: amax clamps at 1e-30, the shift at 40
    w = dict(make_weights(dims))
    w["Wav"] = torch.zeros_like(w["Wav"])
    hs, hc = (t.cpu() for t in CR.pack_critic_weights(*(w[k] for k in NAMES)))
    ds, dc = device_pack(w, dims)
    print("%s, Wav = 0: scales %s" % (dims, dc.tolist()))
    assert bool(torch.isfinite(dc).all()) and float(dc[2]) == 2.0 ** -40
    assert torch.equal(dc.view(torch.int32), hc.view(torch.int32))
    assert int((bits(ds)[rows["action_value"]] != 0).sum()) == 0
    assert bool(torch.isfinite(ds.float()).all())
    for part in ("action_value", "fc2", "fc3"):
        assert torch.equal(bits(ds)[rows[part]], bits(hs)[rows[part]]), part
    # one huge fc2 entry: the shift turns negative, most lo halves land in the float16 subnormals
    w = dict(make_weights(dims))
    w["W2"] = w["W2"].clone()
    w["W2"][3, 5] = 1e4
    hs, hc = (t.cpu() for t in CR.pack_critic_weights(*(w[k] for k in NAMES)))
    ds, dc = device_pack(w, dims)
    print("%s, W2[3, 5] = 1e4: scales %s" % (dims, dc.tolist()))
    assert float(dc[1]) == 2.0 ** 8 and torch.equal(dc.view(torch.int32), hc.view(torch.int32))
    g = CR.critic_geom(*dims)
    f2 = ds[rows["fc2"]].reshape(4, 2 * g.ng, g.mt2, 2, 64, 8)                         # (w, k, m, t, lane, j)
    assert bool(torch.isfinite(f2[:, :, :, 1].float()).all())
    assert torch.equal(bits(ds)[rows["fc2"]], bits(hs)[rows["fc2"]])
    assert float(CR.unpack_critic_weights(ds, dc, *dims)["fc2"][5, 3]) == 1e4 == float(w["W2"][3, 5].double())


def test_two_packs_are_byte_identical():
    dims = (104, 1024, 512, 256, 80)
    w, _, (ds, dc), _, _ = packed(dims, 1.0)
    es, ec = device_pack(w, dims)
    assert torch.equal(bits(es), bits(ds)) and torch.equal(ec.view(torch.int32), dc.view(torch.int32))


def test_weights_that_do_not_start_on_16_bytes():
    """Views one float into a larger buffer: W2 and W3 are then read float by float, the result is the same bytes."""
    dims = (47, 96, 256, 128, 33)
    w, _, (ds, dc), _, _ = packed(dims, 1.0)
    off = {}
    for k, v in w.items():
        buf = torch.zeros(v.numel() + 1, device=DEV)
        off[k] = buf[1:].view(v.shape)
        off[k].copy_(v)
        assert off[k].data_ptr() % 16 == 4 and off[k].is_contiguous()
    es, ec = device_pack(off, dims)
    assert torch.equal(bits(es), bits(ds)) and torch.equal(ec.view(torch.int32), dc.view(torch.int32))


# ---------------------------------------------------------------------------------------------- in the critic
DRIVER = (80, 1024, 512, 256, 56)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(critic, x, a, mode):
    was, critic.gemm = critic.gemm, mode
    try:
        out = torch.full((x.shape[0], 1), float("nan"), device=DEV)
        q = critic.forward(x, a, out=out).clone()
    finally:
        critic.gemm = was
    return q


def meets_the_bars(critic, x, a, what):
    sd = {k: v.numpy() for k, v in critic.state_dict().items()}
    ref64 = R.critic_q64(sd, x.cpu().numpy(), a.cpu().numpy())
    q_f, q_l = run(critic, x, a, "fused"), run(critic, x, a, "library")
    e_f, e_l = R.err(q_f.cpu().numpy(), ref64), R.err(q_l.cpu().numpy(), ref64)
    print("%s: q err fused %.3g library %.3g, max |q64| %.3g" % (what, e_f, e_l, np.abs(ref64).max()))
    assert bool(torch.isfinite(q_f).all())
    assert e_l < R.BAR and e_f < R.BAR
    assert e_f <= R.fused_bar(e_l)
    return q_f


def new_critic(pack, seed=0):
    from ris_vec_marl_amd import BatchedCritic
    IN, F1, F2, F3, A = DRIVER
    return BatchedCritic(IN, A, F1, F2, F3, device=DEV, seed=seed, gemm="fused", pack=pack)


def test_in_the_loop():
    from ris_vec_marl_amd import BatchedCritic
    from ris_vec_marl_amd import _native as N
    from ris_vec_marl_amd import critic as CR
    sd = {k: T(v) for k, v in R.random_critic(DRIVER, 41).items()}       # a learner's tensors under the reference's names
    critic = new_critic("device")
    assert critic.pack == "device" and critic.gemm == "fused"
    critic.share_state_dict(sd)
    assert all(getattr(critic, v).data_ptr() == sd[k].data_ptr() for k, v in BatchedCritic._SD.items())
    x, a = (T(v) for v in R.random_batch(DRIVER, 257, 7))
    q0 = run(critic, x, a, "fused")
    stream, packs = critic._fused_weights()[0], critic.packs
    assert critic._fused_weights()[0] is stream and critic.packs == packs   # nothing changed: nothing rebuilt
    g = torch.Generator(device="cpu").manual_seed(53)
    for t in sd.values():                                     # the learner's step: every tensor, in place
        t.add_((torch.randn(t.shape, generator=g) * 1e-3 * float(t.abs().max())).to(DEV))
    q1 = meets_the_bars(critic, x, a, "after the in-place update")
    assert critic._fused_weights()[0].data_ptr() == stream.data_ptr() and critic.packs == packs + 1
    assert not torch.equal(q0, q1)
    fresh = new_critic("device", seed=99)
    fresh.load_state_dict({k: v.cpu().clone() for k, v in sd.items()})
    assert torch.equal(run(fresh, x, a, "fused"), q1)
    CR.pack_critic_weights_device(*(getattr(critic, k) for k in NAMES))
    assert N.last_kernel().startswith("k_sarl_critic_pack")


def test_host_path_against_device_path():
    sd = R.random_critic(DRIVER, 61)
    x, a = (T(v) for v in R.random_batch(DRIVER, 257, 23))
    out = {}
    for pack in ("host", "device"):
        c = new_critic(pack)
        c.load_state_dict(sd)
        out[pack] = meets_the_bars(c, x, a, "pack=%s" % pack)
    d = float((out["host"] - out["device"]).abs().max())
    print("largest difference between the q of the two packs: %.3g (largest |q| %.3g)" % (d, float(out["host"].abs().max())))


def test_dispatch():
    from ris_vec_marl_amd import BatchedCritic
    with pytest.raises(ValueError):
        BatchedCritic(80, 56, 1024, 384, 256, device=DEV, pack="device")       # no fused kernel at fc2 = 384
    with pytest.raises(ValueError):
        BatchedCritic(80, 56, device=DEV, pack="gpu")
    assert BatchedCritic(80, 56, device=DEV).pack == "host"
    assert BatchedCritic(80, 56, 1024, 384, 256, device=DEV, pack="host").gemm == "library"
    from ris_vec_marl_amd import critic as CR
    w = make_weights((80, 1024, 512, 256, 56))
    for k, bad in (("W2", w["W2"].cpu()), ("b1", w["b1"].double()), ("Wav", w["Wav"].T), ("W3", torch.zeros(256, 256, device=DEV))):
        with pytest.raises(ValueError):
            CR.pack_critic_weights_device(*({**w, k: bad}[n] for n in NAMES))
    with pytest.raises(ValueError):
        CR.pack_critic_weights_device(*(w[n] for n in NAMES), out=(torch.empty(4, device=DEV), torch.empty(4, device=DEV)))
