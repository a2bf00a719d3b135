"""GPU tests of the device weight packing of the DDPG actor (`risvec_sarl_actor_pack`, csrc/k_sarl_actor_pack.hip;
`pack_actor_weights_device`, `BatchedActor(pack="device")`, `share_state_dict`).

The reference is the host function `pack_actor_weights` on the same tensors.  Everything but the fc1 fragments must be
the same bits.  The fc1 operand is centred with a float64 mean that the kernel sums in another order than the library,
which can move a value across a float32 rounding boundary, so there: at least 99.9 % of the halfs bit-equal and the
unpacked matrix within 2^-22 max|centred fc1| of the host's (the host function against itself is 100 % equal; a flip
needs a float64 value within about 1e-16 relative of a float32 rounding midpoint).  The forward bars are those of
test_sarl_actor_hip.py: err = max |logits - logits64| / max(rowmax |logits64|, 1e-3) < 2e-5, fused <= max(8 x library, 1e-7).
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle.policy_oracle import layer_norm  # noqa: E402  (checker)

DEV = "cuda:0"
BAR = 2e-5
# (IN, F1, F2, A): the driver's two shapes; KS = 3, two groups, a nearly empty pass-1 item; IN + 1 fills the k-steps, NG = 3
# is no multiple of the groups per pass-1 item, the head padded by 31 columns; every limit at once
SHAPES = [(80, 512, 256, 56), (104, 512, 256, 80), (21, 64, 128, 6), (47, 96, 128, 33), (128, 1024, 256, 96)]
CASES = [(d, s) for d in SHAPES for s in (1.0, 1e-3)]
NAMES = ("W1", "b1", "ln1_w", "ln1_b", "W2", "Wmu")


def make_weights(dims, scale=1.0, seed=41):
    """The six packed tensors on the device: the reference's init ranges (networks.py:115-125), LayerNorm weights in
    [0.5, 1.5] and biases in +-0.2, everything times `scale`."""
    IN, F1, F2, A = dims
    g = torch.Generator().manual_seed(seed)
    u = lambda *s, r: (torch.rand(*s, generator=g) * 2 - 1) * r     # noqa: E731
    w = dict(W1=u(F1, IN, r=F1 ** -0.5), b1=u(F1, r=F1 ** -0.5), ln1_w=0.5 + torch.rand(F1, generator=g), ln1_b=u(F1, r=0.2),
             W2=u(F2, F1, r=F2 ** -0.5), Wmu=u(A, F2, r=0.003))
    return {k: (v * scale).to(DEV).contiguous() for k, v in w.items()}


def poisoned(dims):
    """Output buffers with every byte 0xFF."""
    from ris_vec_marl_amd import actor as ACT
    g = ACT.actor_geom(*dims)
    return (torch.full((g.items, g.rows, 64, 8), -1, dtype=torch.int16, device=DEV).view(torch.float16),
            torch.full((3,), -1, dtype=torch.int32, device=DEV).view(torch.float32))


def device_pack(w, dims):
    from ris_vec_marl_amd import actor as ACT
    out = poisoned(dims)
    got = ACT.pack_actor_weights_device(*(w[k] for k in NAMES), out=out)
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    return got[0].cpu(), got[1].cpu()


@functools.lru_cache(maxsize=None)
def packed(dims, scale):
    """(weights, host pack, device pack, unpacked host, unpacked device) of one case, computed once and never modified."""
    from ris_vec_marl_amd import actor as ACT
    w = make_weights(dims, scale)
    hs, hc = ACT.pack_actor_weights(*(w[k] for k in NAMES))
    host = (hs.cpu(), hc.cpu())
    dev = device_pack(w, dims)
    return w, host, dev, ACT.unpack_actor_weights(*host, *dims), ACT.unpack_actor_weights(*dev, *dims)


def row_masks(dims):
    """{"fc1", "ln", "fc2", "head"}: bool [items, rows], which fragment rows of the stream hold what (include/risvec.h)."""
    from ris_vec_marl_amd import actor as ACT
    g = ACT.actor_geom(*dims)
    m = {k: torch.zeros(g.items, g.rows, dtype=torch.bool) for k in ("fc1", "ln", "fc2", "head")}
    for grp in range(g.ng):
        it, at = divmod(grp, g.p1)
        m["fc1"][it, 2 * g.ks * at:2 * g.ks * (at + 1)] = True
    m["fc1"][g.t1:g.t1 + g.ng, :2 * g.ks] = True
    m["ln"][g.t1:g.t1 + g.ng, 2 * g.ks] = True
    m["fc2"][g.t1:g.t1 + g.ng, 2 * g.ks + 1:2 * g.ks + 1 + 4 * g.mt] = True
    for st in range(2 * g.mt):
        it, at = divmod(st, g.hs)
        m["head"][g.t1 + g.ng + it, 2 * g.ht * at:2 * g.ht * (at + 1)] = True
    assert int(sum(v.sum() for v in m.values())) == int(torch.stack(list(m.values())).any(0).sum())    # disjoint
    return m


def bits(stream):
    return stream.contiguous().view(torch.int16)


@pytest.mark.parametrize("dims,scale", CASES)
def test_against_the_host_pack(dims, scale):
    from ris_vec_marl_amd import actor as ACT
    w, (hs, hc), (ds, dc), uh, ud = packed(dims, scale)
    m = row_masks(dims)
    assert torch.equal(dc.view(torch.int32), hc.view(torch.int32)), (dc, hc)
    for part in ("ln", "fc2", "head"):
        assert torch.equal(bits(ds)[m[part]], bits(hs)[m[part]]), part
    rest = ~(m["fc1"] | m["ln"] | m["fc2"] | m["head"])
    assert int((bits(ds)[rest] != 0).sum()) == 0 and int((bits(hs)[rest] != 0).sum()) == 0
    a, b = bits(ds)[m["fc1"]], bits(hs)[m["fc1"]]
    differ = int((a != b).sum())
    centred = ACT.centre_fc1(w["W1"].cpu(), w["b1"].cpu())
    d_un = float((ud["fc1"] - uh["fc1"]).abs().max())
    bound = 2.0 ** -22 * float(centred.abs().max())
    print("%s x %g: %d of %d fc1 halfs differ from the host pack; unpacked fc1 differs by %.3g (bound %.3g); rows outside "
          "the fragments: %d" % (dims, scale, differ, a.numel(), d_un, bound, int(rest.sum())))
    assert differ <= 1e-3 * a.numel()
    assert d_un <= bound
    assert float((ud["fc1_pass1"] - uh["fc1_pass1"]).abs().max()) <= bound


@pytest.mark.parametrize("dims,scale", CASES)
def test_both_fc1_copies_are_the_same(dims, scale):
    _, _, _, _, ud = packed(dims, scale)
    assert torch.equal(ud["fc1"], ud["fc1_pass1"])


@pytest.mark.parametrize("dims,scale", CASES)
def test_round_trip_against_float64(dims, scale):
    """The bounds of test_packing_round_trip and test_centred_fc1_rows_sum_to_zero (test_sarl_actor_host.py)."""
    from ris_vec_marl_amd import actor as ACT
    w, _, (ds, dc), _, ud = packed(dims, scale)
    cw = {k: v.cpu() for k, v in w.items()}
    c = ACT.centre_fc1(cw["W1"], cw["b1"])
    assert all(float(torch.log2(s)) == round(float(torch.log2(s))) for s in dc)           # powers of two
    for name, got, want in (("fc1", ud["fc1"], c), ("fc1_pass1", ud["fc1_pass1"], c), ("fc2", ud["fc2"], cw["W2"].double().T),
                            ("mu", ud["mu"], cw["Wmu"].double().T)):
        assert got.shape == want.shape
        e, bound = float((got - want).abs().max()), 2.0 ** -21 * float(want.abs().max())
        print("%s x %g %s: round trip %.3g (bound %.3g)" % (dims, scale, name, e, bound))
        assert e <= bound
    assert torch.equal(ud["ln1_w"].float(), cw["ln1_w"]) and torch.equal(ud["ln1_b"].float(), cw["ln1_b"])
    rs, bound = float(ud["fc1"].sum(-1).abs().max()), dims[1] * 2.0 ** -22 * float(c.abs().max())
    print("%s x %g: largest fc1 row sum %.3g (bound %.3g)" % (dims, scale, rs, bound))
    assert rs <= bound


@pytest.mark.parametrize("dims", [(80, 512, 256, 56), (47, 96, 128, 33)])
def test_degenerate_inputs(dims):
    from ris_vec_marl_amd import actor as ACT
    m = row_masks(dims)
    # an all-zero head: amax clamps at 1e-30, the shift at 40
    w = dict(make_weights(dims))
    w["Wmu"] = torch.zeros_like(w["Wmu"])
    hs, hc = (t.cpu() for t in ACT.pack_actor_weights(*(w[k] for k in NAMES)))
    ds, dc = device_pack(w, dims)
    assert bool(torch.isfinite(dc).all()) and float(dc[2]) == 2.0 ** -40
    assert torch.equal(dc.view(torch.int32), hc.view(torch.int32))
    assert int((bits(ds)[m["head"]] != 0).sum()) == 0
    for part in ("ln", "fc2", "head"):
        assert torch.equal(bits(ds)[m[part]], bits(hs)[m[part]]), part
    # one huge fc2 entry: the shift turns negative, most lo halves land in the float16 subnormals
    w = dict(make_weights(dims))
    w["W2"] = w["W2"].clone()
    w["W2"][3, 5] = 1e4
    hs, hc = (t.cpu() for t in ACT.pack_actor_weights(*(w[k] for k in NAMES)))
    ds, dc = device_pack(w, dims)
    assert float(dc[1]) == 2.0 ** 8 and torch.equal(dc.view(torch.int32), hc.view(torch.int32))
    g = ACT.actor_geom(*dims)
    f2 = ds[g.t1:g.t1 + g.ng, 2 * g.ks + 1:2 * g.ks + 1 + 4 * g.mt].reshape(g.ng, 2, 2, g.mt, 64, 8)   # (g, u, t, m, lane, j)
    assert bool(torch.isfinite(f2[:, :, 1].float()).all())
    assert torch.equal(bits(ds)[m["fc2"]], bits(hs)[m["fc2"]])
    assert float(ACT.unpack_actor_weights(ds, dc, *dims)["fc2"][5, 3]) == 1e4 == float(w["W2"][3, 5].double())


def test_two_packs_are_byte_identical():
    w, _, (ds, dc), _, _ = packed((104, 512, 256, 80), 1.0)
    es, ec = device_pack(w, (104, 512, 256, 80))
    assert torch.equal(bits(es), bits(ds)) and torch.equal(ec.view(torch.int32), dc.view(torch.int32))


# ---------------------------------------------------------------------------------------------- in the actor
def forward64(sd, x):
    """networks.py:132-141 in float64 (pre-sigmoid values); sd: the reference's state_dict names -> arrays."""
    W = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    h = np.asarray(x, np.float64).reshape(len(x), -1) @ W["fc1.weight"].T + W["fc1.bias"]
    h = np.maximum(layer_norm(h, W["bn1.weight"], W["bn1.bias"]), 0.0)
    h = h @ W["fc2.weight"].T + W["fc2.bias"]
    h = np.maximum(layer_norm(h, W["bn2.weight"], W["bn2.bias"]), 0.0)
    return h @ W["mu.weight"].T + W["mu.bias"]


def err(logits, ref64):
    scale = np.maximum(np.abs(ref64).max(-1, keepdims=True), 1e-3)
    return float((np.abs(np.asarray(logits, np.float64) - ref64) / scale).max())


def obs_like(rng, n, V, tn):
    """Observation-shaped inputs (ddpg_train.py:134-149): phase slice in [0, 2 pi), five scalars in [0, 1.2], one zero."""
    o = np.empty((n, V, tn + 5), np.float32)
    o[:, :, :tn] = rng.uniform(0, 2 * np.pi, (n, V, tn))
    o[:, :, tn:] = rng.uniform(0, 1.2, (n, V, 5))
    o[:, :, tn + 3] = 0.0
    return torch.from_numpy(o).to(DEV)


def learner_tensors(seed=51):
    """A learner's actor at the driver's shape, as device tensors under the reference's key names: the init ranges of
    `driver_actor` in test_sarl_actor_hip.py (the head widened 60 x, LayerNorm weights in [0.5, 1.5], biases in +-0.2)."""
    from ris_vec_marl_amd import BatchedActor
    a = BatchedActor(80, 56, 512, 256, device=DEV, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    a.Wmu.mul_(60.0)
    for w, b in ((a.ln1_w, a.ln1_b), (a.ln2_w, a.ln2_b)):
        w.copy_(0.5 + torch.rand(w.shape, generator=g))
        b.copy_((torch.rand(b.shape, generator=g) * 2 - 1) * 0.2)
    return {k: getattr(a, v).clone() for k, v in BatchedActor._SD.items()}


def logits_mu(actor, x, gemm="fused"):
    was, actor.gemm = actor.gemm, gemm
    try:
        lg = torch.full((x.shape[0], actor.n_actions), float("nan"), device=DEV)
        mu = actor.forward(x, logits=lg).clone()
    finally:
        actor.gemm = was
    return lg, mu


def meets_the_bars(actor, x, what):
    sd = {k: v.numpy() for k, v in actor.state_dict().items()}
    ref64 = forward64(sd, x.cpu().numpy())
    lg, mu = logits_mu(actor, x)
    e_f, e_l = err(lg.cpu().numpy(), ref64), err(logits_mu(actor, x, "library")[0].cpu().numpy(), ref64)
    print("%s: logits err fused %.3g library %.3g" % (what, e_f, e_l))
    assert bool(torch.isfinite(lg).all()) and bool(torch.isfinite(mu).all())
    assert e_l < BAR and e_f < BAR
    assert e_f <= max(8 * e_l, 1e-7)
    return lg, mu


def test_in_the_loop():
    from ris_vec_marl_amd import BatchedActor
    from ris_vec_marl_amd import _native as N
    from ris_vec_marl_amd import actor as ACT
    sd = learner_tensors()
    actor = BatchedActor(80, 56, 512, 256, device=DEV, pack="device")
    assert actor.pack == "device" and actor.gemm == "fused"
    actor.share_state_dict(sd)
    assert all(getattr(actor, v).data_ptr() == sd[k].data_ptr() for k, v in BatchedActor._SD.items())
    x = obs_like(np.random.default_rng(19), 257, 8, 5)
    lg0, mu0 = logits_mu(actor, x)
    stream = actor._fused_weights()[0]
    assert actor._fused_weights()[0] is stream                # nothing changed: nothing rebuilt
    g = torch.Generator(device="cpu").manual_seed(53)
    for t in sd.values():                                     # the learner's step: every tensor, in place
        t.add_((torch.randn(t.shape, generator=g) * 1e-3 * float(t.abs().max())).to(DEV))
    lg1, mu1 = meets_the_bars(actor, x, "after the in-place update")
    assert actor._fused_weights()[0].data_ptr() == stream.data_ptr()
    assert not torch.equal(lg0, lg1) and not torch.equal(mu0, mu1)
    fresh = BatchedActor(80, 56, 512, 256, device=DEV, seed=99, pack="device")
    fresh.load_state_dict({k: v.cpu().clone() for k, v in sd.items()})
    lg2, mu2 = logits_mu(fresh, x)
    assert torch.equal(lg1, lg2) and torch.equal(mu1, mu2)
    ACT.pack_actor_weights_device(*(getattr(actor, k) for k in NAMES))
    assert N.last_kernel().startswith("k_sarl_actor_pack")


def test_host_path_against_device_path():
    from ris_vec_marl_amd import BatchedActor
    sd = {k: v.cpu() for k, v in learner_tensors(seed=61).items()}
    x = obs_like(np.random.default_rng(23), 257, 8, 5)
    out = {}
    for pack in ("host", "device"):
        a = BatchedActor(80, 56, 512, 256, device=DEV, pack=pack)
        a.load_state_dict(sd)
        out[pack] = meets_the_bars(a, x, "pack=%s" % pack)[0]
    assert BatchedActor(80, 56, 512, 256, device=DEV).pack == "host"
    d = float((out["host"] - out["device"]).abs().max())
    print("largest difference between the logits of the two packs: %.3g (largest |logit| %.3g)" % (d, float(out["host"].abs().max())))


def test_argument_errors():
    from ris_vec_marl_amd import BatchedActor
    from ris_vec_marl_amd import actor as ACT
    with pytest.raises(ValueError):
        BatchedActor(80, 56, 512, 64, device=DEV, pack="device")          # no fused kernel at fc2 = 64
    with pytest.raises(ValueError):
        BatchedActor(80, 56, 512, 256, device=DEV, pack="gpu")
    assert BatchedActor(80, 56, 512, 64, device=DEV, pack="host").gemm == "library"
    actor = BatchedActor(80, 56, 512, 256, device=DEV, pack="device")
    sd = learner_tensors()
    kept = actor.W2
    for k, bad in (("fc2.weight", sd["fc2.weight"].cpu()), ("fc1.bias", sd["fc1.bias"].double()),
                   ("mu.weight", torch.empty(256, 56, device=DEV).T), ("fc1.weight", sd["fc1.weight"][:, :79].contiguous())):
        with pytest.raises(ValueError):
            actor.share_state_dict({**sd, k: bad})
    assert actor.W2 is kept
    w = make_weights((80, 512, 256, 56))
    for k, bad in (("W2", w["W2"].cpu()), ("b1", w["b1"].double()), ("Wmu", w["Wmu"].T), ("W2", torch.zeros(64, 512, device=DEV))):
        with pytest.raises(ValueError):
            ACT.pack_actor_weights_device(*({**w, k: bad}[n] for n in NAMES))
    with pytest.raises(ValueError):
        ACT.pack_actor_weights_device(*(w[n] for n in NAMES), out=(torch.empty(3, device=DEV), torch.empty(3, device=DEV)))
