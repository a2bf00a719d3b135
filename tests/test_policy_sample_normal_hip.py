"""GPU tests of `risvec_policy_sample_normal` / `BatchedPolicy.sample_normal` (csrc/k_policy_learn.hip): the learner's
`policy.sample_normal` for every row and agent in one launch, its next_actions row and its log-probability sums.

Reference: tests/policy_logp_ref.py, the float64 restatement of sac_agent.py:80-127 that test_policy_sample_normal_host.py
pins to the reference's own outputs.  Bounds (that module): logp_power within rel |ref| + 2^-20 + the row's two
saturation floors, logp_intent within rel |ref| + 2^-20, rel = 1e-5 on float32 heads taken as given and 2e-5 where the
heads come from the device forward (whose heads the policy tests allow 5e-6 on); power / probs 2e-5 absolute as
tests/test_policy_hip.py; the one-hot exact where the top two soft probabilities are further apart than 1e-4, and a
straight-through (hard) row, being its arg-max, judged where that is decided.  The sums over the agents are compared
BIT FOR BIT with a NumPy float32 loop over the per-agent outputs of the same launch.  `[logp margin]` lines print the
largest error of each quantity next to its bound."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import policy_oracle as PO  # noqa: E402  (checker)
from tests import marl_critic_ref as CR  # noqa: E402
from tests import policy_logp_ref as R  # noqa: E402

DEV = "cuda:0"
KBLOCK = 256
NAN = float("nan")
OUTS = dict(power=lambda B, V: (B, V, 2), probs=lambda B, V: (B, V, V), next_actions=lambda B, V: (B, V, V + 2),
            logp_power=lambda B, V: (B, V), logp_intent=lambda B, V: (B, V), logp_power_sum=lambda B, V: (B,),
            logp_intent_sum=lambda B, V: (B,))


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def rows_per_block(V):
    """Batch rows one workgroup owns: (kBlock / pow2ceil(V)) / V slots; 0 above 16 agents."""
    return (KBLOCK // (1 << max(0, (V - 1).bit_length()))) // V


def guarded(n):
    """n floats to be written (NaN until then) and 64 behind them that must stay as they are."""
    buf = torch.full((n + 64,), NAN, device=DEV)
    buf[n:] = 12345.0
    return buf


def native(heads, mask, tau, hard, eps=None, expo=None, seed=0, counter=0, row_offset=0, want=tuple(OUTS), rc_only=False):
    """risvec_policy_sample_normal on host-made float32 heads [V,B,4+V]; every output into a guarded buffer."""
    from ris_vec_marl_amd import _native as N
    V, B, H = heads.shape
    assert H == 4 + V and heads.dtype == np.float32
    lib, st = N.load(), torch.cuda.current_stream().cuda_stream
    h, tt, hd = T(heads), T(np.asarray(tau, np.float32)), T(np.asarray(hard, np.uint8))
    mk = None if mask is None else T(mask.astype(np.uint8))
    ep = None if eps is None else T(eps.astype(np.float32))
    ex = None if expo is None else T(expo.astype(np.float32))
    bufs = {k: guarded(int(np.prod(OUTS[k](B, V)))) if k in want else None for k in OUTS}
    rc = lib.risvec_policy_sample_normal(B, V, row_offset, h.data_ptr(), N.ptr(mk), tt.data_ptr(), hd.data_ptr(), N.ptr(ep),
                                         N.ptr(ex), seed, counter, *(N.ptr(bufs[k]) for k in OUTS), st)
    if rc_only:
        return rc
    N.check(rc)
    torch.cuda.synchronize()
    out = {}
    for k in want:
        n = int(np.prod(OUTS[k](B, V)))
        assert bool((bufs[k][n:] == 12345.0).all()), "%s: written past its end" % k
        out[k] = bufs[k][:n].cpu().numpy().reshape(OUTS[k](B, V))
        assert np.isfinite(out[k]).all(), "%s: not finite or not written" % k
    return out


def choose_native(heads, mask, tau, hard, eps=None, expo=None, seed=0, counter=0, env_offset=0):
    """risvec_policy_sample (the choose_action kernel) on the same inputs -> power_raw, probs, onehot"""
    from ris_vec_marl_amd import _native as N
    V, B, _ = heads.shape
    lib, st = N.load(), torch.cuda.current_stream().cuda_stream
    h, tt, hd = T(heads), T(np.asarray(tau, np.float32)), T(np.asarray(hard, np.uint8))
    mk = None if mask is None else T(mask.astype(np.uint8))
    ep = None if eps is None else T(eps.astype(np.float32))
    ex = None if expo is None else T(expo.astype(np.float32))
    power, probs, onehot = (torch.full(s, NAN, device=DEV) for s in ((B, V, 2), (B, V, V), (B, V, V)))
    N.check(lib.risvec_policy_sample(B, V, env_offset, h.data_ptr(), N.ptr(mk), tt.data_ptr(), hd.data_ptr(), N.ptr(ep), N.ptr(ex),
                                     seed, counter, 0.1, power.data_ptr(), probs.data_ptr(), onehot.data_ptr(), None, None, None, st))
    torch.cuda.synchronize()
    return power.cpu().numpy(), probs.cpu().numpy(), onehot.cpu().numpy()


def make_inputs(V, B, seed, masked, tau):
    """Heads with mu in [-1.5, 1.5], log_std in [-3, -0.5], logits in [-3, 3]; |eps| <= 3: |x_t| <= 3.4 and every
    saturation floor is below 5e-5.  The mask has an all-zero row (row 0, agent 0: opened up) and a row with a single
    open entry (last row, last agent)."""
    rng = np.random.default_rng(seed)
    heads = np.empty((V, B, 4 + V), np.float32)
    heads[..., 0:2] = rng.uniform(-1.5, 1.5, (V, B, 2))
    heads[..., 2:4] = rng.uniform(-3.0, -0.5, (V, B, 2))
    heads[..., 4:] = rng.uniform(-3.0, 3.0, (V, B, V))
    eps = np.clip(rng.normal(size=(B, V, 2)), -3.0, 3.0).astype(np.float32)
    expo = np.maximum(rng.exponential(size=(B, V, V)), 1e-6).astype(np.float32)
    mask = None
    if masked:
        mask = (rng.uniform(size=(B, V, V)) < 0.7).astype(np.uint8)
        mask[0, 0] = 0
        mask[B - 1, V - 1] = 0
        mask[B - 1, V - 1, (V - 1) // 2] = 1
    hard = (np.arange(V) % 3 == 1).astype(np.uint8)
    return heads, mask, np.full(V, tau, np.float32), hard, eps, expo


def margin(what, name, err, bound):
    ratio = err / np.maximum(bound, 1e-300)
    i = int(np.argmax(ratio))
    print("[logp margin] %s: %s max err %.3g, bound there %.3g, max err / bound %.3f"
          % (what, name, err.max(), np.broadcast_to(bound, err.shape).ravel()[i], ratio.max()))


def assert_outputs(got, want, hard, what, rel=R.REL):
    """Per-agent outputs within their bounds on every row."""
    clear = want["clear"]
    hard_rows = np.broadcast_to(np.asarray(hard, bool)[None, :], clear.shape)
    judged = clear | ~hard_rows
    B, V = clear.shape
    for k, ref in (("power", want["power"]), ("probs", want["y"])):
        err = np.abs(got[k].astype(np.float64) - ref)
        if k == "probs":
            err = err[judged]
        margin(what, k, err, np.float64(2e-5))
        assert (err <= 2e-5).all(), (what, k)
    na = got["next_actions"].reshape(B, V, V + 2)
    assert np.array_equal(na[:, :, :V][clear], want["onehot"][clear]), what
    assert ((na[:, :, :V] == 0) | (na[:, :, :V] == 1)).all() and (na[:, :, :V].sum(-1) == 1).all()
    assert np.array_equal(na[:, :, V:].view(np.uint32), got["power"].view(np.uint32)), "next_actions' powers are `power`"
    e_p, b_p = np.abs(got["logp_power"] - want["logp_power"]), R.bound_power(want["logp_power"], want["floor"], rel)
    margin(what, "logp_power", e_p, b_p)
    assert (e_p <= b_p).all(), (what, np.argwhere(e_p > b_p)[:5], e_p.max())
    e_i, b_i = np.abs(got["logp_intent"] - want["logp_intent"])[judged], R.bound_intent(want["logp_intent"], rel)[judged]
    margin(what, "logp_intent", e_i, b_i)
    assert (e_i <= b_i).all(), (what, np.argwhere(e_i > b_i)[:5], e_i.max())


def f32_sum_in_agent_order(x):
    acc = np.zeros(x.shape[0], np.float32)
    for v in range(x.shape[1]):
        acc = (acc + x[:, v]).astype(np.float32)
    return acc


def assert_sums_bitwise(got, what):
    for k in ("logp_power", "logp_intent"):
        want = f32_sum_in_agent_order(got[k])
        assert np.array_equal(got[k + "_sum"].view(np.uint32), want.view(np.uint32)), (what, k)


# ------------------------------------------------------------------------------------------- 1: golden, end to end
@pytest.mark.parametrize("gemm", ["fp32", "default"])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_golden_end_to_end(name, gemm):
    from ris_vec_marl_amd import BatchedPolicy
    fx = R.fixture(name)
    V, B = int(fx["V"]), int(fx["B"])
    pol = BatchedPolicy(V, 5, int(fx["fc1"]), int(fx["fc2"]), device=DEV, gemm=None if gemm == "default" else gemm)
    for a in range(V):
        pol.load_agent_state_dict(a, R.agent_weights(fx, a))
        pol.tau[a] = float(fx["tau"][a])
        pol.gumbel_hard[a] = int(fx["hard"][a])
    obs = np.stack([fx["state"][a] for a in range(V)], 1)
    mask = np.stack([fx["mask"][a] if fx["has_mask"][a] else np.ones((B, V), np.float32) for a in range(V)], 1)
    eps, expo = np.stack(list(fx["eps"]), 1), np.stack(list(fx["expo"]), 1)
    calls = pol._calls
    ret = pol.sample_normal(T(obs), T(mask), T(eps), T(expo))
    assert pol._calls == calls + 1
    got = {k: t.cpu().numpy() for k, t in zip(("power", "probs", "logp_power", "logp_intent", "next_actions",
                                               "logp_power_sum", "logp_intent_sum"), ret)}
    assert got["next_actions"].shape == (B, V * (V + 2)) and got["logp_power_sum"].shape == (B,)
    # the float64 restatement on the fixture's own float32 heads
    heads = np.concatenate([fx["mu"], fx["log_std"], fx["logits"]], -1).astype(np.float32)          # [V, B, 4 + V]
    want = R.batch(heads, mask, fx["tau"], fx["hard"], eps, expo)
    what = "%s gemm=%s" % (name, pol.gemm)
    assert_outputs(got, want, fx["hard"], what, rel=R.REL_DEVICE_HEADS)
    assert_sums_bitwise(got, what)
    # and, for the record, against the reference's own float32 outputs at the same bounds
    ref_p, ref_i = fx["logp_power"].T.astype(np.float64), fx["logp_intent"].T.astype(np.float64)
    margin(what, "logp_power vs the reference's float32", np.abs(got["logp_power"] - ref_p),
           R.bound_power(ref_p, want["floor"], R.REL_DEVICE_HEADS))
    margin(what, "logp_intent vs the reference's float32", np.abs(got["logp_intent"] - ref_i), R.bound_intent(ref_i, R.REL_DEVICE_HEADS))
    # the library-kernel statement of the same computation agrees too
    lib = pol.sample_normal_torch(T(obs), T(mask), T(eps), T(expo))
    got_l = {k: t.cpu().numpy() for k, t in zip(("power", "probs", "logp_power", "logp_intent", "next_actions"), lib)}
    assert_outputs(got_l, want, fx["hard"], what + " (sample_normal_torch)", rel=R.REL_DEVICE_HEADS)


# ------------------------------------------------------------------------------------------- 2: the kernel alone
SHAPES = [(V, B) for V in (4, 5, 8, 16) for B in sorted({1, rows_per_block(V) - 1, rows_per_block(V) + 1, 2 * rows_per_block(V) + 1})]


@functools.lru_cache(maxsize=None)
def kernel_case(V, B, masked, tau):
    """(inputs, float64 reference, device outputs) of one case, computed once and shared (never modified)."""
    inp = make_inputs(V, max(B, 1), 1000 * V + B + (7 if masked else 0), masked, tau)
    heads, mask, taus, hard, eps, expo = inp
    want = R.batch(heads, mask, taus, hard, eps, expo)
    assert want["floor"].max() <= 5e-5                         # nothing saturates: no sample is left out
    got = native(heads, mask, taus, hard, eps, expo)
    return inp, want, got


@pytest.mark.parametrize("tau", [2.0, 0.3])
@pytest.mark.parametrize("masked", [False, True], ids=["open", "masked"])
@pytest.mark.parametrize("V,B", SHAPES)
def test_kernel_on_host_made_heads(V, B, masked, tau):
    if B == 0:                                                 # V = 16 owns one row per workgroup: n - 1 is the empty batch
        heads, mask, taus, hard, eps, expo = make_inputs(V, 1, 5, masked, tau)
        assert native(heads[:, :0], None, taus, hard, rc_only=True) == 0
        return
    (heads, mask, taus, hard, eps, expo), want, got = kernel_case(V, B, masked, tau)
    what = "V=%d B=%d %s tau=%g" % (V, B, "masked" if masked else "open", tau)
    assert_outputs(got, want, hard, what)
    assert_sums_bitwise(got, what)
    if masked:
        blocked = (mask == 0) & (mask.sum(-1, keepdims=True) > 0)
        assert (got["probs"][blocked] == 0.0).all()
        last = (V - 1) // 2                                    # the single open entry: probability 1, log-probability 0
        assert got["probs"][B - 1, V - 1, last] == 1.0 and abs(got["logp_intent"][B - 1, V - 1]) <= 2.0 ** -20
        if V > 1:
            assert (got["probs"][0, 0] > 0).sum() > 1 or hard[0]        # the all-zero row is opened up


# ------------------------------------------------------------------------------------------- 3: sums
@pytest.mark.parametrize("V", [4, 8, 16])
def test_sums_equal_the_float32_loop_bit_for_bit(V):
    n = rows_per_block(V)
    B = 3 * n + 2
    heads, mask, taus, hard, eps, expo = make_inputs(V, B, 31 + V, True, 1.0)
    got = native(heads, mask, taus, hard, eps, expo)
    assert_sums_bitwise(got, "sums V=%d B=%d" % (V, B))
    only = native(heads, mask, taus, hard, eps, expo, want=("logp_power_sum", "logp_intent_sum"))    # nothing else asked for
    assert np.array_equal(only["logp_power_sum"].view(np.uint32), got["logp_power_sum"].view(np.uint32))
    assert np.array_equal(only["logp_intent_sum"].view(np.uint32), got["logp_intent_sum"].view(np.uint32))


def test_twenty_agents_sum_through_the_python_layer():
    from ris_vec_marl_amd import BatchedPolicy
    from ris_vec_marl_amd import _native as N
    V, B = 20, 19
    heads, mask, taus, hard, eps, expo = make_inputs(V, B, 77, True, 1.0)
    assert native(heads, mask, taus, hard, eps, expo, rc_only=True) == N.ERR_ARG                    # a sum pointer, V > 16
    assert native(heads, mask, taus, hard, eps, expo, want=("logp_power_sum",), rc_only=True) == N.ERR_ARG
    per_agent = tuple(k for k in OUTS if not k.endswith("_sum"))
    want = R.batch(heads, mask, taus, hard, eps, expo)
    assert_outputs(native(heads, mask, taus, hard, eps, expo, want=per_agent), want, hard, "V=20 flat slots")
    pol = BatchedPolicy(V, 5, 64, 128, device=DEV, seed=3)
    with torch.no_grad():
        pol.Wh.mul_(30.0)
        pol.bh[:, 0, 2:4] -= 1.5
        pol.gumbel_hard.copy_(T(hard))
    obs = np.random.default_rng(5).uniform(0, 1.2, (B, V, 5)).astype(np.float32)
    h = pol.forward_heads(T(obs)).cpu().numpy()
    ret = pol.sample_normal(T(obs), T(mask), T(eps), T(expo))
    w = R.batch(h, mask, pol.tau.cpu().numpy(), hard, eps, expo)
    decided = (w["clear"] | (hard == 0)[None, :]).all(1)       # rows whose hard agents' arg-max is decided
    for got, ref in ((ret[5], w["logp_power"]), (ret[6], w["logp_intent"])):
        got, s64 = got.cpu().numpy().astype(np.float64), ref.sum(1)
        assert got.shape == (B,)
        bound = 1e-5 * np.abs(s64) + V * 2.0 ** -20
        margin("V=20 python sums", "sum", np.abs(got - s64)[decided], bound[decided])
        assert (np.abs(got - s64) <= bound)[decided].all()
    assert decided.mean() > 0.8
    assert pol.sample_normal(T(obs), T(mask), T(eps), T(expo), sums=False)[5:] == (None, None)


# ------------------------------------------------------------------------------------------- 4: same bits as choose_action
@pytest.mark.parametrize("V", [4, 5, 8, 16, 20])
def test_same_bits_as_the_choose_action_kernel(V):
    B = 2 * max(rows_per_block(V), 1) + 3
    heads, mask, taus, hard, eps, expo = make_inputs(V, B, 400 + V, True, 0.7)
    per_agent = tuple(k for k in OUTS if not k.endswith("_sum"))
    for draws in (dict(eps=eps, expo=expo), dict(seed=91, counter=5)):
        got = native(heads, mask, taus, hard, row_offset=3000 if "seed" in draws else 0, want=per_agent, **draws)
        power, probs, onehot = choose_native(heads, mask, taus, hard, env_offset=3000 if "seed" in draws else 0, **draws)
        na = got["next_actions"]
        assert np.array_equal(got["power"].view(np.uint32), power.view(np.uint32))
        assert np.array_equal(got["probs"].view(np.uint32), probs.view(np.uint32))
        assert np.array_equal(na[:, :, :V].view(np.uint32), onehot.view(np.uint32))
        assert np.array_equal(na[:, :, V:].view(np.uint32), got["power"].view(np.uint32))


# ------------------------------------------------------------------------------------------- 5: saturation and clamps
def test_saturation_clamp_and_single_open_entry():
    V, B = 4, 6
    heads = np.zeros((V, B, 4 + V), np.float32)
    heads[..., 4:] = np.random.default_rng(2).uniform(-3, 3, (V, B, V))
    eps = np.zeros((B, V, 2), np.float32)
    expo = np.maximum(np.random.default_rng(3).exponential(size=(B, V, V)), 1e-6).astype(np.float32)
    heads[:, 0, 0:2], heads[:, 1, 0:2] = 20.0, -20.0           # rows 0 / 1: x_t = +-20 (log_std 0, eps 0): tanh is +-1
    heads[:, 2, 2:4], heads[:, 3, 2:4] = 5.0, -30.0            # rows 2 / 3: log_std above 2 / below -20
    heads[:, 2:4, 0:2] = 0.1
    eps[2:4] = 0.01
    heads[:, 4:, 2:4] = -1.0
    mask = np.ones((B, V, V), np.uint8)
    mask[4:, :, :] = 0
    mask[4:, :, 1] = 1                                         # rows 4 / 5: V - 1 blocked entries
    hard = np.array([1, 1, 0, 1], np.uint8)
    for tau in (2.0, 0.3):
        got = native(heads, mask, np.full(V, tau, np.float32), hard, eps, expo)
        assert (got["power"][0] == 1.0).all() and (got["power"][1] == -1.0).all()
        # per component -log(2 pi) / 2 - logf(1e-6f): the correction within 1 ulp of 13.8 (2^-20), the difference and the
        # sum of the two rounded once each (2^-21 at 12.9 twice, 2^-20 at 25.8): 4 x 2^-20 in all
        want = 2.0 * (-R.HALF_LOG_2PI - np.log(np.float64(np.float32(1e-6))))
        err = np.abs(got["logp_power"][0:2].astype(np.float64) - want)
        print("[logp margin] saturated rows tau=%g: max err %.3g, bound %.3g" % (tau, err.max(), 2.0 ** -18))
        assert (err <= 2.0 ** -18).all()
        for row, ls in ((2, 2.0), (3, -20.0)):                 # the clamp: std = exp(ls), the Normal term carries -ls
            x_t = np.float64(np.float32(0.1)) + np.exp(ls) * np.float64(np.float32(0.01))
            p32 = np.float64(np.float32(np.tanh(x_t)))
            w = 2.0 * (-0.5 * np.float64(np.float32(0.01)) ** 2 - ls - R.HALF_LOG_2PI - np.log(1.0 - p32 * p32 + 1e-6))
            e = np.abs(got["logp_power"][row].astype(np.float64) - w)
            b = R.REL * abs(w) + R.ABS + 2 * 2.0 ** -22 / (1.0 - p32 * p32 + 1e-6)
            print("[logp margin] log_std clamped to %g: max err %.3g, bound %.3g" % (ls, e.max(), b))
            assert (e <= b).all()
            np.testing.assert_allclose(got["power"][row], np.tanh(x_t), atol=2e-5)
        assert (np.abs(got["logp_intent"][4:]) <= 2.0 ** -20).all()
        assert (got["probs"][4:, :, 1] == 1.0).all() and (got["next_actions"][4:, :, 1] == 1.0).all()
        want_all = R.batch(heads, mask, np.full(V, tau, np.float32), hard, eps, expo)
        assert_outputs(got, want_all, hard, "saturation rows tau=%g" % tau)
        assert_sums_bitwise(got, "saturation rows")


# ------------------------------------------------------------------------------------------- 6: Philox draws
@pytest.mark.parametrize("V,B", [(8, 37), (5, 20), (16, 9), (20, 11)])
def test_philox_draws_at_an_offset_and_counter(V, B):
    seed, counter, off = 77, 7, 4096 + 13
    heads, mask, taus, hard, _, _ = make_inputs(V, B, 600 + V, True, 0.8)
    eps, expo = PO.philox_draws(np.arange(off, off + B), V, counter, seed)
    want = R.batch(heads, mask, taus, hard, eps, expo)
    got = native(heads, mask, taus, hard, seed=seed, counter=counter, row_offset=off,
                 want=tuple(k for k in OUTS if V <= 16 or not k.endswith("_sum")))
    what = "philox V=%d B=%d" % (V, B)
    assert_outputs(got, want, hard, what)
    if V <= 16:
        assert_sums_bitwise(got, what)
    other = native(heads, mask, taus, hard, seed=seed, counter=counter + 1, row_offset=off, want=("power", "probs"))
    assert not np.array_equal(other["power"], got["power"]) and not np.array_equal(other["probs"], got["probs"])


# ------------------------------------------------------------------------------------------- 7: out= into td_target
def test_out_tensors_feed_td_target_in_place():
    from ris_vec_marl_amd import BatchedPolicy, BatchedTwinCritic
    V, B, dims = 8, 33, (40, 80, 96, 256, 256)
    pol = BatchedPolicy(V, 5, 64, 128, device=DEV, seed=5)
    hard = (np.arange(V) % 4 == 3).astype(np.uint8)
    with torch.no_grad():
        pol.Wh.mul_(30.0)
        pol.bh[:, 0, 2:4] -= 1.5
        pol.gumbel_hard.copy_(T(hard))
    sds = [CR.random_net(dims, 61), CR.random_net(dims, 62)]
    critic = BatchedTwinCritic(*dims, device=DEV, seed=1, gemm="fused")
    critic.load_state_dict(*sds)
    rng = np.random.default_rng(8)
    states_ = rng.uniform(0, 1.2, (B, V * 5)).astype(np.float32)
    mask = (rng.uniform(size=(B, V, V)) < 0.7).astype(np.uint8)
    eps = np.clip(rng.normal(size=(B, V, 2)), -3, 3).astype(np.float32)
    expo = np.maximum(rng.exponential(size=(B, V, V)), 1e-6).astype(np.float32)
    reward = rng.uniform(-6, 1, B).astype(np.float32)
    done = rng.uniform(size=B) < 0.25
    done[0], done[1] = True, False
    coef = np.array([0.15, 0.06], np.float32)
    t_states = T(states_)
    na, sp, si = guarded(B * V * (V + 2)), guarded(B), guarded(B)
    mine = (na[:B * V * (V + 2)].view(B, V * (V + 2)), sp[:B], si[:B])
    ret = pol.sample_normal(t_states.view(B, V, 5), T(mask), T(eps), T(expo), out=mine)
    assert ret[4] is mine[0] and ret[5] is mine[1] and ret[6] is mine[2]
    for buf, t in zip((na, sp, si), mine):
        assert bool((buf[t.numel():] == 12345.0).all()) and bool(torch.isfinite(t).all())
    y = critic.td_target(T(reward), t_states, mine[0], T(done), 0.99, mine[1], mine[2], T(coef))
    # float64: the log-prob sums of the restatement on the device's float32 heads, the critics on the same next_actions
    heads = pol.forward_heads(t_states.view(B, V, 5)).cpu().numpy()
    want = R.batch(heads, mask, pol.tau.cpu().numpy(), hard, eps, expo)
    got_na = mine[0].cpu().numpy().reshape(B, V, V + 2)
    assert np.array_equal(got_na[:, :, :V][want["clear"]], want["onehot"][want["clear"]])
    np.testing.assert_allclose(got_na[:, :, V:], want["power"], atol=2e-5)
    decided = (want["clear"] | (hard == 0)[None, :]).all(1)
    q64 = [CR.critic_q64(sd, states_, got_na.reshape(B, -1)) for sd in sds]
    y64 = CR.td_target64(reward, q64[0], q64[1], done, float(np.float32(0.99)), coef, want["logp_power"].sum(1), want["logp_intent"].sum(1))
    e_y = CR.err(y.cpu().numpy()[decided], y64[decided])
    print("[logp margin] sample_normal(out=) -> td_target: target vs float64 %.3g (bar %.3g), %d of %d rows decided"
          % (e_y, CR.BAR, decided.sum(), B))
    assert decided.sum() >= B - 3 and e_y < CR.BAR
    assert torch.equal(y[T(done)], T(reward)[T(done)])
    with pytest.raises(ValueError):
        pol.sample_normal(t_states.view(B, V, 5), T(mask), T(eps), T(expo), out=(mine[0], mine[1].double(), mine[2]))
    with pytest.raises(ValueError):
        pol.sample_normal(t_states.view(B, V, 5), T(mask), T(eps), T(expo), sums=False, out=mine)


# ------------------------------------------------------------------------------------------- 8: the example
def test_example_runs():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "marl_next_actions.py"), "64", "1"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("episode 0")]
    assert len(line) == 1 and "nan" not in line[0] and "inf" not in line[0], out.stdout
