"""GPU tests of the DDPG actor forward (`BatchedActor`, `risvec_sarl_actor`, csrc/k_sarl_actor.hip): the reference's
`ActorNetwork.forward` (Simulation-SARL/networks.py:132-141) in one MFMA launch, against vectors captured from the
reference's own network and against a float64 restatement.

Error measure (as in test_policy_hip.py): err = max over ALL samples of |logits - logits64| / max(rowmax |logits64|, 1e-3).
Bars:
  * err < 2e-5 for every mode: the project's bar for a hand-written forward against the library one;
  * fused: err <= max(8 x the library mode's err on the same inputs, 1e-7): the split product carries 2^-22 per
    product against float32's 2^-24 (the margin of test_split_fp16_gemm_has_float32_accuracy);
  * mu against the float64 sigmoid of the kernel's OWN float32 logits: at most 4 x what torch.sigmoid on the device
    makes of the same logits, with a floor of 2^-23.
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle.policy_oracle import layer_norm  # noqa: E402  (checker)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
BAR = 2e-5
DRIVER = {"8_40": (80, 512, 256, 56), "8_64": (104, 512, 256, 80)}


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def forward64(sd, x):
    """networks.py:132-141 in float64 (pre-sigmoid values); sd: the reference's state_dict names -> arrays."""
    W = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    h = np.asarray(x, np.float64).reshape(len(x), -1) @ W["fc1.weight"].T + W["fc1.bias"]
    h = np.maximum(layer_norm(h, W["bn1.weight"], W["bn1.bias"]), 0.0)
    h = h @ W["fc2.weight"].T + W["fc2.bias"]
    h = np.maximum(layer_norm(h, W["bn2.weight"], W["bn2.bias"]), 0.0)
    return h @ W["mu.weight"].T + W["mu.bias"]


def sigmoid64(z):
    z = np.asarray(z, np.float64)
    return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


def err(logits, ref64):
    scale = np.maximum(np.abs(ref64).max(-1, keepdims=True), 1e-3)
    return float((np.abs(np.asarray(logits, np.float64) - ref64) / scale).max())


def run(actor, x, mode):
    """(logits, mu) of `actor` in `mode` on the device tensor x, as numpy."""
    was, actor.gemm = actor.gemm, mode
    try:
        lg = torch.full((x.shape[0], actor.n_actions), float("nan"), device=DEV)
        mu = actor.forward(x, logits=lg)
    finally:
        actor.gemm = was
    return lg.cpu().numpy(), mu.cpu().numpy()


def check_bars(actor, x, what, ref64=None):
    """Both modes against the float64 restatement on the same inputs, every bar of the module docstring."""
    sd = {k: v.numpy() for k, v in actor.state_dict().items()}
    ref64 = forward64(sd, x.cpu().numpy()) if ref64 is None else ref64
    lg_f, mu_f = run(actor, x, "fused")
    lg_l, mu_l = run(actor, x, "library")
    e_f, e_l = err(lg_f, ref64), err(lg_l, ref64)
    own = sigmoid64(lg_f)
    d_mu = float(np.abs(mu_f - own).max())
    d_torch = float(np.abs(torch.sigmoid(T(lg_f)).cpu().numpy() - own).max())
    print("%s: logits err fused %.3g library %.3g (ratio %.2f); mu vs own-logit sigmoid %.3g, torch.sigmoid %.3g"
          % (what, e_f, e_l, e_f / max(e_l, 1e-30), d_mu, d_torch))
    assert np.isfinite(lg_f).all() and np.isfinite(mu_f).all()
    assert e_l < BAR and e_f < BAR
    assert e_f <= max(8 * e_l, 1e-7)
    assert d_mu <= max(4 * d_torch, 2.0 ** -23)
    return lg_f, mu_f, ref64


def obs_like(rng, n, V, tn):
    """Observation-shaped inputs (ddpg_train.py:134-149): phase slice in [0, 2 pi), five scalars in [0, 1.2], one zero."""
    o = np.empty((n, V, tn + 5), np.float32)
    o[:, :, :tn] = rng.uniform(0, 2 * np.pi, (n, V, tn))
    o[:, :, tn:] = rng.uniform(0, 1.2, (n, V, 5))
    o[:, :, tn + 3] = 0.0
    return o


@functools.lru_cache(maxsize=None)
def driver_actor(tag):
    """The driver's sizes with weights in the reference's init ranges, the head widened 60 x so that the outputs span
    (0, 1), LayerNorm weights in [0.5, 1.5] and biases in +-0.2.  Shared and never modified: tests that update weights
    build their own."""
    from ris_vec_marl_amd import BatchedActor
    IN, F1, F2, A = DRIVER[tag]
    a = BatchedActor(IN, A, F1, F2, device=DEV, seed=31)
    g = torch.Generator(device="cpu").manual_seed(32)
    a.Wmu.mul_(60.0)
    for w, b in ((a.ln1_w, a.ln1_b), (a.ln2_w, a.ln2_b)):
        w.copy_(0.5 + torch.rand(w.shape, generator=g))
        b.copy_((torch.rand(b.shape, generator=g) * 2 - 1) * 0.2)
    return a


def fresh_actor(tag="8_40", seed=31):
    from ris_vec_marl_amd import BatchedActor
    IN, F1, F2, A = DRIVER[tag]
    a = BatchedActor(IN, A, F1, F2, device=DEV, seed=seed)
    a.load_state_dict(driver_actor(tag).state_dict())
    return a


@pytest.mark.parametrize("mode", ["fused", "library"])
@pytest.mark.parametrize("name", ["sarl_actor_8_40.npz", "sarl_actor_4_16.npz"])
def test_vs_golden(name, mode):
    from ris_vec_marl_amd import BatchedActor
    d = np.load(os.path.join(GOLD, name))
    V, M = int(d["V"]), int(d["M"])
    sd = {k[2:]: d[k] for k in d.files if k.startswith("w.")}
    actor = BatchedActor(V * (M // V + 5), 2 * V + M, int(d["fc1"]), int(d["fc2"]), device=DEV, gemm=mode)
    assert actor.gemm == mode
    actor.load_state_dict(sd)
    x = T(d["obs"])                                           # [B, V, tn + 5]: read in place as [B, V (tn + 5)]
    ref64 = forward64(sd, d["obs"])
    e_ref = err(d["logits"], ref64)
    lg = torch.empty(x.shape[0], actor.n_actions, device=DEV)
    mu = actor.forward(x, logits=lg)
    e_gold, e_64 = err(lg.cpu().numpy(), d["logits"].astype(np.float64)), err(lg.cpu().numpy(), ref64)
    print("%s %s: vs the reference's float32 logits %.3g, vs float64 %.3g (the reference itself: %.3g)" % (name, mode, e_gold, e_64, e_ref))
    assert e_ref < BAR                                        # the restatement is the reference's network
    assert e_gold < BAR and e_64 < BAR
    # |sigmoid'| <= 1/4: the logits bar carried through the sigmoid, plus one float32 rounding of mu
    np.testing.assert_allclose(mu.cpu().numpy(), d["mu"], atol=0.25 * BAR * float(np.abs(ref64).max()) + 2.0 ** -23)
    assert float(mu.min()) < 0.1 and float(mu.max()) > 0.9   # the fixture spans (0, 1)
    if mode == "fused":
        check_bars(actor, x, name, ref64)


@pytest.mark.parametrize("tag", sorted(DRIVER))
def test_driver_sizes_vs_float64(tag):
    actor = driver_actor(tag)
    IN, F1, F2, A = DRIVER[tag]
    assert actor.gemm == "fused"
    x = T(obs_like(np.random.default_rng(7), 1024, 8, IN // 8 - 5))
    _, mu, _ = check_bars(actor, x, "driver " + tag)
    assert mu.min() < 0.1 and mu.max() > 0.9


@pytest.mark.parametrize("n", [1, 33, 65, 257])
def test_row_counts_zero_row_and_untouched_tail(n):
    """Partly empty wavefronts and workgroups; an all-zero row (row 0: the observation of a fresh env has zero phases,
    here everything is zero); rows of `out` beyond n keep their sentinel."""
    actor = driver_actor("8_40")
    o = obs_like(np.random.default_rng(n), n, 8, 5)
    o[0] = 0.0
    x = T(o)
    lg, mu, _ = check_bars(actor, x, "n = %d" % n)
    big = torch.full((n + 40, actor.n_actions), -7.0, device=DEV)
    big_l = torch.full((n + 40, actor.n_actions), -7.0, device=DEV)
    got = actor.forward(x, out=big[:n], logits=big_l[:n])
    assert got.data_ptr() == big.data_ptr()
    assert np.array_equal(big[:n].cpu().numpy(), mu) and np.array_equal(big_l[:n].cpu().numpy(), lg)
    assert bool((big[n:] == -7.0).all()) and bool((big_l[n:] == -7.0).all())


def test_nearly_constant_fc1():
    """fc1 a thousand times smaller than its init range: the pre-activation's variance (1e-7) is far below the
    LayerNorm eps, so what is normalised is mostly eps; LayerNorm weight 3."""
    actor = fresh_actor()
    actor.W1.mul_(1e-3)
    actor.b1.mul_(1e-3)
    actor.ln1_w.fill_(3.0)
    x = T(obs_like(np.random.default_rng(9), 257, 8, 5))
    lg, mu, _ = check_bars(actor, x, "nearly constant fc1")
    assert np.isfinite(lg).all() and np.isfinite(mu).all()


def test_rows_are_independent_and_calls_repeat():
    actor = driver_actor("8_40")
    x = T(obs_like(np.random.default_rng(11), 300, 8, 5))
    whole, whole_l = torch.empty(300, 56, device=DEV), torch.empty(300, 56, device=DEV)
    parts, parts_l = torch.empty(300, 56, device=DEV), torch.empty(300, 56, device=DEV)
    actor.forward(x, out=whole, logits=whole_l)
    actor.forward(x[:170], out=parts[:170], logits=parts_l[:170])
    actor.forward(x[170:], out=parts[170:], logits=parts_l[170:])
    assert torch.equal(whole, parts) and torch.equal(whole_l, parts_l)
    again = actor.forward(x)
    assert torch.equal(whole, again)


def test_weight_updates_are_picked_up():
    actor = fresh_actor()
    x = T(obs_like(np.random.default_rng(13), 130, 8, 5))
    before = actor.forward(x).clone()
    packed = actor._fused_weights()
    assert actor._fused_weights() is packed                   # nothing changed: nothing rebuilt
    actor.W2.mul_(1.25)
    actor.ln1_b.add_(0.1)
    after = actor.forward(x).clone()
    assert actor._fused_weights() is not packed
    assert not torch.equal(before, after)
    check_bars(actor, x, "after the in-place update")
    twin = fresh_actor(seed=99)
    twin.load_state_dict(actor.state_dict())
    assert torch.equal(twin.forward(x), after)
    for k, v in actor.state_dict().items():
        assert torch.equal(v, twin.state_dict()[k])


def test_dispatch_and_argument_checks():
    from ris_vec_marl_amd import BatchedActor
    from ris_vec_marl_amd import _native as N
    with pytest.raises(ValueError):
        BatchedActor(80, 56, 512, 64, device=DEV, gemm="fused")
    with pytest.raises(ValueError):
        BatchedActor(80, 56, 512, 256, device=DEV, gemm="fp32")
    small = BatchedActor(80, 56, 512, 64, device=DEV)
    assert small.gemm == "library"
    x = T(obs_like(np.random.default_rng(15), 40, 8, 5))
    sd = {k: v.numpy() for k, v in small.state_dict().items()}
    lg = torch.empty(40, 56, device=DEV)
    mu = small.forward(x, logits=lg)
    assert err(lg.cpu().numpy(), forward64(sd, x.cpu().numpy())) < BAR and tuple(mu.shape) == (40, 56)
    actor = driver_actor("8_40")
    actor.forward(x)
    assert N.last_kernel().startswith("k_sarl_actor<8,6>")
    assert driver_actor("8_64").gemm == "fused"
    driver_actor("8_64").forward(T(obs_like(np.random.default_rng(15), 40, 8, 8)))
    assert N.last_kernel().startswith("k_sarl_actor<8,7>")
    for bad in (x.double(), x.cpu(), x[:, :, :9], x.transpose(0, 1), x.reshape(40, 4, 20)[:, ::2]):
        with pytest.raises(ValueError):
            actor.forward(bad)
    for bad_out in (torch.empty(41, 56, device=DEV), torch.empty(40, 56, device=DEV, dtype=torch.float64),
                    torch.empty(40, 56), torch.empty(40, 112, device=DEV)[:, ::2]):
        with pytest.raises(ValueError):
            actor.forward(x, out=bad_out)
        with pytest.raises(ValueError):
            actor.forward(x, logits=bad_out)


def test_in_the_rollout_loop():
    """actor -> rollout launch for three steps at E = 64, (V, M) = (8, 40): the actor reads `launch.obs` and writes the
    bound `mu` in place.  A second env whose `mu` is filled by copying must end up with the same action, phase,
    observation and replay rows bit for bit -- from step 2 on the actor's input is the observation the launch wrote."""
    from ris_vec_marl_amd import OUNoise, SarlReplayBuffer, VecEnviron, reference_lanes
    E, V, M = 64, 8, 40
    A, tn = 2 * V + M, M // V
    actor = driver_actor("8_40")
    rng = np.random.default_rng(17)
    L = reference_lanes()
    side = []
    for _ in range(2):
        env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3, n_envs=E,
                         device=DEV, seed=21)
        env.make_new_game()
        env.compute_parms()
        mu = torch.zeros(E, A, device=DEV)
        z = torch.zeros(E, A, device=DEV)
        arr = torch.zeros(E, V, dtype=torch.int32, device=DEV)
        noise = OUNoise(E, A, device=DEV, seed=3)
        ring = SarlReplayBuffer(4 * E, tn + 5, A, V, device=DEV)
        side.append(dict(env=env, mu=mu, z=z, arr=arr, ring=ring,
                         launch=env.bind_sarl_rollout(mu, noise=noise, replay=ring, z=z, arrivals=arr)))
    a, b = side
    seen = []
    for k in range(3):
        zk, ak = T(rng.standard_normal((E, A)).astype(np.float32)), T(rng.poisson(1.0, (E, V)).astype(np.int32))
        for s in side:
            s["z"].copy_(zk)
            s["arr"].copy_(ak)
        x_in = a["launch"].obs.clone()
        got = actor.forward(a["launch"].obs, out=a["mu"])
        assert got.data_ptr() == a["mu"].data_ptr()
        assert torch.equal(a["mu"], actor.forward(x_in.view(E, -1)))          # [E, V, tn + 5] in place == the flat view
        b["mu"].copy_(a["mu"])
        a["launch"](done=k == 2)
        b["launch"](done=k == 2)
        for name in ("action", "phase", "obs"):
            assert torch.equal(getattr(a["launch"], name), getattr(b["launch"], name)), (k, name)
        assert not torch.equal(a["launch"].obs, x_in)
        seen.append(a["mu"].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    for name in a["ring"]._ARRAYS:
        assert torch.equal(getattr(a["ring"], name), getattr(b["ring"], name)), name
    assert a["ring"].mem_cntr == b["ring"].mem_cntr == 3 * E


def test_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sarl_rollout.py"), "256", "1"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "env-steps/s" in out.stdout
