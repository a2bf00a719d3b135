"""GPU tests of the DDPG critic forward and TD target (`BatchedCritic`, `ddpg_td_target`, `risvec_sarl_critic`,
csrc/k_sarl_critic.hip): the reference's `CriticNetwork.forward` (Simulation-SARL/networks.py:66-79) and the target of
`learn()` (ddpg_torch.py:80-88) in one MFMA launch, against vectors captured from the reference's own network and
against a float64 restatement (tests/sarl_critic_ref.py).

Error measure: err = max over rows |q - q64| / max(max over the batch |q64|, 1e-3) -- batch-wide, because a single q can
cancel to near zero.  Bars (the project's, from test_sarl_actor_hip.py):
  * err < 2e-5 in every mode;
  * fused: err <= max(8 x the library mode's err on the same inputs, 1e-7).
The epilogue: |y - (r + gamma q_own)| <= 2^-23 (|r| + |gamma q_own|) against the q the same launch wrote (one product
and one sum rounding), rows with `done` equal the reward bit for bit.
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import sarl_critic_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DRIVER = {"8_40": (80, 1024, 512, 256, 56), "8_64": (104, 1024, 512, 256, 80)}
FIXTURES = ["sarl_critic_8_40", "sarl_critic_4_16"]


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def make_critic(dims, sd=None, gemm=None, seed=0):
    from ris_vec_marl_amd import BatchedCritic
    IN, F1, F2, F3, A = dims
    c = BatchedCritic(IN, A, F1, F2, F3, device=DEV, seed=seed, gemm=gemm)
    if sd is not None:
        c.load_state_dict(sd)
    return c


def run(critic, x, a, mode):
    """q [n] of `critic` in `mode` on device tensors, as numpy."""
    was, critic.gemm = critic.gemm, mode
    try:
        out = torch.full((x.shape[0], 1), float("nan"), device=DEV)
        q = critic.forward(x, a, out=out)
        assert q.data_ptr() == out.data_ptr()
    finally:
        critic.gemm = was
    return q.cpu().numpy().reshape(-1)


def check_bars(critic, x, a, what, ref64=None):
    """Both modes against the float64 restatement on the same inputs, both bars of the module docstring."""
    if ref64 is None:
        sd = {k: v.numpy() for k, v in critic.state_dict().items()}
        ref64 = R.critic_q64(sd, x.cpu().numpy(), a.cpu().numpy())
    q_f, q_l = run(critic, x, a, "fused"), run(critic, x, a, "library")
    e_f, e_l = R.err(q_f, ref64), R.err(q_l, ref64)
    print("%s: q err fused %.3g library %.3g (ratio %.2f), max |q64| %.3g" % (what, e_f, e_l, e_f / max(e_l, 1e-30), np.abs(ref64).max()))
    assert np.isfinite(q_f).all()
    assert e_l < R.BAR and e_f < R.BAR
    assert e_f <= R.fused_bar(e_l)
    return q_f, ref64


def check_epilogue(y, q_own, reward, done, gamma, what):
    """y against float64 r + gamma q_own (gamma as the float32 the kernel receives)"""
    y, q_own, reward = (np.asarray(v, np.float64).reshape(-1) for v in (y, q_own, reward))
    gq = float(np.float32(gamma)) * q_own
    live = ~np.asarray(done, bool)
    excess = np.abs(y - (reward + gq)) - 2.0 ** -23 * (np.abs(reward) + np.abs(gq))
    print("%s: epilogue, worst |y - (r + gamma q_own)| - bound = %.3g over %d live rows"
          % (what, excess[live].max() if live.any() else float("nan"), live.sum()))
    assert (excess[live] <= 0).all()
    assert np.array_equal(y[~live], reward[~live])


@functools.lru_cache(maxsize=None)
def driver_critic(tag):
    """The driver's sizes with weights in the reference's init ranges, q widened to +-0.4, LayerNorm weights in
    [0.5, 1.5] and biases in +-0.2.  Shared and never modified: tests that update weights build their own."""
    return make_critic(DRIVER[tag], R.random_critic(DRIVER[tag], 41), gemm="fused")


def fresh_critic(tag="8_40", seed=5):
    return make_critic(DRIVER[tag], driver_critic(tag).state_dict(), gemm="fused", seed=seed)


def batch(dims, n, seed, zero_row0=True):
    s, a = R.random_batch(dims, n, seed, zero_row0)
    return T(s), T(a)


@pytest.mark.parametrize("mode", ["fused", "library"])
@pytest.mark.parametrize("name", FIXTURES)
def test_vs_golden(name, mode):
    from ris_vec_marl_amd import BatchedActor, ddpg_td_target
    fx = R.fixture(name)
    V, M, B = int(fx["V"]), int(fx["M"]), int(fx["B"])
    dims = (V * (M // V + 5), int(fx["fc1"]), int(fx["fc2"]), int(fx["fc3"]), 2 * V + M)
    sd, asd = R.weights_of(fx), R.weights_of(fx, "aw.")
    critic = make_critic(dims, sd, gemm=mode)
    assert critic.gemm == mode
    x, a = T(fx["state"]), T(fx["action"])                    # state [B, V, tn + 5]: read in place
    q64 = R.critic_q64(sd, fx["state"], fx["action"])
    q = critic.forward(x, a).cpu().numpy()
    assert q.shape == (B, 1)
    e_gold, e_64 = R.err(q, fx["q"]), R.err(q, q64)
    print("%s %s: q vs the reference's float32 %.3g, vs float64 %.3g" % (name, mode, e_gold, e_64))
    assert e_gold < R.BAR and e_64 < R.BAR
    # td_target on the reference's own target action, then the two-launch helper with the reference's target actor
    gamma, done, reward = float(fx["gamma"]), T(fx["done"]), T(fx["reward"])
    q_own = torch.empty(B, 1, device=DEV)
    y = critic.td_target(reward, T(fx["state_"]), T(fx["target_action"]), done, gamma, q=q_own)
    y64 = R.td_target64(fx["reward"], R.critic_q64(sd, fx["state_"], fx["target_action"]), fx["done"], gamma)
    e_y, e_y64 = R.err(y.cpu().numpy(), fx["target"]), R.err(y.cpu().numpy(), y64)
    e_qn = R.err(q_own.cpu().numpy(), fx["q_next"])
    print("%s %s: target vs the reference's %.3g, vs float64 %.3g; Q(s', a') vs the reference's %.3g" % (name, mode, e_y, e_y64, e_qn))
    assert tuple(y.shape) == (B,) and e_y < R.BAR and e_y64 < R.BAR and e_qn < R.BAR
    assert torch.equal(y[done], reward[done])                 # bit for bit
    check_epilogue(y.cpu().numpy(), q_own.cpu().numpy(), fx["reward"], fx["done"], gamma, name + " " + mode)
    actor = BatchedActor(dims[0], dims[4], int(fx["afc1"]), int(fx["afc2"]), device=DEV, gemm=mode)
    actor.load_state_dict(asd)
    y2 = ddpg_td_target(actor, critic, T(fx["state_"]), reward, done, gamma)
    e_y2 = R.err(y2.cpu().numpy(), fx["target"])
    print("%s %s: ddpg_td_target vs the reference's target %.3g" % (name, mode, e_y2))
    assert e_y2 < R.BAR and torch.equal(y2[done], reward[done])
    if mode == "fused":
        check_bars(critic, x, a, name, q64)


@pytest.mark.parametrize("tag", sorted(DRIVER))
def test_driver_sizes_vs_float64(tag):
    critic = driver_critic(tag)
    x, a = batch(DRIVER[tag], 257, 7)
    q, _ = check_bars(critic, x, a, "driver " + tag)
    assert np.abs(q).max() > 0.3


@pytest.mark.parametrize("n", [1, 33, 65, 129, 257])
def test_row_counts_zero_row_and_untouched_tail(n):
    """Partly filled tiles and more than one workgroup; row 0 all zero in state and action; rows of out / q / y beyond n
    keep their sentinel."""
    critic = driver_critic("8_40")
    x, a = batch(DRIVER["8_40"], n, 100 + n)
    assert not x[0].any() and not a[0].any()
    q, _ = check_bars(critic, x, a, "n = %d" % n)
    rng = np.random.default_rng(n)
    reward, done = T(rng.uniform(-6, 1, n).astype(np.float32)), T(rng.uniform(size=n) < 0.3)
    big, big_q, big_y = (torch.full(s, -7.0, device=DEV) for s in ((n + 40, 1), (n + 40, 1), (n + 40,)))
    assert critic.forward(x, a, out=big[:n]).data_ptr() == big.data_ptr()
    assert critic.td_target(reward, x, a, done, 0.99, out=big_y[:n], q=big_q[:n]).data_ptr() == big_y.data_ptr()
    assert np.array_equal(big[:n, 0].cpu().numpy(), q) and torch.equal(big_q[:n], big[:n])
    assert bool((big[n:] == -7.0).all()) and bool((big_q[n:] == -7.0).all()) and bool((big_y[n:] == -7.0).all())
    check_epilogue(big_y[:n].cpu().numpy(), q, reward.cpu().numpy(), done.cpu().numpy(), 0.99, "n = %d" % n)


def test_rows_are_independent_and_calls_repeat():
    critic = driver_critic("8_40")
    x, a = batch(DRIVER["8_40"], 300, 11)
    whole, parts = torch.empty(300, 1, device=DEV), torch.empty(300, 1, device=DEV)
    critic.forward(x, a, out=whole)
    critic.forward(x[:172], a[:172], out=parts[:172])
    critic.forward(x[172:], a[172:], out=parts[172:])
    assert torch.equal(whole, parts)
    assert torch.equal(whole, critic.forward(x, a))


def test_action_branch_on_its_own():
    dims = DRIVER["8_40"]
    x, a = batch(dims, 130, 13)
    only_a = fresh_critic()
    only_a.ln2_w.zero_()
    only_a.ln2_b.zero_()                                      # LN2(fc2 s) = 0: q depends on the action only
    q, _ = check_bars(only_a, x, a, "bn2 = 0")
    x2, _ = batch(dims, 130, 14)
    assert np.array_equal(run(only_a, x2, a, "fused"), q)
    no_a = fresh_critic()
    no_a.Wav.zero_()                                          # independent of the action, bit for bit
    _, a2 = batch(dims, 130, 15)
    assert not torch.equal(a, a2)
    assert np.array_equal(run(no_a, x, a, "fused"), run(no_a, x, a2, "fused"))
    critic = driver_critic("8_40")
    a3 = a.clone()
    a3[77, 31] += 0.25                                        # one element of one row
    q0, q1 = run(critic, x, a, "fused"), run(critic, x, a3, "fused")
    changed = np.flatnonzero(q0 != q1)
    assert changed.tolist() == [77]
    check_bars(critic, x, a3, "one action element changed")


@pytest.mark.parametrize("layer", ["fc1", "fc3"])
def test_degenerate_layernorms(layer):
    """The layer a thousand times smaller than its init range: the pre-activation's variance is far below the LayerNorm
    eps, so what is normalised is mostly eps; LayerNorm weight 3."""
    critic = fresh_critic()
    if layer == "fc1":
        critic.W1.mul_(1e-3); critic.b1.mul_(1e-3); critic.ln1_w.fill_(3.0)
    else:
        critic.W3.mul_(1e-3); critic.b3.mul_(1e-3); critic.ln3_w.fill_(3.0)
    x, a = batch(DRIVER["8_40"], 257, 9)
    q, _ = check_bars(critic, x, a, "nearly constant " + layer)
    assert np.isfinite(q).all()


def test_epilogue_outputs_agree():
    """q-only, y-only and both-outputs calls agree bit for bit on what they share; y against the q of the same launch."""
    critic = driver_critic("8_64")
    n = 200
    x, a = batch(DRIVER["8_64"], n, 17)
    rng = np.random.default_rng(18)
    r_np, d_np = rng.uniform(-6, 1, n).astype(np.float32), rng.uniform(size=n) < 0.4
    reward, done = T(r_np), T(d_np)
    q_only = critic.forward(x, a)
    y_only = critic.td_target(reward, x, a, done, 0.97)
    q_both = torch.empty(n, 1, device=DEV)
    y_both = critic.td_target(reward, x, a, done, 0.97, q=q_both)
    assert torch.equal(q_only, q_both) and torch.equal(y_only, y_both)
    assert torch.equal(critic.td_target(reward, x, a, done.to(torch.uint8), 0.97), y_both)     # uint8 0 / 1 as bool
    check_epilogue(y_both.cpu().numpy(), q_both.cpu().numpy(), r_np, d_np, 0.97, "driver 8_64")
    assert d_np.sum() >= 5 and (~d_np).sum() >= 5


def test_two_launch_helper_and_sampled_batch():
    """`ddpg_td_target` = actor.forward + critic.td_target bit for bit; then on the tensors `sample_buffer` returns after a
    3-step rollout at E = 64, (V, M) = (8, 40), read in place."""
    from ris_vec_marl_amd import BatchedActor, OUNoise, SarlReplayBuffer, VecEnviron, ddpg_td_target, reference_lanes
    from ris_vec_marl_amd import _native as N
    E, V, M = 64, 8, 40
    A, tn = 2 * V + M, M // V
    critic = driver_critic("8_40")
    actor = BatchedActor(V * (tn + 5), A, 512, 256, device=DEV, seed=3)
    actor.Wmu.mul_(60.0)
    L = reference_lanes()
    env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3, n_envs=E,
                     device=DEV, seed=21)
    env.make_new_game()
    env.compute_parms()
    mu = torch.zeros(E, A, device=DEV)
    memory = SarlReplayBuffer(4 * E, tn + 5, A, V, device=DEV)
    rollout = env.bind_sarl_rollout(mu, noise=OUNoise(E, A, device=DEV, seed=3), replay=memory)
    obs = env.sarl_observation()
    for k in range(3):
        actor.forward(obs, out=mu)
        rollout(done=k == 2)
    states, actions, rewards, states_, dones = memory.sample_buffer(96)
    assert dones.dtype == torch.bool and bool(dones.any()) and not bool(dones.all())
    keep = [t.clone() for t in (states_, rewards, dones)]
    act_buf, y = torch.empty(96, A, device=DEV), torch.empty(96, device=DEV)
    got = ddpg_td_target(actor, critic, states_, rewards, dones, 0.99, out=y, actions_=act_buf)
    assert got.data_ptr() == y.data_ptr() and N.last_kernel().startswith("k_sarl_critic<4,2>")
    assert all(torch.equal(t, k) for t, k in zip((states_, rewards, dones), keep))      # read in place, not written
    mu_t = actor.forward(states_)
    assert torch.equal(act_buf, mu_t)
    q_own = torch.empty(96, 1, device=DEV)
    assert torch.equal(critic.td_target(rewards, states_, mu_t, dones, 0.99, q=q_own), y)
    assert torch.equal(ddpg_td_target(actor, critic, states_, rewards, dones, 0.99), y)
    assert torch.equal(y[dones], rewards[dones])
    sd = {k: v.numpy() for k, v in critic.state_dict().items()}
    e = R.err(q_own.cpu().numpy(), R.critic_q64(sd, states_.cpu().numpy(), mu_t.cpu().numpy()))
    print("sampled batch: Q(s', a') err %.3g" % e)
    assert e < R.BAR
    # the critic's own forward on the stored (state, action) pairs: actions in +-1 after the exploration noise
    check_bars(critic, states, actions, "sampled (state, action)")


def test_weight_updates_are_picked_up():
    critic = fresh_critic()
    x, a = batch(DRIVER["8_40"], 130, 19)
    before = critic.forward(x, a).clone()
    packed, packs = critic._fused_weights(), critic.packs
    critic.forward(x, a)
    assert critic._fused_weights() is packed and critic.packs == packs      # nothing changed: nothing repacked
    critic.ln2_b.add_(0.1)                                    # read in place by the kernel: no repack needed
    mid = critic.forward(x, a).clone()
    assert critic.packs == packs and not torch.equal(before, mid)
    critic.W3.mul_(1.25)
    critic.Wav.mul_(0.5)
    after = critic.forward(x, a).clone()
    assert critic._fused_weights() is not packed and critic.packs == packs + 1
    assert not torch.equal(mid, after)
    check_bars(critic, x, a, "after the in-place update")
    twin = fresh_critic(seed=99)
    twin.load_state_dict(critic.state_dict())
    assert torch.equal(twin.forward(x, a), after)
    # the learner's own tensors, by reference: an in-place step on them is seen
    learner = {k: v.to(DEV) for k, v in critic.state_dict().items()}
    shared = fresh_critic(seed=98)
    shared.share_state_dict(learner)
    assert shared.W2.data_ptr() == learner["fc2.weight"].data_ptr()
    assert torch.equal(shared.forward(x, a), after)
    learner["fc2.weight"].mul_(0.9)
    learner["q.bias"].add_(0.5)
    moved = shared.forward(x, a)
    assert not torch.equal(moved, after)
    twin.load_state_dict({k: v.cpu() for k, v in learner.items()})
    assert torch.equal(twin.forward(x, a), moved)
    with pytest.raises(ValueError):
        shared.share_state_dict({k: v.double() for k, v in learner.items()})


def test_dispatch_and_argument_checks():
    from ris_vec_marl_amd import BatchedCritic
    from ris_vec_marl_amd import _native as N
    with pytest.raises(ValueError):
        BatchedCritic(80, 56, 1024, 384, 256, device=DEV, gemm="fused")
    with pytest.raises(ValueError):
        BatchedCritic(80, 56, device=DEV, gemm="fp32")
    odd = BatchedCritic(80, 56, 1024, 384, 256, device=DEV, seed=2)
    assert odd.gemm == "library"                              # an unsupported fc2 chooses the library path
    x, a = batch(DRIVER["8_40"], 40, 23)
    sd = {k: v.numpy() for k, v in odd.state_dict().items()}
    q = odd.forward(x, a)
    assert tuple(q.shape) == (40, 1)
    odd_err = R.err(q.cpu().numpy(), R.critic_q64(sd, x.cpu().numpy(), a.cpu().numpy()))
    print("fc2 = 384 (library): err %.3g" % odd_err)
    assert odd_err < R.BAR
    critic = driver_critic("8_40")
    assert BatchedCritic(80, 56, device=DEV).gemm == "fused"
    critic.forward(x, a)
    assert N.last_kernel().startswith("k_sarl_critic<4,2>")
    small = make_critic((36, 64, 128, 128, 24), gemm="fused")
    xs, as_ = batch((36, 64, 128, 128, 24), 40, 24)
    q_small = small.forward(xs, as_)
    assert N.last_kernel().startswith("k_sarl_critic<1,1>")
    small_sd = {k: v.numpy() for k, v in small.state_dict().items()}
    small_err = R.err(q_small.cpu().numpy(), R.critic_q64(small_sd, xs.cpu().numpy(), as_.cpu().numpy()))
    print("(36, 64, 128, 128, 24) fused <1,1>: err %.3g" % small_err)
    assert small_err < R.BAR
    reward, done = torch.zeros(40, device=DEV), torch.zeros(40, dtype=torch.bool, device=DEV)
    x3 = x.reshape(40, 8, 10)
    assert torch.equal(critic.forward(x3, a), critic.forward(x, a))      # [n, V, input_dims / V] in place
    for bad in (x.double(), x.cpu(), x[:, :72], x.t(), x.reshape(40, 4, 20)[:, ::2], None):
        with pytest.raises(ValueError):
            critic.forward(bad, a)
        with pytest.raises(ValueError):
            critic.td_target(reward, bad, a, done)
    for bad in (a.double(), a.cpu(), a[:, :48], a[:39], torch.empty(40, 112, device=DEV)[:, ::2], None):
        with pytest.raises(ValueError):
            critic.forward(x, bad)
        with pytest.raises(ValueError):
            critic.td_target(reward, x, bad, done)
    for bad_out in (torch.empty(41, 1, device=DEV), torch.empty(40, 1, device=DEV, dtype=torch.float64), torch.empty(40, 1),
                    torch.empty(40, 2, device=DEV)[:, ::2], torch.empty(40, device=DEV)):
        with pytest.raises(ValueError):
            critic.forward(x, a, out=bad_out)
        with pytest.raises(ValueError):
            critic.td_target(reward, x, a, done, q=bad_out)
    for bad_y in (torch.empty(41, device=DEV), torch.empty(40, device=DEV, dtype=torch.float64), torch.empty(40),
                  torch.empty(80, device=DEV)[::2], torch.empty(40, 1, device=DEV)):
        with pytest.raises(ValueError):
            critic.td_target(reward, x, a, done, out=bad_y)
        with pytest.raises(ValueError):
            critic.td_target(bad_y, x, a, done)
    for bad_done in (done.float(), done.cpu(), done[:39], torch.zeros(80, dtype=torch.bool, device=DEV)[::2], None):
        with pytest.raises(ValueError):
            critic.td_target(reward, x, a, bad_done)
    with pytest.raises(ValueError):
        critic.td_target(reward, x, a, done, gamma=float("inf"))


def test_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sarl_td_target.py"), "256", "1"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "mean target" in out.stdout
