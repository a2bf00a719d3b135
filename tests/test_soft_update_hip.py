"""GPU tests of the one-launch Polyak blend (`risvec_soft_update`, csrc/k_soft_update.hip; `soft_update_from`,
`ddpg_soft_update`).

The oracle is the reference's own statement, `tau * a.clone() + (1 - tau) * b.clone()` on CPU float32 tensors
(Simulation-SARL/ddpg_torch.py:122-127), compared BIT FOR BIT (int32 views): two rounded products and one rounded sum.
A kernel that contracts a product and the sum into a fused multiply-add differs from it in about a quarter of the
elements and fails here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import sarl_critic_ref as R  # noqa: E402

DEV = "cuda:0"
TAUS = [0.005, 0.3, 1.0, 0.0]
GUARD = 8                                          # floats in front of and behind every target
SENTINEL = -12345.0
NUMELS = [1, 3, 4, 5, 33 * 128, 1024 * 80]


def oracle(a, b, tau):
    """ddpg_torch.py:122-127 on CPU float32 tensors"""
    return tau * a.clone() + (1 - tau) * b.clone()


def same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def guarded(values, offset=0):
    """(buffer, view): `values` on the device with GUARD + offset sentinel floats in front and GUARD behind; the view
    starts `offset` floats behind a 16-byte boundary."""
    n = values.numel()
    buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + offset:GUARD + offset + n]
    view.copy_(values)
    return buf, view


def blend_and_check(cases, tau):
    """cases: [(numel, online offset, target offset)]; one launch over all of them, everything checked against the oracle."""
    from ris_vec_marl_amd.actor import soft_update_tensors
    g = torch.Generator().manual_seed(1000 + len(cases))
    on_cpu = [torch.randn(n, generator=g) for n, _, _ in cases]
    tg_cpu = [torch.randn(n, generator=g) * 3 for n, _, _ in cases]
    on = [guarded(v, o) for v, (_, o, _) in zip(on_cpu, cases)]
    tg = [guarded(v, o) for v, (_, _, o) in zip(tg_cpu, cases)]
    for (_, ov), (_, tv), (n, oo, to) in zip(on, tg, cases):
        assert ov.data_ptr() % 16 == 4 * oo and tv.data_ptr() % 16 == 4 * to
    versions = [tv._version for _, tv in tg]
    soft_update_tensors([(ov, tv) for (_, ov), (_, tv) in zip(on, tg)], tau, torch.device(DEV))
    torch.cuda.synchronize()
    for i, (n, oo, to) in enumerate(cases):
        want = oracle(on_cpu[i], tg_cpu[i], tau)
        got = tg[i][1].cpu()
        n_diff = int((got.view(torch.int32) != want.view(torch.int32)).sum())
        assert n_diff == 0, "tau %g, tensor %d (numel %d, offsets %d / %d): %d elements differ" % (tau, i, n, oo, to, n_diff)
        tb = tg[i][0].cpu()
        assert bool((tb[:GUARD + to] == SENTINEL).all()) and bool((tb[GUARD + to + n:] == SENTINEL).all())      # in place, nothing else
        ob = on[i][0].cpu()
        assert same_bits(ob[GUARD + oo:GUARD + oo + n], on_cpu[i])                                               # online unchanged
        assert bool((ob[:GUARD + oo] == SENTINEL).all()) and bool((ob[GUARD + oo + n:] == SENTINEL).all())
    assert [tv._version for _, tv in tg] == versions                    # as the docstrings say: not advanced


@pytest.mark.parametrize("tau", TAUS)
def test_a_list_of_tensors_against_the_oracle(tau):
    """Every numel of the issue, aligned; then both views one float off a 16-byte boundary (still 16 bytes at a time),
    only the target off (float by float), only the online off; sizes with heads and tails of every length."""
    cases = [(n, 0, 0) for n in NUMELS]
    cases += [(33 * 128, 1, 1), (1024 * 80, 1, 1), (5, 1, 1), (2, 3, 3)]
    cases += [(33 * 128, 0, 1), (1024 * 80 + 3, 0, 1), (5, 0, 1), (1, 0, 3)]
    cases += [(4097, 2, 0), (7, 2, 2), (4 * 1024 * 4 + 6, 3, 3)]
    blend_and_check(cases, tau)


def test_tau_one_is_a_copy_and_tau_zero_keeps_the_target():
    from ris_vec_marl_amd.actor import soft_update_tensors
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(1000, generator=g).to(DEV), torch.randn(1000, generator=g).to(DEV)
    b0 = b.clone()
    soft_update_tensors([(a, b)], 0.0, torch.device(DEV))
    assert same_bits(b, b0)
    soft_update_tensors([(a, b)], 1.0, torch.device(DEV))
    assert same_bits(b, a)


def test_32_tensors_at_once_and_the_contracted_form_would_fail():
    from ris_vec_marl_amd import _native as N
    blend_and_check([(1 + 37 * i, i % 4, i % 4 if i % 3 else (i + 1) % 4) for i in range(32)], 0.005)
    assert N.last_kernel() == "k_soft_update"
    # 33 are more than a launch takes: the entry point refuses them, and `soft_update_tensors` blends them in runs of 32 and 1
    import ctypes as C
    ts = [torch.zeros(4, device=DEV) for _ in range(66)]
    on, tg = (C.c_void_p * 33)(*(t.data_ptr() for t in ts[:33])), (C.c_void_p * 33)(*(t.data_ptr() for t in ts[33:]))
    assert N.load().risvec_soft_update(33, on, tg, (C.c_int64 * 33)(*([4] * 33)), 0.5, 0.5, N.stream(torch.device(DEV))) == N.ERR_SHAPE
    with pytest.raises(ValueError):
        N.check(N.ERR_SHAPE)
    blend_and_check([(1 + 37 * i, i % 4, i % 4 if i % 3 else (i + 1) % 4) for i in range(33)], 0.005)
    # the oracle tells the two forms apart: a fused multiply-add (computed in float64, rounded once) gives other bits
    g = torch.Generator().manual_seed(9)
    a, b = torch.randn(1 << 16, generator=g), torch.randn(1 << 16, generator=g)
    tau32, omt32 = float(np.float32(0.005)), float(np.float32(1 - 0.005))
    fused = (tau32 * a.double() + (omt32 * b).double()).float()         # fma(tau, a, fl32(omt * b))
    n_diff = int((fused.view(torch.int32) != oracle(a, b, 0.005).view(torch.int32)).sum())
    print("a contracted blend differs from the oracle in %d of %d elements" % (n_diff, a.numel()))
    assert n_diff > a.numel() // 100


# ---------------------------------------------------------------------------------------------- end to end
CRITIC = (80, 1024, 512, 256, 56)
ACTOR = (80, 512, 256, 56)
ROWS = 129


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def networks(seed, pack="device"):
    """(actor, critic) at the driver's shape with random weights (LayerNorm parameters included), pack="device"."""
    from ris_vec_marl_amd import BatchedActor, BatchedCritic
    IN, F1, F2, F3, A = CRITIC
    critic = BatchedCritic(IN, A, F1, F2, F3, device=DEV, seed=seed, gemm="fused", pack=pack)
    critic.load_state_dict(R.random_critic(CRITIC, seed))
    actor = BatchedActor(ACTOR[0], ACTOR[3], ACTOR[1], ACTOR[2], device=DEV, seed=seed, gemm="fused", pack=pack)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    actor.Wmu.mul_(60.0)
    for w, b in ((actor.ln1_w, actor.ln1_b), (actor.ln2_w, actor.ln2_b)):
        w.copy_(0.5 + torch.rand(w.shape, generator=g))
        b.copy_((torch.rand(b.shape, generator=g) * 2 - 1) * 0.2)
    return actor, critic


def sampled(seed=3):
    s_, _ = R.random_batch(CRITIC, ROWS, seed)
    rng = np.random.default_rng(seed)
    return T(s_), T(rng.uniform(-6, 1, ROWS).astype(np.float32)), T(rng.uniform(size=ROWS) < 0.3)


def blended(online, target, tau):
    """{key: oracle blend} of two networks' state_dicts (CPU float32)"""
    so, st = online.state_dict(), target.state_dict()
    return {k: oracle(so[k], st[k], tau) for k in st}


@pytest.mark.parametrize("tau", [0.005, 1.0])
def test_end_to_end(tau):
    from ris_vec_marl_amd import ddpg_soft_update, ddpg_td_target
    from ris_vec_marl_amd import _native as N
    actor, critic = networks(11)
    t_actor, t_critic = networks(12)
    states_, rewards, dones = sampled()
    y0 = ddpg_td_target(t_actor, t_critic, states_, rewards, dones, 0.99).clone()
    g = torch.Generator(device="cpu").manual_seed(13)
    for net in (actor, critic):                               # stands in for the optimiser step: every tensor, in place
        for a in net._WEIGHTS:
            t = getattr(net, a)
            t.add_((torch.randn(t.shape, generator=g) * 1e-2 * float(t.abs().max())).to(DEV))
    want_a, want_c = blended(actor, t_actor, tau), blended(critic, t_critic, tau)
    online_before = [{k: v.clone() for k, v in net.state_dict().items()} for net in (actor, critic)]
    stream_a, stream_c = t_actor._fused_weights()[0].data_ptr(), t_critic._fused_weights()[0].data_ptr()
    packs = t_critic.packs
    ddpg_soft_update(actor, t_actor, critic, t_critic, tau)
    assert N.last_kernel() == "k_soft_update"
    got_a, got_c = t_actor.state_dict(), t_critic.state_dict()
    assert len(got_a) + len(got_c) == 26
    for got, want in ((got_a, want_a), (got_c, want_c)):
        for k in want:
            assert same_bits(got[k], want[k]), k
    for net, before in zip((actor, critic), online_before):   # the online networks are only read
        assert all(same_bits(v, before[k]) for k, v in net.state_dict().items())
    if tau == 1.0:
        assert all(same_bits(got_a[k], v) for k, v in actor.state_dict().items())
        assert all(same_bits(got_c[k], v) for k, v in critic.state_dict().items())
    y1 = ddpg_td_target(t_actor, t_critic, states_, rewards, dones, 0.99).clone()
    assert t_critic.packs == packs + 1
    assert t_actor._fused_weights()[0].data_ptr() == stream_a and t_critic._fused_weights()[0].data_ptr() == stream_c
    f_actor, f_critic = networks(14)
    f_actor.load_state_dict(want_a)
    f_critic.load_state_dict(want_c)
    y2 = ddpg_td_target(f_actor, f_critic, states_, rewards, dones, 0.99)
    assert same_bits(y1, y2)
    assert not torch.equal(y1, y0)
    assert torch.equal(y1[dones], rewards[dones])


def test_stale_marking_and_mappings():
    """No version counter moves, yet the next td_target rebuilds the stream once; a second call does not.  The online
    network given as a mapping of the learner's tensors under the reference's names."""
    actor, critic = networks(21)
    t_actor, t_critic = networks(22)
    states_, rewards, dones = sampled(4)
    actions_ = t_actor.forward(states_).clone()
    t_critic.td_target(rewards, states_, actions_, dones, 0.99)
    packs = t_critic.packs
    versions = [getattr(t_critic, a)._version for a in t_critic._WEIGHTS]
    want = blended(critic, t_critic, 0.3)
    online = {k: getattr(critic, a) for k, a in critic._SD.items()}
    t_critic.soft_update_from(online, 0.3)
    assert [getattr(t_critic, a)._version for a in t_critic._WEIGHTS] == versions
    assert all(same_bits(v, want[k]) for k, v in t_critic.state_dict().items())
    y1 = t_critic.td_target(rewards, states_, actions_, dones, 0.99).clone()
    assert t_critic.packs == packs + 1
    y2 = t_critic.td_target(rewards, states_, actions_, dones, 0.99)
    assert t_critic.packs == packs + 1 and torch.equal(y1, y2)
    # the actor's method; then a host-packed target critic: the same marking
    want = blended(actor, t_actor, 0.005)
    t_actor.soft_update_from(actor, 0.005)
    assert all(same_bits(v, want[k]) for k, v in t_actor.state_dict().items())
    f_actor, _ = networks(23)
    f_actor.load_state_dict(want)
    assert torch.equal(t_actor.forward(states_), f_actor.forward(states_))
    h_critic = networks(24, pack="host")[1]
    h_critic.td_target(rewards, states_, actions_, dones, 0.99)
    packs = h_critic.packs
    h_critic.soft_update_from(critic, 0.005)
    h_critic.td_target(rewards, states_, actions_, dones, 0.99)
    assert h_critic.packs == packs + 1
    with pytest.raises(ValueError):
        t_critic.soft_update_from(t_critic, 0.5)              # the target's own tensors
    with pytest.raises(ValueError):
        t_critic.soft_update_from(critic, 1.5)


def test_example_runs():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "sarl_soft_update.py"), "256", "1"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "mean target" in out.stdout
    assert "k_soft_update -> 2 x k_sarl_actor_pack -> 2 x k_sarl_critic_pack -> k_sarl_actor<8,6> -> k_sarl_critic<4,2>" in out.stdout
