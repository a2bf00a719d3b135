"""CPU-side checks of the sweep of tests/test_mlp_sweep_hip.py, at the very shapes, seeds and row counts it uses
(tests/mlp_sweep_shapes.py):
  * the table is what it says: each shape is inside the library's `*_supported()` domain, its geometry selects the
    instantiation the table names, every instantiation of the three kernels is reached, and the run-time parameters of
    the edges a case is there for (KS, NG, groups per wavefront, LDS bytes, items) have the stated values;
  * the inputs leave headroom under the project's bars: a plain torch float32 forward -- what the library mode computes,
    up to the order of its sums -- is within BAR / 8 of the float64 restatement, so a kernel that meets
    fused_bar(library err) = 8 x library err is inside BAR as well, and the two bars never pull against each other;
  * where fc1 <= 160 the packed stream, walked through the kernel's index rules in NumPy, is within half of
    fused_bar(float32 err): the split-fp16 arithmetic itself fits the fused bar with a factor 2 to spare for the MFMA's
    float32 accumulation.
Every figure is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest
import torch

from ris_vec_marl_amd import _native as N
from ris_vec_marl_amd import actor as ACT
from ris_vec_marl_amd import critic as CR
from ris_vec_marl_amd import marl_critic as MC
from tests import marl_critic_ref as MR
from tests import mlp_sweep_shapes as SW
from tests import sarl_critic_ref as R
from tests.test_sarl_actor_hip import err as actor_err
from tests.test_sarl_actor_hip import forward64 as actor_logits64
from tests.test_sarl_actor_hip import obs_like, sigmoid64

F = torch.nn.functional
HEADROOM = R.BAR / 8.0                        # fused_bar(e) = 8 e <= BAR for every library err e below this


def t32(w, k):
    return torch.from_numpy(np.asarray(w[k], np.float32))


def lin(x, w, name):
    return F.linear(x, t32(w, name + ".weight"), t32(w, name + ".bias"))


def ln(x, w, name):
    return F.layer_norm(x, (x.shape[-1],), t32(w, name + ".weight"), t32(w, name + ".bias"), 1e-5)


def marl_q32(w, state, action):
    """`BatchedTwinCritic.q_torch` of one net on the CPU"""
    x = torch.cat([torch.from_numpy(state), torch.from_numpy(action)], 1)
    for name in ("fc1", "fc2", "fc3"):
        x = torch.relu(lin(x, w, name))
    return lin(x, w, "q").numpy().reshape(-1)


def critic_q32(w, state, action):
    """`BatchedCritic.q_torch` on the CPU"""
    s = torch.relu(ln(lin(torch.from_numpy(state), w, "fc1"), w, "bn1"))
    s = ln(lin(s, w, "fc2"), w, "bn2")
    h = torch.relu(s + lin(torch.from_numpy(action), w, "action_value"))
    h = torch.relu(ln(lin(h, w, "fc3"), w, "bn3"))
    return lin(h, w, "q").numpy().reshape(-1)


def actor_logits32(w, x):
    """`BatchedActor.logits_torch` on the CPU"""
    h = torch.relu(ln(lin(torch.from_numpy(x).reshape(len(x), -1), w, "fc1"), w, "bn1"))
    h = torch.relu(ln(lin(h, w, "fc2"), w, "bn2"))
    return lin(h, w, "mu").numpy()


# --------------------------------------------------------------------------------------------------------- the table
def test_marl_table_names_the_instantiation_and_the_edges():
    lib = N.load()
    seen = set()
    for case in SW.MARL_CRITIC:
        assert lib.risvec_marl_critic_supported(*case.dims) == 1 and MC._supported(*case.dims), case
        g = MC.marl_critic_geom(*case.dims)
        assert case.kernel == "k_marl_critic<%d,%d>" % (g.mt2, g.mt3), case
        assert lib.risvec_marl_critic_stream_bytes(*case.dims) == g.rows * 1024
        seen.add((g.mt2, g.mt3))
    # with <4,2> (test_marl_critic_hip.py: DRIVER) all six are run
    assert seen == {(1, 1), (4, 1), (1, 2), (2, 1), (2, 2)}
    assert seen | {(4, 2)} == {(a, b) for a in (1, 2, 4) for b in (1, 2)} and (4, 2) not in seen
    geom = [MC.marl_critic_geom(*c.dims) for c in SW.MARL_CRITIC]
    assert [(g.ks, g.ng) for g in geom] == [(1, 1), (1, 1), (2, 2), (8, 5), (8, 32), (5, 31), (4, 3)]
    assert [c.dims[0] + c.dims[1] for c in SW.MARL_CRITIC] == [2, 16, 17, 128, 128, 79, 64]
    lds = [(g.ks + max(2 * g.ng, 8 * g.mt2)) * 2048 + 2 * 4 * 32 * 4 for g in geom]
    assert lds[4] == 148480 and lds[5] > 64 * 1024 and all(v <= 160 * 1024 for v in lds)
    assert 2 * geom[1].ng < 8 * geom[1].mt2 and 2 * geom[4].ng > 8 * geom[4].mt2      # what sizes s_h
    assert sorted(SW.MARL_CRITIC_RUNS) == sorted([(i, 2) for i in range(7)] + [(0, 1), (4, 1)])
    # what the backward adds at the same shapes (tests/test_marl_critic_grad_sweep_hip.py): s_h = max(2 NG, K3 + K4) k-steps, the LDS
    # of the row launch, XF = S + A rounded up to 32 and the live columns of the last column tile of d fc1.weight
    from tests.test_marl_critic_grad_sweep_hip import BACKWARD_EDGE
    assert list(BACKWARD_EDGE) == [c.dims for c in SW.MARL_CRITIC]
    glds = [(g.ks + max(2 * g.ng, 8 * g.mt2 + 8 * g.mt3)) * 2048 + 2 * 4 * 32 * 4 for g in geom]
    assert glds[4] == 148480 and all(v <= 160 * 1024 for v in glds)
    assert [2 * g.ng > 8 * g.mt2 + 8 * g.mt3 for g in geom] == [False, False, False, False, True, True, False]
    xf = [(c.dims[0] + c.dims[1] + 31) // 32 * 32 for c in SW.MARL_CRITIC]
    assert xf == [32, 32, 32, 128, 128, 96, 64]
    assert [c.dims[0] + c.dims[1] - (x - 32) for c, x in zip(SW.MARL_CRITIC, xf)] == [2, 16, 17, 32, 32, 15, 32]
    assert {(g.mt2, g.mt3) for g in geom} | {(4, 2)} == {(a, b) for a in (1, 2, 4) for b in (1, 2)}   # <4,2>: test_marl_critic_grad_hip.py


def test_sarl_critic_table_names_the_instantiation_and_the_edges():
    lib = N.load()
    seen = set()
    for case in SW.SARL_CRITIC:
        assert lib.risvec_sarl_critic_supported(*case.dims) == 1 and CR._supported(*case.dims), case
        g = CR.critic_geom(*case.dims)
        assert case.kernel == "k_sarl_critic<%d,%d>" % (g.mt2, g.mt3), case
        assert lib.risvec_sarl_critic_stream_bytes(*case.dims) == g.rows * 1024
        seen.add((g.mt2, g.mt3))
    # with <4,2> (test_sarl_critic_hip.py: DRIVER) all six are run
    assert seen == {(1, 1), (1, 2), (2, 1), (2, 2), (4, 1)}
    geom = [CR.critic_geom(*c.dims) for c in SW.SARL_CRITIC]
    assert [(g.ks, g.ksa, g.ng) for g in geom] == [(1, 1, 1), (2, 1, 2), (9, 6, 5), (3, 2, 3), (8, 3, 32), (1, 6, 31)]
    assert {c.dims[0] for c in SW.SARL_CRITIC} >= {15, 16, 128} and {c.dims[4] for c in SW.SARL_CRITIC} >= {1, 16, 17, 96}
    lds = [(g.ks + max(g.ksa, 2 * g.ng, 8 * g.mt2)) * 2048 + 6 * 4 * 32 * 4 for g in geom]
    assert lds[4] > 64 * 1024 and lds[5] > 64 * 1024 and all(v <= 160 * 1024 for v in lds)


def test_actor_table_names_the_instantiation_and_the_edges():
    lib = N.load()
    seen = set()
    for case in SW.SARL_ACTOR:
        IN, F1, F2, A = case.dims
        assert lib.risvec_sarl_actor_supported(*case.dims) == 1 and ACT._supported(*case.dims), case
        g = ACT.actor_geom(*case.dims)
        assert case.kernel == "k_sarl_actor<%d,%d>" % (g.mt, g.ks), case
        assert case.obs[0] * (case.obs[1] + 5) == IN
        seen.add((g.mt, g.ks))
    # with <8,6> (test_sarl_actor_hip.py: DRIVER 8_40) all eight are run
    assert seen | {(8, 6)} == {(m, k) for m in (4, 8) for k in ACT._KS_BUILT} and (8, 6) not in seen
    geom = [ACT.actor_geom(*c.dims) for c in SW.SARL_ACTOR]
    true_ks = [-(-(c.dims[0] + 1) // 16) for c in SW.SARL_ACTOR]
    assert [(k, g.ks) for k, g in zip(true_ks, geom)] == [(1, 3), (3, 3), (4, 6), (7, 7), (7, 7), (8, 9), (9, 9)]
    assert [(g.ng, g.p1, g.t1) for g in geom] == [(1, 4, 1), (3, 6, 1), (5, 2, 3), (2, 2, 1), (31, 3, 11), (32, 2, 16), (32, 2, 16)]
    assert [g.ht for g in geom] == [1, 2, 1, 3, 3, 3, 3] and geom[0].items == 3
    assert 3 * geom[6].rows * 1024 == 156 * 1024
    assert {c.dims[3] for c in SW.SARL_ACTOR} >= {1, 32, 33, 65, 96}


# ------------------------------------------------------------------------------------------------------ the headroom
@pytest.mark.parametrize("index", range(len(SW.MARL_CRITIC)), ids=[SW.case_id(c) for c in SW.MARL_CRITIC])
def test_marl_inputs_leave_headroom(index):
    case = SW.MARL_CRITIC[index]
    dims, n = case.dims, SW.CRITIC_ROWS
    w_seed, b_seed = SW.seeds("marl", index)
    state, action = MR.random_batch(dims, n, b_seed)
    assert not state[0].any() and not action[0].any()
    for c in (0, 1):
        w = MR.random_net(dims, w_seed + c)
        ref = MR.critic_q64(w, state, action)
        e32 = MR.err(marl_q32(w, state, action), ref)
        print("marl %s net %d: float32 err %.3g, max |q64| %.3g" % (SW.case_id(case), c + 1, e32, np.abs(ref).max()))
        assert np.abs(ref).max() > 0.05
        assert e32 <= HEADROOM
        if dims[2] <= 160:
            stream, scales = MC.pack_marl_critic_weights(*(t32(w, k + ".weight") for k in ("fc1", "fc2", "fc3")))
            walk = MR.walk_stream(stream.numpy(), scales.numpy(), w, state, action, dims, MC.marl_critic_geom(*dims))
            e_w = MR.err(walk, ref)
            print("marl %s net %d: walk err %.3g (half the fused bar: %.3g)" % (SW.case_id(case), c + 1, e_w, MR.fused_bar(e32) / 2))
            assert e_w <= MR.fused_bar(e32) / 2


@pytest.mark.parametrize("index", range(len(SW.SARL_CRITIC)), ids=[SW.case_id(c) for c in SW.SARL_CRITIC])
def test_sarl_critic_inputs_leave_headroom(index):
    case = SW.SARL_CRITIC[index]
    dims, n = case.dims, SW.CRITIC_ROWS
    w_seed, b_seed = SW.seeds("critic", index)
    w = R.random_critic(dims, w_seed)
    state, action = R.random_batch(dims, n, b_seed)
    assert not state[0].any() and not action[0].any()
    ref = R.critic_q64(w, state, action)
    e32 = R.err(critic_q32(w, state, action), ref)
    print("critic %s: float32 err %.3g, max |q64| %.3g" % (SW.case_id(case), e32, np.abs(ref).max()))
    assert np.abs(ref).max() > 0.05
    assert e32 <= HEADROOM
    if dims[1] <= 160:
        stream, scales = CR.pack_critic_weights(t32(w, "fc1.weight"), t32(w, "fc1.bias"), t32(w, "fc2.weight"),
                                                t32(w, "action_value.weight"), t32(w, "fc3.weight"))
        walk = R.walk_stream(stream.numpy(), scales.numpy(), w, state, action, dims, CR.critic_geom(*dims))
        e_w = R.err(walk, ref)
        print("critic %s: walk err %.3g (half the fused bar: %.3g)" % (SW.case_id(case), e_w, R.fused_bar(e32) / 2))
        assert e_w <= R.fused_bar(e32) / 2


@pytest.mark.parametrize("index", range(len(SW.SARL_ACTOR)), ids=[SW.case_id(c) for c in SW.SARL_ACTOR])
def test_actor_inputs_leave_headroom(index):
    case = SW.SARL_ACTOR[index]
    dims, n = case.dims, SW.ACTOR_ROWS
    w_seed, b_seed = SW.seeds("actor", index)
    w = SW.actor_weights(dims, w_seed)
    assert set(w) == set(ACT.BatchedActor._SD)
    o = obs_like(np.random.default_rng(b_seed), n, *case.obs)
    o[0] = 0.0
    ref = actor_logits64(w, o)
    assert ref.shape == (n, dims[3])
    e32 = actor_err(actor_logits32(w, o), ref)
    mu64 = sigmoid64(ref)
    print("actor %s: float32 err %.3g, mu64 spans [%.3g, %.3g]" % (SW.case_id(case), e32, mu64.min(), mu64.max()))
    assert np.abs(mu64 - 0.5).max() > 0.1                       # the widened head: the sigmoid is not stuck at 1/2
    assert e32 <= HEADROOM
