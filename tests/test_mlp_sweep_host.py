"""CPU-side checks of the sweep of tests/test_mlp_sweep_hip.py, at the very shapes, seeds and row counts it uses
(tests/mlp_sweep_shapes.py):
  * the table is what it says: each shape is inside the library's `*_supported()` domain, its geometry selects the
    instantiation the table names, every instantiation of the five kernels (`k_marl_critic`, `k_sarl_critic`,
    `k_sarl_actor`, `k_marl_critic_wide`, `k_local_critics`) is reached, and the run-time parameters of the edges a case
    is there for (KS, the chunk list, NG, groups per wavefront, LDS bytes, items) have the stated values;
  * the inputs leave headroom under the project's bars: a plain torch float32 forward -- what the library mode computes,
    up to the order of its sums -- is within BAR / 8 of the float64 restatement, so a kernel that meets
    fused_bar(library err) = 8 x library err is inside BAR as well, and the two bars never pull against each other;
  * where fc1 <= 160 the packed stream, walked through the kernel's index rules in NumPy, is within half of
    fused_bar(float32 err): the split-fp16 arithmetic itself fits the fused bar with a factor 2 to spare for the MFMA's
    float32 accumulation.  The wide kernel's stream is walked in its chunks (`walk_stream_wide` of
    test_marl_critic_wide_host.py, whose chunk list must be the table's), a local critic's per agent on that agent's
    columns.
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
from tests.test_marl_critic_wide_host import CHUNK, walk_stream_wide
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


def wave_groups(ng):
    """fc1 groups per wavefront: wavefront w owns groups w, w + 4, .."""
    return [len(range(w, ng, 4)) for w in range(4)]


def chunks_of(ks):
    return [min(CHUNK, ks - c) for c in range(0, ks, CHUNK)]


def test_wide_table_names_the_instantiation_and_the_edges():
    lib = N.load()
    seen = []
    for case in SW.MARL_CRITIC_WIDE:
        assert lib.risvec_marl_critic_wide_supported(*case.dims) == 1 and MC._supported_wide(*case.dims), case
        g = MC.marl_critic_geom(*case.dims)
        assert case.kernel == "k_marl_critic_wide<%d,%d>" % (g.mt2, g.mt3), case
        assert lib.risvec_marl_critic_wide_stream_bytes(*case.dims) == g.rows * 1024
        seen.append((g.mt2, g.mt3))
    assert seen == [(1, 2), (2, 1), (4, 1), (1, 1), (2, 2), (1, 2), (4, 2), (4, 1)]
    assert set(seen) == {(a, b) for a in (1, 2, 4) for b in (1, 2)}                    # all six, none left to another file
    # only the first shape is the fused kernel's too
    assert [lib.risvec_marl_critic_supported(*c.dims) for c in SW.MARL_CRITIC_WIDE] == [1, 0, 0, 0, 0, 0, 0, 0]
    geom = [MC.marl_critic_geom(*c.dims) for c in SW.MARL_CRITIC_WIDE]
    assert [c.dims[0] + c.dims[1] for c in SW.MARL_CRITIC_WIDE] == [2, 129, 192, 208, 256, 512, 512, 173]
    assert [g.ks for g in geom] == [1, 9, 12, 13, 16, 32, 32, 11]
    assert [chunks_of(g.ks) for g in geom] == [[1], [8, 1], [8, 4], [8, 5], [8, 8], [8, 8, 8, 8], [8, 8, 8, 8], [8, 3]]
    # the last chunk against kAhead = 4: below it (1, 3), on it (4, 8), one past it (5); fewer than kAhead k-steps in all
    assert {ch[-1] for ch in map(chunks_of, (g.ks for g in geom))} == {1, 3, 4, 5, 8} and geom[0].ks < 4
    assert [g.ng for g in geom] == [1, 5, 31, 2, 3, 32, 1, 4]
    assert [wave_groups(g.ng) for g in geom] == [[1, 0, 0, 0], [2, 1, 1, 1], [8, 8, 8, 7], [1, 1, 0, 0], [1, 1, 1, 0], [8, 8, 8, 8],
                                                 [1, 0, 0, 0], [1, 1, 1, 1]]
    # live columns of the last k-step; the k-step and the chunk that hold the state / action boundary
    assert [c.dims[0] + c.dims[1] - 16 * (g.ks - 1) for c, g in zip(SW.MARL_CRITIC_WIDE, geom)] == [2, 1, 16, 16, 16, 16, 16, 13]
    assert [(c.dims[0] // 16, c.dims[0] // 128, c.dims[0] % 128) for c in SW.MARL_CRITIC_WIDE] == [
        (0, 0, 1), (7, 0, 127), (8, 1, 0), (0, 0, 3), (15, 1, 122), (0, 0, 1), (31, 3, 127), (5, 0, 90)]
    lds = [(CHUNK + max(2 * g.ng, 8 * g.mt2)) * 2048 + 2 * 4 * 32 * 4 for g in geom]
    assert lds == [33792, 50176, 144384, 33792, 50176, 148480, 82944, 82944]
    assert lds[5] == 148480 and lds[2] > 64 * 1024 and lds[6] > 64 * 1024 and all(v <= 160 * 1024 for v in lds)
    assert 2 * geom[6].ng < 8 * geom[6].mt2 and 2 * geom[5].ng > 8 * geom[5].mt2      # what sizes s_h
    assert sorted(SW.MARL_CRITIC_WIDE_RUNS) == sorted([(i, 2) for i in range(8)] + [(0, 1), (5, 1)])


def test_local_table_names_the_instantiation_and_the_edges():
    lib = N.load()
    seen = []
    for case in SW.LOCAL_CRITICS:
        V, net = case.dims[0], case.dims[1:]
        assert lib.risvec_local_critics_supported(*case.dims) == 1 and 1 <= V <= 16 and MC._supported(*net), case
        g = MC.marl_critic_geom(*net)
        assert case.kernel == "k_local_critics<%d,%d>x%d" % (g.mt2, g.mt3, V), case
        assert lib.risvec_marl_critic_stream_bytes(*net) == g.rows * 1024             # an agent's stream is the global kernel's
        seen.append((g.mt2, g.mt3))
    assert seen == [(1, 2), (2, 1), (2, 2), (4, 1), (1, 1), (1, 2)]
    # with <4,2> (test_local_critics_hip.py: test_same_arithmetic_at_the_drivers_sizes) all six are run
    assert set(seen) | {(4, 2)} == {(a, b) for a in (1, 2, 4) for b in (1, 2)} and (4, 2) not in seen
    assert lib.risvec_local_critics_supported(17, *SW.LOCAL_CRITICS[1].dims[1:]) == 0  # 16 is the limit
    geom = [MC.marl_critic_geom(*c.dims[1:]) for c in SW.LOCAL_CRITICS]
    assert [c.dims[0] for c in SW.LOCAL_CRITICS] == [1, 16, 3, 2, 16, 9]
    assert [c.dims[1] + c.dims[2] for c in SW.LOCAL_CRITICS] == [2, 23, 17, 128, 128, 16]
    assert [(g.ks, g.ng) for g in geom] == [(1, 1), (2, 5), (2, 3), (8, 31), (8, 2), (1, 32)]
    assert [wave_groups(g.ng) for g in geom] == [[1, 0, 0, 0], [2, 1, 1, 1], [1, 1, 1, 0], [8, 8, 8, 7], [1, 1, 0, 0], [8, 8, 8, 8]]
    # the from-policy form needs A = V + 2: two cases; in the second the one-hot k = 5 .. 20 meets the 8-value fragments
    # 0, 1 and 2 and crosses the k-step edge at 16
    assert [c.dims[2] == c.dims[0] + 2 for c in SW.LOCAL_CRITICS] == [False, True, False, False, False, True]
    V, S = SW.LOCAL_CRITICS[1].dims[:2]
    assert {k // 8 for k in range(S, S + V)} == {0, 1, 2} and S < 16 < S + V
    assert SW.LOCAL_CRITICS[2].dims[1] == 16 and SW.LOCAL_CRITICS[4].dims[1] == 127
    lds = [(g.ks + max(2 * g.ng, 8 * g.mt2)) * 2048 + 2 * 4 * 32 * 4 for g in geom]
    assert lds == [19456, 37888, 37888, 144384, 33792, 134144]
    assert lds[3] > 64 * 1024 and lds[5] > 64 * 1024 and all(v <= 160 * 1024 for v in lds)
    assert sorted(SW.LOCAL_CRITICS_RUNS) == sorted([(i, 2) for i in range(6)] + [(0, 1), (3, 1)])


def test_new_seeds_are_the_stated_ones_and_apart_from_the_old():
    assert [SW.seeds("wide", i) for i in (0, 7)] == [(1700, 1705), (1770, 1775)]
    assert [SW.seeds("local", i) for i in (0, 5)] == [(1900, 1905), (2400, 2405)]
    assert [SW.seeds(k, 0) for k in ("marl", "critic", "actor")] == [(1100, 1105), (1300, 1305), (1508, 1505)]


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


@pytest.mark.parametrize("index", range(len(SW.MARL_CRITIC_WIDE)), ids=[SW.case_id(c) for c in SW.MARL_CRITIC_WIDE])
def test_wide_inputs_leave_headroom(index):
    case = SW.MARL_CRITIC_WIDE[index]
    dims, n = case.dims, SW.CRITIC_ROWS
    w_seed, b_seed = SW.seeds("wide", index)
    state, action = MR.random_batch(dims, n, b_seed)
    assert state.shape == (n, dims[0]) and action.shape == (n, dims[1]) and not state[0].any() and not action[0].any()
    g = MC.marl_critic_geom(*dims)
    for c in (0, 1):
        w = MR.random_net(dims, w_seed + c)
        ref = MR.critic_q64(w, state, action)
        e32 = MR.err(marl_q32(w, state, action), ref)
        print("wide %s net %d: float32 err %.3g, max |q64| %.3g" % (SW.case_id(case), c + 1, e32, np.abs(ref).max()))
        assert np.abs(ref).max() > 0.05
        assert e32 <= HEADROOM
        if dims[2] <= 160:
            stream, scales = MC.pack_marl_critic_weights(*(t32(w, k + ".weight") for k in ("fc1", "fc2", "fc3")), wide=True)
            walk, chunks = walk_stream_wide(stream.numpy(), scales.numpy(), w, state, action, dims, g)
            assert chunks == chunks_of(g.ks)
            e_w = MR.err(walk, ref)
            print("wide %s net %d: chunks %s, walk err %.3g (half the fused bar: %.3g)"
                  % (SW.case_id(case), c + 1, chunks, e_w, MR.fused_bar(e32) / 2))
            assert e_w <= MR.fused_bar(e32) / 2


@pytest.mark.parametrize("index", range(len(SW.LOCAL_CRITICS)), ids=[SW.case_id(c) for c in SW.LOCAL_CRITICS])
def test_local_inputs_leave_headroom(index):
    case = SW.LOCAL_CRITICS[index]
    dims, n = case.dims, SW.CRITIC_ROWS
    V, net = dims[0], dims[1:]
    w_seed, b_seed = SW.seeds("local", index)
    obs, act = SW.local_batch(dims, n, b_seed)
    assert obs.shape == (n, V, dims[1]) and act.shape == (n, V, dims[2]) and not obs[0].any() and not act[0].any()
    sds = SW.local_nets(dims, w_seed)
    assert len(sds) == V and all(len(pair) == 2 for pair in sds)
    g = MC.marl_critic_geom(*net)
    worst32, worst_w, least_q = 0.0, 0.0, np.inf
    for j in range(V):
        s_j, a_j = np.ascontiguousarray(obs[:, j]), np.ascontiguousarray(act[:, j])
        for c, w in enumerate(sds[j]):
            ref = MR.critic_q64(w, s_j, a_j)
            e32 = MR.err(marl_q32(w, s_j, a_j), ref)
            worst32, least_q = max(worst32, e32), min(least_q, np.abs(ref).max())
            assert np.abs(ref).max() > 0.05, (j, c)
            assert e32 <= HEADROOM, (j, c, e32)
            if net[2] <= 160:
                stream, scales = MC.pack_marl_critic_weights(*(t32(w, k + ".weight") for k in ("fc1", "fc2", "fc3")))
                e_w = MR.err(MR.walk_stream(stream.numpy(), scales.numpy(), w, s_j, a_j, net, g), ref)
                worst_w = max(worst_w, e_w / MR.fused_bar(e32))
                assert e_w <= MR.fused_bar(e32) / 2, (j, c, e_w, e32)
    print("local %s: over %d agents x 2 nets: largest float32 err %.3g, smallest max |q64| %.3g, largest walk err / fused bar %.3g"
          % (SW.case_id(case), V, worst32, least_q, worst_w))
    if dims[2] == V + 2:                                      # the from-policy form of the GPU test: the same headroom there
        heads, power, act_p, idx = SW.local_policy_inputs(dims, n, b_seed + 2)
        assert act_p.shape == (n, V, V + 2) and (act_p[:, :, :V].sum(-1) == 1).all()
        worst32 = 0.0
        for j in range(V):
            a, b = [i for i in range(V) if i != j][1:3]
            assert idx[j, 0] != j and idx[j, 1] == a and idx[j, 2] == j                # the planted rows
            s_j, a_j = np.ascontiguousarray(obs[:, j]), np.ascontiguousarray(act_p[:, j])
            for c, w in enumerate(sds[j]):
                ref = MR.critic_q64(w, s_j, a_j)
                e32 = MR.err(marl_q32(w, s_j, a_j), ref)
                worst32 = max(worst32, e32)
                assert np.abs(ref).max() > 0.05 and e32 <= HEADROOM, (j, c, e32)
        print("local %s, from the policy: largest float32 err %.3g" % (SW.case_id(case), worst32))


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
