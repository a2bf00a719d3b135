"""CPU-side checks of the sweep of tests/test_policy_forward_hip.py, at the very shapes, seeds and row counts it uses
(tests/policy_forward_shapes.py):
  * the table is what it says: the dispatch rules of k_policy.hip, restated in Python, name the kernels each case lists;
    every NT and FPL of {1, 2, 4, 8, 16} is reached for layer 1 and for the heads, every NT by the split-fp16 layer 1,
    both MT and every input_dims 1..5 by the fused kernel; `risvec_policy_mlp_supported` agrees with the fused list; the
    rounds, NG, H and LDS bytes the edges speak of have the stated values; the guards refuse one step past them;
  * the float64 restatement (tests/policy_forward_ref.py) is the reference's network: on every tests/golden/policy_*.npz
    it equals `oracle.policy_oracle.forward` and the recorded float32 outputs to the 5e-6 of test_policy_hip.py;
  * the inputs leave headroom under the project's bars: a plain torch float32 forward on the CPU -- what
    `forward_heads_torch` computes, up to the order of its sums -- is within BAR / 8 of float64, for the whole forward,
    for layer 1 alone and for the heads from the random `g`, so a kernel that meets fused_bar(library err) is inside
    BAR as well and the two bars never pull against each other.
Every figure is printed before it is asserted (pytest -s shows them)."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import policy_oracle as PO
from ris_vec_marl_amd import _native as N
from tests import policy_forward_ref as R
from tests import policy_forward_shapes as PS

F = torch.nn.functional
HEADROOM = R.BAR / 8.0                        # fused_bar(e) = 8 e <= BAR for every library err e below this
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def t32(w, k):
    return torch.from_numpy(np.asarray(w[k], np.float32))


def ln_relu32(x, w, name):
    """relu(LayerNorm) as `BatchedPolicy.forward_heads_torch` writes it"""
    return torch.relu(F.layer_norm(x, (x.shape[-1],)) * t32(w, name + ".weight") + t32(w, name + ".bias"))


def layer1_32(w, obs):
    return ln_relu32(F.linear(torch.tensor(obs), t32(w, "fc1.weight"), t32(w, "fc1.bias")), w, "bn1")


def heads_from_g32(w, g):
    h = ln_relu32(torch.tensor(g) + t32(w, "fc2.bias"), w, "bn2")
    return torch.cat([F.linear(h, t32(w, k + ".weight"), t32(w, k + ".bias")) for k in R.HEAD_NAMES], -1)


def heads32(w, obs):
    return heads_from_g32(w, F.linear(layer1_32(w, obs), t32(w, "fc2.weight")).numpy())


# --------------------------------------------------------------------------------------------------------- the table
def test_table_names_the_kernels_and_every_instantiation_is_reached():
    lib = N.load()
    for kind, cases in PS.LISTS.items():
        for case in cases:
            IN, F1, F2, V = case.dims
            assert case.layer1 == PS.layer1_kernel(IN, F1) and case.heads == PS.heads_kernel(F2), case
            assert 1 <= F1 <= 1024 and 1 <= F2 <= 1024
            assert PS.layer1_lds(IN, F1) <= PS.LDS_LIMIT and PS.heads_lds(F2, 4 + V) <= PS.LDS_LIMIT, case
            fused_ok = lib.risvec_policy_mlp_supported(IN, F1, F2, 4 + V) == 1
            split_ok = PS.split16_kernel(IN, F1) is not None
            assert fused_ok == (kind == "fused") == (case.fused is not None), case
            assert case.modes == (("fused",) if fused_ok else ()) + (("fp16x3",) if split_ok else ()) + ("fp32",), case
            if fused_ok:
                assert case.fused == "k_policy_mlp<%d>" % (F2 // 32) and F1 % 32 == 0 and F2 in (128, 256)
    every = {"v4<%d>" % k for k in (1, 2, 4, 8, 16)}
    assert {c.layer1 for c in PS.V4} == every and {c.heads for c in PS.V4} == every
    every = {"<%d>" % k for k in (1, 2, 4, 8, 16)}
    assert {c.layer1 for c in PS.GENERAL} == every and {c.heads for c in PS.GENERAL} == every
    assert {PS.split16_kernel(*c.dims[:2]) for c in PS.V4} == {"v4<%d,8,true>" % k for k in (1, 2, 4, 8, 16)}
    assert all(PS.split16_kernel(*c.dims[:2]) is None for c in PS.GENERAL)
    assert {c.fused for c in PS.FUSED} == {"k_policy_mlp<4>", "k_policy_mlp<8>"}
    assert {c.dims[0] for c in PS.FUSED} == {1, 2, 3, 4, 5}
    assert len({c.dims for cases in PS.LISTS.values() for c in cases}) == len(PS.RUNS) == 18
    # what the fused kernel is NOT built for: 25 heads, fc2 = 64, six inputs
    assert lib.risvec_policy_mlp_supported(5, 64, 128, 25) == 0 and lib.risvec_policy_mlp_supported(5, 64, 128, 24) == 1
    assert lib.risvec_policy_mlp_supported(5, 64, 64, 8) == 0 and lib.risvec_policy_mlp_supported(6, 64, 128, 8) == 0


def test_table_edges_have_the_stated_figures():
    # 16 lanes per row: (chunks, rounds needed, NT) of fc1 and fc2
    fig = [tuple((F // 4, PS.need16(F), PS.nt(F)) for F in c.dims[1:3]) for c in PS.V4]
    assert fig == [((5, 1, 1), (3, 1, 1)), ((16, 1, 1), (17, 2, 2)), ((32, 2, 2), (33, 3, 4)), ((64, 4, 4), (65, 5, 8)),
                   ((65, 5, 8), (64, 4, 4)), ((129, 9, 16), (128, 8, 8)), ((256, 16, 16), (256, 16, 16))]
    assert [PS.heads_of(c) for c in PS.V4] == [6, 5, 7, 20, 8, 12, 12]
    assert PS.V4[1].dims[0] == PS.INMAX and PS.V4[1].dims[3] == 1
    # chunks in the last needed round, and rounds of NT that hold none
    last = [tuple((F // 4 - 16 * (PS.need16(F) - 1), PS.nt(F) - PS.need16(F)) for F in c.dims[1:3]) for c in PS.V4]
    assert last[1][1] == (1, 0) and last[2][1] == (1, 1) and last[3][1] == (1, 3) and last[4][0] == (1, 3) and last[5][0] == (1, 7)
    assert -(-PS.heads_of(PS.V4[3]) // 16) == 2 and PS.heads_of(PS.V4[3]) - 16 == 4
    # the heads LDS at fc2 = 1024: 12 heads fit, 13 do not
    assert PS.heads_lds(1024, 12) == 61488 <= PS.LDS_LIMIT < PS.heads_lds(1024, 13) == 65588
    assert PS.HEADS_LDS_OVER == PS.V4[6].dims[:3] + (PS.V4[6].dims[3] + 1,)
    assert PS.layer1_lds(*PS.LAYER1_LDS_LAST) == 65536 == PS.LDS_LIMIT < PS.layer1_lds(*PS.LAYER1_LDS_OVER) == 69632
    # one wavefront per row: (rounds needed, FPL, features in the last needed round)
    fig = [tuple((PS.need64(F), PS.fpl(F), F - 64 * (PS.need64(F) - 1)) for F in c.dims[1:3]) for c in PS.GENERAL]
    assert fig == [((1, 1, 1), (1, 1, 63)), ((2, 2, 64), (2, 2, 1)), ((3, 4, 2), (3, 4, 2)), ((5, 8, 2), (5, 8, 2)),
                   ((16, 16, 63), (9, 16, 2))]
    assert [PS.heads_of(c) for c in PS.GENERAL] == [6, 9, 20, 37, 8]
    assert PS.GENERAL[1].dims[0] == 9 > PS.INMAX and PS.GENERAL[1].dims[1] % 4 == 0 and PS.GENERAL[2].dims[0] == 3
    # fused: (IN, NG, MT, H); float4 stores iff H % 4 == 0
    fig = [(c.dims[0], c.dims[1] // 32, c.dims[2] // 32, PS.heads_of(c)) for c in PS.FUSED]
    assert fig == [(1, 1, 4, 5), (2, 2, 8, 24), (3, 3, 4, 8), (4, 4, 8, 9), (5, 31, 4, 23), (5, 32, 8, 12)]
    assert [h % 4 == 0 for _, _, _, h in fig] == [False, True, True, False, False, True]
    # rows: 64 per block of the 16-lane kernels, 32 of the general ones, 256 per fused workgroup in wavefronts of 32
    assert divmod(PS.ROWS, 64) == (4, 33) and 33 % 4 == 1 and divmod(PS.ROWS, 32) == (9, 1)
    assert divmod(PS.ROWS, 256) == (1, 33) and divmod(33, 32) == (1, 1)
    assert PS.FUSED_H_OVER[3] + 4 == 25


def test_guards_refuse_one_step_past_their_bounds():
    """The shape checks of the C ABI come before any pointer is looked at or any device touched"""
    lib = N.load()
    p = 16                                                                      # never dereferenced
    IN, F1, F2, V = PS.HEADS_LDS_OVER
    assert lib.risvec_policy_heads(PS.ROWS, V, F2, 4 + V, p, p, p, p, p, p, p, None) == N.ERR_SHAPE
    assert lib.risvec_policy_layer1(PS.ROWS, 1, *PS.LAYER1_LDS_OVER, p, p, p, p, p, p, None) == N.ERR_SHAPE
    assert lib.risvec_policy_layer1_split16(PS.ROWS, 1, 9, 128, p, p, p, p, p, p, None) == N.ERR_SHAPE
    assert lib.risvec_policy_layer1_split16(PS.ROWS, 1, 5, 130, p, p, p, p, p, p, None) == N.ERR_SHAPE
    assert lib.risvec_policy_mlp(PS.ROWS, 21, 5, 64, 128, 25, *([p] * 12), None) == N.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------- the restatement is the reference
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "policy_*.npz"))), ids=os.path.basename)
def test_forward64_is_the_oracle_and_the_recorded_forward(path):
    d = np.load(path)
    V = int(d["V"])
    assert V >= 1
    for a in range(V):
        w = {k[len("a%d." % a):]: d[k] for k in d.files if k.startswith("a%d." % a)}
        mu, log_std, logits = R.forward64(w, d["state"][a])
        o_mu, o_ls, o_lg = PO.forward(w, d["state"][a])
        assert np.array_equal(mu, o_mu) and np.array_equal(np.clip(log_std, -20.0, 2.0), o_ls) and np.array_equal(logits, o_lg)
        assert np.array_equal(R.heads64(w, d["state"][a]), np.concatenate([mu, log_std, logits], -1))
        worst = max(float(np.abs(mu - d["mu"][a]).max()), float(np.abs(np.clip(log_std, -20.0, 2.0) - d["log_std"][a]).max()),
                    float(np.abs(logits - d["logits"][a]).max()))
        print("%s agent %d: forward64 against the recorded float32 outputs %.3g" % (os.path.basename(path), a, worst))
        np.testing.assert_allclose(mu, d["mu"][a], atol=5e-6, rtol=0)
        np.testing.assert_allclose(np.clip(log_std, -20.0, 2.0), d["log_std"][a], atol=5e-6, rtol=0)
        np.testing.assert_allclose(logits, d["logits"][a], atol=5e-6, rtol=0)


# ------------------------------------------------------------------------------------------------------ the headroom
@pytest.mark.parametrize("run", PS.RUNS, ids=[PS.run_id(r) for r in PS.RUNS])
def test_inputs_leave_headroom(run):
    D = R.case_data(*run)
    IN, F1, F2, V = D.dims
    what = "%s %s" % (run[0], PS.case_id(D.case))
    assert D.obs.shape == (PS.ROWS, V, IN) and not D.obs[0].any() and (D.obs[1] == np.float32(1.2)).all()
    assert 0.0 <= D.obs.min() and D.obs.max() <= np.float32(1.2) and D.g.shape == (V, PS.ROWS, F2) and not D.g[:, 0].any()
    e_all, e_l1, e_hd, small = [], [], [], []
    for a in range(V):
        w = D.weights[a]
        assert w["bn1.weight"][-1] == 2.0 and w["bn2.weight"][0] == -1.0 and w["bn2.weight"][-1] == 2.0
        assert w["bn1.weight"][0] == (-1.0 if F1 > 1 else 2.0)
        assert a == 0 or not np.array_equal(w["fc1.weight"], D.weights[0]["fc1.weight"])
        obs = np.ascontiguousarray(D.obs[:, a])
        e_all.append(R.err(heads32(w, obs).numpy(), D.heads_64[a]))
        e_l1.append(R.err(layer1_32(w, obs).numpy(), D.h1_64[a]))
        e_hd.append(R.err(heads_from_g32(w, D.g[a]).numpy(), D.heads_g_64[a]))
        small.append(min(float(np.abs(D.heads_64[a]).max()), float(np.abs(D.heads_g_64[a]).max())))
    print("%s: float32 against float64, worst of %d agents: forward %.3g, layer 1 %.3g, heads from g %.3g; "
          "smallest max |heads64| %.3g" % (what, V, max(e_all), max(e_l1), max(e_hd), min(small)))
    assert min(small) > 0.05                                    # the widened heads: not a zero output
    assert max(e_all) <= HEADROOM and max(e_l1) <= HEADROOM and max(e_hd) <= HEADROOM
    if F1 == 1:
        # LayerNorm over one feature: x - mean is exactly 0, the output is ReLU(bias) whatever the observation, in
        # float32 as in float64
        assert max(e_l1) == 0.0
        assert all(np.array_equal(D.h1_64[a], np.broadcast_to(np.maximum(D.weights[a]["bn1.bias"].astype(np.float64), 0.0), (PS.ROWS, 1)))
                   for a in range(V))
