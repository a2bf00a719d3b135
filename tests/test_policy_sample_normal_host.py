"""`risvec_policy_sample_normal` / `BatchedPolicy.sample_normal` without a GPU: the symbol is declared, exported and
bound at ABI 17; the entry point's argument checks run before any launch; and tests/policy_logp_ref.py, the float64
restatement the GPU tests compare against, reproduces what the reference's own `PolicyNetwork.sample_normal` returned
(tests/golden/logp_policy_*.npz, tools/capture_golden_policy_logp.py).

Bounds (tests/policy_logp_ref.py): power / y / one-hot as tests/test_policy_oracle_golden.py; logp_power within
1e-5 |ref| + 2^-20 + the row's two saturation floors; logp_intent within 1e-5 |ref| + 2^-20.  The reference's side of
the comparison is float32 (`Normal.log_prob` on x_t, `log_softmax`), so this is also the statement that its formulas
stay inside those bounds against float64 on rows that do not saturate.  `[logp margin]` lines print the largest
error next to its bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import policy_oracle as PO
from ris_vec_marl_amd import _native as N
from tests import policy_logp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "risvec_policy_sample_normal"


def test_symbol_is_declared_exported_and_bound_at_abi_17():
    header = open(os.path.join(ROOT, "include", "risvec.h")).read()
    assert re.search(r"\bint %s\s*\(" % NAME, header)
    assert int(re.search(r"#define RISVEC_ABI_VERSION (\d+)", header).group(1)) == 17 == N.ABI_VERSION
    assert NAME in N.EXPORTS
    res, args = N._PROTOS[NAME]
    assert res is C.c_int and len(args) == 19
    decl = re.search(r"int %s\s*\((.*?)\);" % NAME, header, re.S).group(1)
    assert len(decl.split(",")) == len(args)
    lib = N.load()
    assert hasattr(lib, NAME) and lib.risvec_abi_version() == 17
    from ris_vec_marl_amd import BatchedPolicy
    assert callable(BatchedPolicy.sample_normal) and callable(BatchedPolicy.sample_normal_torch)


def test_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf = (C.c_float * 64)()                                   # host memory: never dereferenced, only checked
    p = (C.addressof(buf) + 15) & ~15
    base = dict(n=4, V=8, off=0, heads=p, mask=None, tau=p, hard=None, eps=None, expo=None, power=p, probs=None, na=None,
                lpp=None, lpi=None, sp=None, si=None)

    def call(**kw):
        a = dict(base, **kw)
        return getattr(lib, NAME)(a["n"], a["V"], a["off"], a["heads"], a["mask"], a["tau"], a["hard"], a["eps"], a["expo"], 3, 1,
                                  a["power"], a["probs"], a["na"], a["lpp"], a["lpi"], a["sp"], a["si"], None)

    assert call(n=0) == N.OK                                   # an empty batch: OK, nothing launched
    assert call(n=0, heads=None, tau=None, power=None) == N.OK
    assert call(n=-1) == N.ERR_ARG
    assert call(heads=None) == N.ERR_ARG and b"heads" in lib.risvec_last_error()
    assert call(tau=None) == N.ERR_ARG and b"tau" in lib.risvec_last_error()
    for V in (0, -3, 65, 100):
        assert call(V=V) == N.ERR_ARG and b"n_veh" in lib.risvec_last_error()
    assert call(power=None) == N.ERR_ARG and b"no output" in lib.risvec_last_error()
    assert call(power=p + 4) == N.ERR_ARG and b"aligned" in lib.risvec_last_error()
    assert call(off=-1) == N.ERR_ARG and call(off=0xFFFFFFFF) == N.ERR_ARG
    for V in (17, 20, 64):                                     # the sums are built for V <= 16
        assert call(V=V, sp=p) == N.ERR_ARG and b"n_veh <= 16" in lib.risvec_last_error()
        assert call(V=V, power=None, si=p) == N.ERR_ARG and b"n_veh <= 16" in lib.risvec_last_error()


def _margin(what, err, bound):
    i = int(np.argmax(err / bound))
    print("[logp margin] %s: max err %.3g (bound there %.3g), max err / bound %.3f" % (what, err.max(), bound.ravel()[i], (err / bound).max()))


@pytest.mark.parametrize("name", R.FIXTURES)
def test_float64_restatement_reproduces_the_references_outputs(name):
    fx = R.fixture(name)
    V, B = int(fx["V"]), int(fx["B"])
    assert fx["logp_power"].shape == fx["logp_intent"].shape == (V, B) and fx["power"].shape == (V, B, 2)
    assert fx["has_mask"].any() and not fx["has_mask"].all() and fx["hard"].any() and not fx["hard"].all()
    assert set(np.unique(fx["tau"])) <= {2.0, 1.0, 0.5}
    for a in range(V):
        w = R.agent_weights(fx, a)
        mu, log_std, logits = PO.forward(w, fx["state"][a])
        for got, key in ((mu, "mu"), (log_std, "log_std"), (logits, "logits")):
            np.testing.assert_allclose(got, fx[key][a], atol=2e-6)
        mask = fx["mask"][a] if fx["has_mask"][a] else None
        if mask is not None:
            assert not mask[0].any()                            # the all-zero row
        hard, tau = bool(fx["hard"][a]), float(fx["tau"][a])
        # the restatement on the fixture's own float32 heads: what is compared is the epilogue
        r = R.sample_normal(fx["mu"][a], fx["log_std"][a], fx["logits"][a], mask, tau, fx["eps"][a], fx["expo"][a], hard)
        np.testing.assert_allclose(r["power"], fx["power"][a], atol=1e-5)
        soft = PO.sample_heads(fx["mu"][a], fx["log_std"][a], fx["logits"][a], mask, tau, fx["eps"][a], fx["expo"][a])[1]
        clear = PO.top2_gap(soft) > 1e-4
        assert clear.mean() > 0.9
        ref_onehot = np.eye(V)[fx["probs"][a].argmax(-1)]
        assert np.array_equal(r["onehot"][clear], ref_onehot[clear])
        if hard:
            np.testing.assert_allclose(r["y"][clear], fx["probs"][a][clear], atol=2e-7)
        else:
            np.testing.assert_allclose(r["y"], fx["probs"][a], atol=1e-5)
        e_p, b_p = np.abs(r["logp_power"] - fx["logp_power"][a]), R.bound_power(r["logp_power"], r["floor"])
        _margin("%s agent %d logp_power" % (name, a), e_p, b_p)
        assert (e_p <= b_p).all(), np.argwhere(e_p > b_p)[:5]
        sel = clear if hard else np.ones(B, bool)               # a hard row is its arg-max: judged where that is decided
        e_i, b_i = np.abs(r["logp_intent"] - fx["logp_intent"][a])[sel], R.bound_intent(r["logp_intent"])[sel]
        _margin("%s agent %d logp_intent (%s)" % (name, a, "hard" if hard else "soft"), e_i, b_i)
        assert (e_i <= b_i).all(), np.argwhere(e_i > b_i)[:5]
        np.testing.assert_array_equal(fx["logp_total"][a], fx["logp_power"][a] + fx["logp_intent"][a])


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixture_rarely_saturates(name):
    fx = R.fixture(name)
    p = fx["power"].astype(np.float64)
    floor = 2.0 ** -22 / (1.0 - p * p + 1e-6)
    share = float((floor > R.FLOOR_CAP).mean())
    print("[logp margin] %s: %.2f %% of the samples have a floor above %g; largest floor %.3g" % (name, 100 * share, R.FLOOR_CAP, floor.max()))
    assert share <= R.FLOOR_CAP_SHARE


def test_restatement_edge_cases():
    """Blocked entries contribute exactly nothing, a single open entry gives logp_intent == 0, and the eps form of the
    Normal term is the float64 value of the reference's (x_t - mu)^2 / (2 var) form."""
    rng = np.random.default_rng(3)
    B, V = 7, 5
    mu, ls, lg = rng.uniform(-1, 1, (B, 2)), rng.uniform(-3, -0.5, (B, 2)), rng.uniform(-3, 3, (B, V))
    eps, expo = rng.normal(size=(B, 2)), rng.exponential(size=(B, V))
    mask = np.zeros((B, V)); mask[:, 2] = 1.0
    for hard in (False, True):
        r = R.sample_normal(mu, ls, lg, mask, 0.3, eps, expo, hard)
        assert np.isfinite(r["logp_intent"]).all() and (r["logp_intent"] == 0.0).all()
        assert (r["onehot"][:, 2] == 1.0).all()
    r = R.sample_normal(mu, ls, lg, None, 1.0, eps, expo)
    std = np.exp(ls)
    x_t = mu + std * eps
    p32 = np.tanh(x_t).astype(np.float32).astype(np.float64)
    want = (-(x_t - mu) ** 2 / (2 * std ** 2) - ls - 0.5 * np.log(2 * np.pi) - np.log(1 - p32 ** 2 + 1e-6)).sum(-1)
    np.testing.assert_allclose(r["logp_power"], want, rtol=1e-12, atol=1e-12)
