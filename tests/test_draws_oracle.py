"""The float64 restatements of the on-device production draws that have no recorded reference to be pinned against:
`oracle.risvec_oracle.philox_fading` (3GPP fading, `draws_3gpp`) and `oracle.policy_oracle.philox_draws` (the policy
epilogue, `k_policy_sample`).  Ranges, moments at 5 sigma of their sampling error, independence of the words that must
be independent, distinct blocks per counter and sub-site -- and the Philox coordinates at which a word has all-ones top
24 bits (u == 1, Exp(1) == 0), which tests/test_draws_hip.py runs the kernels at.  CPU only."""
import math

import numpy as np
import pytest

from oracle import policy_oracle as PO
from oracle import risvec_oracle as orc

# (env id, agent, logit k) whose Gumbel word has all-ones top 24 bits at seed 77, call 1 (site 10, sub-site 0)
GUMBEL_ONES = [(192560, 0, 0), (976975, 5, 0), (805036, 5, 2)]
GUMBEL_SEED, GUMBEL_CALL = 77, 1
# (env id, vehicle) whose 3GPP word .w has all-ones top 24 bits at seed 21, channel counter 1 (site 5)
FADING_ONES = (136505, 7)
FADING_SEED, FADING_COUNTER = 21, 1

IDS = np.arange(1000, 1000 + 12500)          # x V = 8: 1e5 draws per quantity
N = IDS.size * 8


def corr(a, b):
    return float(np.corrcoef(a.ravel(), b.ravel())[0, 1])


def test_normal2_matches_the_inline_box_muller():
    rng = np.random.default_rng(0)
    a, b = (rng.integers(0, 2 ** 32, 1000, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    a[0], b[0] = 0xFFFFFFFF, 0                      # u1 == 1 -> radius 0; u2 == 0 -> (r, 0)
    n0, n1 = orc.normal2(a, b)
    u1 = ((a >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (b >> 8).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    assert np.array_equal(n0, r * np.cos(2 * np.pi * u2)) and np.array_equal(n1, r * np.sin(2 * np.pi * u2))
    assert n0[0] == 0.0 and n1[0] == 0.0
    assert np.isfinite(n0).all() and np.abs(n0).max() <= math.sqrt(2 * 24 * math.log(2.0))      # 5.77: u1 >= 2^-24


@pytest.mark.parametrize("K", [0.0, 3.0, 6.0])
def test_fading_ranges_moments_and_independence(K):
    u, z, sm = orc.philox_fading(IDS, 8, 3, 21, K)
    assert u.shape == z.shape == sm.shape == (IDS.size, 8)
    assert (u >= 0).all() and (u < 1).all() and (sm >= 0).all()
    s = 5 / math.sqrt(N)
    assert abs(u.mean() - 0.5) <= s * math.sqrt(1 / 12) and abs(u.var() - 1 / 12) <= s * math.sqrt(1 / 180)
    assert abs(z.mean()) <= s and abs(z.var() - 1.0) <= s * math.sqrt(2.0)
    # small-scale power: mean 1 for Rayleigh and Rice; variance 1 (Exp(1)) or (2K + 1) / (K + 1)^2 (Rice)
    k = 10 ** (K / 10) if K > 1e-6 else 0.0
    var = (2 * k + 1) / (k + 1) ** 2
    assert abs(sm.mean() - 1.0) <= s * math.sqrt(var)
    assert abs(sm.var() - var) <= 5 * math.sqrt(12.0 * var * var / N)        # fourth moment <= 9 var^2 for both laws
    # the shadow must not know the LOS decision, nor the small-scale power the shadow
    assert abs(corr(u, z)) <= s and abs(corr(z, sm)) <= s and abs(corr(u, sm)) <= s


def test_fading_words_counters_and_rice_site():
    e = IDS[:, None].astype(np.uint64); v = np.arange(8, dtype=np.uint64)[None, :]
    x = orc.philox4x32(e, v, np.uint64(3), np.uint64(orc.SITE_3GPP), 21)
    u, z, sm = orc.philox_fading(IDS, 8, 3, 21, 0.0)
    assert np.array_equal(u, orc.u01(x[0]).astype(np.float64))
    assert np.array_equal(z, orc.normal2(x[1], x[2])[0])
    assert np.array_equal(sm, -np.log(((x[3] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24))
    y = orc.philox4x32(e, v, np.uint64(3), np.uint64(orc.SITE_3GPP + 0x100), 21)
    ur, zr, smr = orc.philox_fading(IDS, 8, 3, 21, 6.0)
    assert np.array_equal(ur, u) and np.array_equal(zr, z)                  # K changes the power only
    assert np.array_equal(smr, orc.rice_power(*orc.normal2(y[0], y[1]), 6.0))
    assert all(not np.array_equal(a, b) for a, b in zip(x, y))              # another block, not the same words again
    # the threshold is the kernel's float32 compare: 1e-6 as a double is above float32(1e-6) ... and rounds onto it
    assert np.array_equal(orc.philox_fading(IDS[:50], 8, 3, 21, 1e-6)[2], sm[:50])
    assert not np.array_equal(orc.philox_fading(IDS[:50], 8, 3, 21, 2e-6)[2], sm[:50])
    u4, z4, sm4 = orc.philox_fading(IDS, 8, 4, 21, 0.0)
    assert not (u4 == u).all(1).any() and not np.array_equal(z4, z) and not np.array_equal(sm4, sm)
    assert abs(corr(u4, u)) <= 5 / math.sqrt(N) and abs(corr(sm4, sm)) <= 5 / math.sqrt(N)
    us, _, _ = orc.philox_fading(IDS, 8, 3, 22, 0.0)
    assert not np.array_equal(us, u)
    # sharding: rows are a function of the global env id alone
    assert np.array_equal(orc.philox_fading(IDS[300:], 8, 3, 21, 6.0)[2], smr[300:])


def test_policy_draws_ranges_moments_and_sub_sites():
    V = 8
    eps, expo = PO.philox_draws(IDS, V, 1, 77)
    assert eps.shape == (IDS.size, V, 2) and expo.shape == (IDS.size, V, V)
    assert (expo > 0).all() and np.isfinite(eps).all() and np.isfinite(expo).all()
    s = 5 / math.sqrt(N)
    for c in (0, 1):
        assert abs(eps[..., c].mean()) <= s and abs(eps[..., c].var() - 1.0) <= s * math.sqrt(2.0)
    assert abs(corr(eps[..., 0], eps[..., 1])) <= s
    n = expo.size
    assert abs(expo.mean() - 1.0) <= 5 / math.sqrt(n) and abs(expo.var() - 1.0) <= 5 * math.sqrt(8.0 / n)
    for k in range(1, V):                                   # words of one block and of the next sub-site
        assert abs(corr(expo[..., 0], expo[..., k])) <= s
    # word k & 3 of the block at site 10 + 0x100 (k >> 2), agent in c1
    e = IDS[:, None].astype(np.uint64); v = np.arange(V, dtype=np.uint64)[None, :]
    for k in (0, 3, 4, 7):
        blk = orc.philox4x32(e, v, np.uint64(1), np.uint64(10 + 0x100 * (k >> 2)), 77)
        assert np.array_equal(expo[..., k], -np.log(((blk[k & 3] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24))
    x = orc.philox4x32(e, v, np.uint64(1), np.uint64(9), 77)
    assert np.array_equal(eps[..., 0], orc.normal2(x[0], x[1])[0]) and np.array_equal(eps[..., 1], orc.normal2(x[0], x[1])[1])
    # another call, another agent count: fresh blocks / the same leading columns
    eps2, expo2 = PO.philox_draws(IDS, V, 2, 77)
    assert not np.array_equal(eps2, eps) and not (expo2 == expo).all(-1).any()
    for V2 in (1, 3, 20, 33, 64):                           # up to 16 sub-sites; partial last block
        e3, x3 = PO.philox_draws(IDS[:40], V2, 1, 77)
        m = min(V, V2)
        assert x3.shape == (40, V2, V2) and (x3 > 0).all()
        assert np.array_equal(x3[:, :m, :m], expo[:40, :m, :m]) and np.array_equal(e3[:, :m], eps[:40, :m])
    big = PO.philox_draws(IDS[:40], 64, 1, 77)[1]
    cols = big.reshape(-1, 64)
    assert len({cols[:, k].tobytes() for k in range(64)}) == 64          # 16 sub-sites x 4 words: all distinct
    assert np.array_equal(PO.philox_draws(IDS[300:340], V, 1, 77)[1], expo[300:340])


@pytest.mark.parametrize("env,agent,k", GUMBEL_ONES)
def test_gumbel_word_with_all_ones_top_bits(env, agent, k):
    """The coordinates at which -log(u) is 0: the oracle returns torch's 2^-24 there (a Gumbel of 16.6, not +inf)
    and leaves every other draw of the neighbourhood as it is."""
    ids = np.arange(env - 2, env + 3)
    blk = orc.philox4x32(np.uint64(env), np.uint64(agent), np.uint64(GUMBEL_CALL), np.uint64(10 + 0x100 * (k >> 2)), GUMBEL_SEED)
    assert int(blk[k & 3]) >> 8 == 0xFFFFFF
    _, expo = PO.philox_draws(ids, 8, GUMBEL_CALL, GUMBEL_SEED)
    assert expo[2, agent, k] == 2.0 ** -24 == PO.EXPO_FLOOR
    assert (expo == PO.EXPO_FLOOR).sum() == 1 and expo.min() == PO.EXPO_FLOOR
    assert abs(-math.log(expo[2, agent, k]) - 16.6355) < 1e-3
    raw = np.stack([orc.exp1_from_u32(w) for w in orc.philox4x32(ids[:, None].astype(np.uint64), np.arange(8, dtype=np.uint64)[None, :],
                                                               np.uint64(GUMBEL_CALL), np.uint64(10), GUMBEL_SEED)], -1)
    assert raw[2, agent, k] == 0.0
    keep = np.ones((5, 8, 4), bool); keep[2, agent, k] = False
    assert np.array_equal(raw[keep], expo[..., :4][keep])                 # the clamp changes no other draw


def test_fading_word_with_all_ones_top_bits():
    env, veh = FADING_ONES
    x = orc.philox4x32(np.uint64(env), np.uint64(veh), np.uint64(FADING_COUNTER), np.uint64(orc.SITE_3GPP), FADING_SEED)
    assert int(x[3]) >> 8 == 0xFFFFFF
    u, z, sm = orc.philox_fading(np.arange(env - 2, env + 3), 8, FADING_COUNTER, FADING_SEED, 0.0)
    assert sm[2, veh] == 0.0 and (np.delete(sm.ravel(), 2 * 8 + veh) > 0).all()
    p = orc.OracleParams()
    pos = np.full((5, 8, 2), 150.0)
    for mode in ("3gpp_umi", "3gpp_uma", "other"):
        g = orc.gain_3gpp(pos, mode, u, z, sm, p)
        assert g[2, veh] == 0.0 and (np.delete(g.ravel(), 2 * 8 + veh) > 0).all()
