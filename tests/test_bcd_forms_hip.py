"""GPU tests of every BCD form the library dispatches (k_bcd.hip: launch_colsum / launch_bcd) against the float64
oracle, on the device's own float32 inputs: each column-sum member, the generic sweep for every 2^b, the two-lane
sweep for 2^b = 8 in both of its instantiations (padded / M % 8 = 0, theta written / kept by index), its exact
tie and zero-score replay, a full run of cached-sum reuses, and the host-side cache bookkeeping that picks them
(announced direct writes to h_r / theta).  Every case asserts the kernel it ran, so that a dispatch change cannot
quietly leave a form untested.  Reference: Environment.py:208-231 (optimize_phase_shift + its objective)."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import risvec_oracle as orc  # noqa: E402  (checker)
from tests.test_hip_parity import (c128, cpu, make_vec, put_complex, random_step_inputs, record, snap)  # noqa: E402

# float32 image of candidate k = 0..7 of 2^b = 8 (what the kernels store), index -1 (the integer 0) -> 0
_R32 = np.float32(0.70710677)
_CAND32 = np.array([1, _R32 + 1j * _R32, 1j, -_R32 + 1j * _R32, -1, -_R32 - 1j * _R32, -1j, _R32 - 1j * _R32, 0],
                   dtype=np.complex64).astype(np.complex128)


def _geo_env(E, V, M, b=3, seed=0, lazy=False):
    """E envs at random vehicle positions: compute_parms() (h_r, c_col), random candidate phases."""
    rng = np.random.default_rng(seed)
    env = make_vec(E, V, M, b=b, seed=seed + 1)
    env.lazy_theta = lazy
    env.make_new_game()
    t = env.tensors
    t["pos"].copy_(torch.from_numpy(np.stack([rng.uniform(0, 400, (E, V)), rng.uniform(0, 400, (E, V))], -1)))
    env.compute_parms()
    env.Random_phase()
    return env


def _pair_name(M, lazy):
    return "k_bcd_sweep8_pair<%s,%s>" % ("PAD" if M % 8 else "M%8=0", "theta by index" if lazy else "theta written")


def _check_sweep(env, th_in, idx, bbit=3, exact=None):
    """One sweep against orc.bcd_sweep from th_in (the snapped theta it started from): decisions equal wherever the
    accumulated float64 margin exceeds 1e-9 (>= 99.9 % of them), theta within 1.5e-7.  `exact` marks exact-tie
    coordinates: they are asserted exactly by the caller and left out of the margin accumulation.  Reads
    `env.tensors`, i.e. materialises a theta kept by index."""
    t = env.tensors
    h, b = c128(t["h_r"]), c128(t["b"])
    E, M = th_in.shape
    o_th, o_idx = orc.bcd_sweep(th_in, h, b, np.ones((E, env.n_veh)), bbit)
    gap = orc.bcd_margin(th_in, h, b, bbit)
    if exact is not None:
        gap[exact] = np.inf
    safe = np.minimum.accumulate(gap, axis=1) > 1e-9          # a flipped decision taints the rest of its sweep
    record("BCD decisions left out of the comparison (fraction; float64 margin below 1e-9)", 1.0 - safe.mean())
    assert safe.mean() >= 0.999
    assert np.array_equal(idx[safe], o_idx[safe])
    th1 = c128(t["theta"])
    err = np.abs(th1 - o_th)[safe]
    record("BCD forms: max |theta - oracle theta|", err.max())
    assert err.max() <= 1.5e-7
    return th1, o_th, o_idx, h, b


def _check_state(env, idx, th1, h, b, bbit=3, ssum_tol=1e-10):
    """What a sweep leaves besides theta: the candidate bytes (2^b = 8) say what idx says, theta is exactly the
    float32 image of its candidate, and s_sum is the sum theta.c of what was stored."""
    t = env.tensors
    M = idx.shape[1]
    if bbit == 3:
        ti = cpu(t["theta_idx"])[:, :M].astype(np.int64)
        assert np.array_equal(ti, np.where(idx < 0, 8, idx))
        assert np.array_equal(th1, _CAND32[np.where(idx < 0, 8, idx)])
    S = cpu(t["s_sum"]); S = S[:, 0] + 1j * S[:, 1]
    want = np.sum(snap(th1, bbit) * (h.sum(axis=1) * b[None, :]), axis=1)
    if ssum_tol is not None:
        np.testing.assert_allclose(S, want, rtol=ssum_tol, atol=ssum_tol)
    return S, want


# ---------------------------------------------------------------------------- column sums, every member
# (E, V, M, member): rows256 groups 16 envs, the slab 64 -- every E is a tail of both; V below the template's VU
_COLSUM = [
    (17, 3, 256, "k_colsum_rows256<8>"), (130, 8, 256, "k_colsum_rows256<8>"), (1, 5, 256, "k_colsum_rows256<8>"),
    (15, 13, 256, "k_colsum_rows256<16>"), (65, 16, 256, "k_colsum_rows256<16>"),
    (63, 5, 48, "k_colsum_slab<8>"), (1, 8, 1024, "k_colsum_slab<8>"), (130, 3, 16, "k_colsum_slab<8>"),
    (65, 11, 48, "k_colsum_slab<16>"), (17, 16, 2048, "k_colsum_slab<16>"), (130, 9, 48, "k_colsum_slab<16>"),
    (1, 13, 2048, "k_colsum_slab<16>"),
    (15, 17, 256, "k_colsum<2>"), (65, 64, 2, "k_colsum<2>"), (63, 5, 36, "k_colsum<2>"), (17, 64, 2048, "k_colsum<2>"),
    (130, 17, 48, "k_colsum<2>"),
    (1, 3, 1, "k_colsum<1>"), (130, 11, 21, "k_colsum<1>"), (33, 64, 21, "k_colsum<1>"),
]


@pytest.mark.parametrize("E,V,M,name", _COLSUM)
def test_colsum_every_member(E, V, M, name):
    """c_col[e, m] = (sum_v h_r[e, v, m]) b[m] in float64 from every column-sum member, on random complex h_r
    written directly (rebuild_colsum), with the default cache policy and with the non-temporal loads forced: the
    same bits both times, and the float64 sum of the same float32 inputs to 1e-14."""
    from ris_vec_marl_amd import _native as N
    rng = np.random.default_rng(E * 7 + V * 3 + M)
    h = (rng.standard_normal((E, V, M)) + 1j * rng.standard_normal((E, V, M))) * rng.uniform(0.1, 10, (E, V, 1))
    nt_name = name if name.startswith("k_colsum<") else name[:-1] + ",NT>"      # k_colsum<VEC> has no NT form
    got = []
    for nt in (False, True):
        env = make_vec(E, V, M)
        t = env.tensors
        put_complex(t["h_r"], h)
        with N.forced(colsum_nt=True) if nt else contextlib.nullcontext():
            env.rebuild_colsum()
        assert N.last_kernel() == (nt_name if nt else name), N.last_kernel()
        c = cpu(env.colsum_rows())
        want = c128(t["h_r"]).sum(axis=1) * c128(t["b"])[None, :]
        np.testing.assert_allclose(c, want, rtol=1e-14, atol=1e-14)
        record("colsum rel err", np.max(np.abs(c - want) / np.maximum(np.abs(want), 1e-300)))
        got.append(c)
    assert np.array_equal(got[0], got[1])


# ---------------------------------------------------------------------------- the pair sweep against the oracle
# (E, V, M, lazy): PAD and M % 8 = 0, tile counts 1 .. 256 against the 4-tile index groups (5, 10, 13, 15, 32, 33
# among them), every size of the reference's RIS-element study (plt/plt-ris.py:7: 20 .. 120), E tails of the 32-env
# wavefront and of the 64-env c_col slab; lazy rows with odd M and V outside {4, 8, 16} (k_theta_from_index's tail).
# (V = 1 only at even M: one vehicle's c_m is a geometric sequence, and at odd M its middle element is a float64
# near-tie of the oracle's own -- margins of ~5e-10 from the second sweep on, which the mask has to leave out.)
_PAIR = [
    (1, 1, 2, False), (31, 5, 7, False), (33, 8, 8, False), (97, 16, 9, False), (300, 8, 20, False),
    (31, 64, 36, False), (300, 8, 40, False), (97, 8, 60, False), (300, 8, 80, False), (300, 8, 100, False),
    (300, 8, 120, False), (97, 16, 250, False), (300, 16, 256, False), (33, 5, 264, False), (33, 8, 2048, False),
    (31, 5, 7, True), (97, 5, 9, True), (97, 1, 20, True), (33, 64, 2, True), (300, 8, 20, True), (97, 5, 40, True),
    (300, 8, 60, True), (31, 16, 80, True), (300, 8, 100, True), (97, 8, 120, True), (300, 16, 256, True),
    (33, 8, 264, True), (1, 5, 2048, True),
]


@pytest.mark.parametrize("E,V,M,lazy", _PAIR)
def test_pair_sweep_vs_oracle(E, V, M, lazy):
    """One generic sweep (the candidate indices become known), then three sweeps of k_bcd_sweep8_pair -- the first
    re-sums theta.c from the indices (rebuild_colsum() in between keeps them), the next two start from the sum the
    previous one left -- each against the oracle.  With lazy_theta the sweeps keep theta by index and the tensor
    compared is what k_theta_from_index materialises."""
    from ris_vec_marl_amd import _native as N
    env = _geo_env(E, V, M, seed=E + V + M, lazy=lazy)
    for sweep in range(4):
        if sweep == 1:
            env.rebuild_colsum()                               # same c_col; the cached sum is dropped
        th_in = snap(c128(env.tensors["theta"]), 3)
        idx = cpu(env.optimize_phase_shift(return_idx=True))
        assert N.last_kernel() == ("k_bcd_sweep<8>" if sweep == 0 else _pair_name(M, lazy)), N.last_kernel()
        assert env._ssum_sweeps == max(1, sweep)
        assert env._theta_stale == (lazy and sweep > 0)
        th1, o_th, o_idx, h, b = _check_sweep(env, th_in, idx)
        _check_state(env, idx, th1, h, b)


# ---------------------------------------------------------------------------- exact ties and all-zero scores
@pytest.mark.parametrize("M", [21, 64])
@pytest.mark.parametrize("kind", ["zero", "tie"])
@pytest.mark.parametrize("lazy", [False, True])
def test_pair_sweep_exact_ties_and_zero_scores(M, kind, lazy):
    """The replay path of the pair sweep, which the margin mask can never reach (the decisions it makes have a margin
    of exactly 0).  h_r[e, :, m] = 0 makes c_m = 0 exactly: at every m of an env ("zero": S = rest = q = 0, no
    candidate scores above 0, every element becomes the integer 0, ENV:211, 220) or at chosen m ("tie": q = 0 with
    rest != 0, all candidates tie and the first wins, ENV:210-218).  The envs sit at lanes 0, 31, 32, 63 of the
    wavefronts and at the last env; those decisions are asserted exactly, the rest of the sweep under the margin."""
    from ris_vec_marl_amd import _native as N
    E, V = 97, 8
    env = _geo_env(E, V, M, seed=M + (kind == "tie") * 3 + lazy, lazy=lazy)
    env.optimize_phase_shift()                                 # generic sweep: the candidate indices become known
    t = env.tensors
    envs = [0, 31, 32, 63, E - 1]
    exact = np.zeros((E, M), dtype=bool)
    ms = [0, 1, 7, 8, 13, M - 1] if kind == "tie" else list(range(M))
    for e in envs:
        exact[e, ms] = True
        exact[e, (e * 5) % M] = True                           # one more, different per env
    hz = cpu(t["h_r"]).copy()
    hz[np.nonzero(exact)[0], :, np.nonzero(exact)[1]] = 0.0
    t["h_r"].copy_(torch.from_numpy(hz))
    env.rebuild_colsum()                                       # keeps the candidate indices valid
    assert env._idx_valid
    for sweep in range(2):                                     # re-summing pass, then the cached sum
        th_in = snap(c128(env.tensors["theta"]), 3)
        idx = cpu(env.optimize_phase_shift(return_idx=True))
        assert N.last_kernel() == _pair_name(M, lazy), N.last_kernel()
        assert env._ssum_sweeps == sweep + 1
        th1, o_th, o_idx, h, b = _check_sweep(env, th_in, idx, exact=exact)
        S, _ = _check_state(env, idx, th1, h, b)
        want_k = -1 if kind == "zero" else 0
        assert (o_idx[exact] == want_k).all()                  # the construction is what it claims in the oracle
        assert (idx[exact] == want_k).all(), np.argwhere(exact & (idx != want_k))[:5]
        assert np.array_equal(th1[exact], o_th[exact])         # 0, or the phasor 1 exactly
        assert (th1[exact] == (0 if kind == "zero" else 1)).all()
        ti = cpu(env.tensors["theta_idx"])[:, :M]
        assert (ti[exact] == (8 if kind == "zero" else 0)).all()
        if kind == "zero":
            assert (S[envs] == 0).all()


# ---------------------------------------------------------------------------- every control_bit
@pytest.mark.parametrize("b", [0, 1, 2, 4, 5, 6])
@pytest.mark.parametrize("E,V,M", [(130, 5, 21), (97, 8, 64)])
def test_generic_sweep_every_control_bit(b, E, V, M):
    """k_bcd_sweep<2^b> for every 2^b but 8: two consecutive sweeps against the oracle, the second starting from the
    sum the first left in s_sum."""
    from ris_vec_marl_amd import _native as N
    env = _geo_env(E, V, M, b=b, seed=10 * b + M)
    for sweep in range(2):
        th_in = snap(c128(env.tensors["theta"]), b)
        idx = cpu(env.optimize_phase_shift(return_idx=True))
        assert N.last_kernel() == "k_bcd_sweep<%d>" % (1 << b), N.last_kernel()
        assert env._ssum_sweeps == sweep + 1
        th1, o_th, o_idx, h, bb = _check_sweep(env, th_in, idx, bbit=b)
        _check_state(env, idx, th1, h, bb, bbit=b)


# ---------------------------------------------------------------------------- a full cached-sum streak
def test_cached_sum_streak_of_64_sweeps():
    """C5's cadence, step(bcd=True) on fixed geometry, 70 times, eager and lazy theta side by side (bit for bit):
    sweep 1 re-sums theta.c, sweeps 2..64 start from s_sum, sweep 65 re-sums again (vec_env._bcd_flags).  Every
    sweep's decisions match the oracle under the margin mask.

    Drift bound of the cached sum.  Per coordinate a sweep updates each float64 component of S with at most six
    rounded operations (the pair kernel: four fused ones) -- remove the old term, add the new one -- each off by at
    most 2^-53 of a value below |S| + 2|c_m| <= sum|c| + 2|c_m|; so one sweep moves S by at most
    6 sqrt(2) (M + 2) 2^-53 sum|c| away from the exact sum of what it stored, and a re-summing sweep at most twice
    that.  Over the 64 sweeps of one streak (63 reuses), with the float64 reference sum's own M 2^-53 sum|c|:
        |s_sum - sum theta.c| <= 64 * 16 * (M + 2) * 2^-53 * sum_m |c_m|     per env."""
    from ris_vec_marl_amd import _native as N
    E, V, M = 300, 8, 60
    rng = np.random.default_rng(64)
    action, partner, ng, _ = random_step_inputs(E, V, rng)
    a, pt, ngt = action.astype(np.float32), partner.astype(np.int32), ng.astype(np.int32)
    envs = [_geo_env(E, V, M, seed=64, lazy=lazy) for lazy in (False, True)]
    eager, lz = envs
    t = eager.tensors
    h, b = c128(t["h_r"]), c128(t["b"])
    c = h.sum(axis=1) * b[None, :]
    bound = 64 * 16 * (M + 2) * 2.0 ** -53 * np.abs(c).sum(axis=1)
    seen, worst = [], 0.0
    for i in range(70):
        th_in = snap(c128(eager.tensors["theta"]), 3)
        for env in envs:
            env.step(a, pt, ngt, None, fused=True, bcd=True)
        seen.append(eager._ssum_sweeps)
        assert lz._ssum_sweeps == eager._ssum_sweeps
        assert lz._theta_stale == (i > 0) and not eager._theta_stale
        if i > 0:                                            # the lazy env's step read theta by index
            assert ",TK" in N.last_kernel(), N.last_kernel()
        for k in ("theta", "theta_idx", "s_sum", "gain", "reward", "data_buf"):
            assert torch.equal(eager.tensors[k], lz.tensors[k]), (i, k)
        idx = cpu(eager.tensors["theta_idx"])[:, :M].astype(np.int64)
        idx = np.where(idx == 8, -1, idx)
        th1, o_th, o_idx, _, _ = _check_sweep(eager, th_in, idx)
        S, want = _check_state(eager, idx, th1, h, b, ssum_tol=None)
        drift = np.abs(S - want)
        assert (drift <= bound).all(), (i, float(np.max(drift / bound)))
        worst = max(worst, float(np.max(drift / bound)))
        if eager._ssum_sweeps == 1:                          # a re-summing sweep: one sweep's rounding only
            np.testing.assert_allclose(S, want, rtol=1e-10, atol=1e-10)
        if eager._ssum_sweeps == 64:
            record("s_sum drift after 63 reuses (max over envs, / 2^-52 M sum|c|)",
                   np.max(drift / (2.0 ** -52 * M * np.abs(c).sum(axis=1))))
    assert seen == list(range(1, 65)) + list(range(1, 7)), seen
    record("s_sum drift over the streak (fraction of the stated bound)", worst)


# ---------------------------------------------------------------------------- announced direct writes
def test_announced_writes_keep_lazy_theta_equal_to_eager():
    """A lazy_theta env and an eager one, driven alike through every announced direct write while the lazy one holds
    theta by index (the tensors dict is held from before the sweeps, as a caller would): h_r + invalidate_colsum()
    must not lose the sweeps kept by index, a theta write announced with invalidate_colsum() / invalidate_theta()
    makes the written tensor the truth, h_r + rebuild_colsum() keeps the indices.  After each pattern both envs
    equal each other bit for bit and the oracle's sweep from the theta the pattern leaves."""
    from ris_vec_marl_amd import _native as N
    E, V, M = 130, 8, 36
    rng = np.random.default_rng(36)
    action, partner, ng, _ = random_step_inputs(E, V, rng)
    a, pt, ngt = action.astype(np.float32), partner.astype(np.int32), ng.astype(np.int32)
    envs = [_geo_env(E, V, M, seed=36, lazy=lazy) for lazy in (False, True)]
    held = [env.tensors for env in envs]                     # a reference kept across the sweeps
    eager, lz = envs
    keys = ("theta", "theta_idx", "s_sum", "gain", "reward", "data_buf", "mec_q", "metrics", "obs")

    def steps(n):
        for _ in range(n):
            for env in envs:
                env.step(a, pt, ngt, None, fused=True, bcd=True)

    def h_r_write(t, r):
        put_complex(t["h_r"], c128(t["h_r"]) * np.exp(1j * r.uniform(0, 2 * np.pi, (E, V, M))))

    def theta_write(t, r):
        put_complex(t["theta"], np.exp(1j * r.uniform(0, 2 * np.pi, (E, M))))

    patterns = [("h_r + invalidate_colsum", h_r_write, "invalidate_colsum"),
                ("theta + invalidate_colsum", theta_write, "invalidate_colsum"),
                ("theta + invalidate_theta", theta_write, "invalidate_theta"),
                ("h_r + rebuild_colsum", h_r_write, "rebuild_colsum")]
    steps(3)                                                 # generic sweep, then two kept by index
    for what, write, announce in patterns:
        assert lz._theta_stale, what
        th_eager = c128(held[0]["theta"])                    # what the sweeps left (the eager env writes it)
        for env, t in zip(envs, held):
            write(t, np.random.default_rng(len(what)))       # the same write into both envs
            getattr(env, announce)()
        th_in = snap(c128(held[0]["theta"]) if write is theta_write else th_eager, 3)
        steps(1)
        if announce == "rebuild_colsum":                     # the indices survive: the pair sweep, by index
            assert lz._theta_stale and ",TK" in N.last_kernel(), (what, N.last_kernel())
        for k in keys:
            assert torch.equal(eager.tensors[k], lz.tensors[k]), (what, k)
        for env in envs:
            idx = cpu(env.tensors["theta_idx"])[:, :M].astype(np.int64)
            idx = np.where(idx == 8, -1, idx)
            th1, o_th, o_idx, h, b = _check_sweep(env, th_in, idx)
            _check_state(env, idx, th1, h, b)
        steps(2)                                             # the lazy env holds theta by index again


def test_steer_refused_after_announced_h_r_write():
    """invalidate_colsum() announces a direct h_r write: from there h_r is not known to be the steering vectors
    z_r^m, so the steering form of the fused step is refused (as after rebuild_colsum()) instead of computing
    gains from the old z_r; compute_parms() makes it valid again."""
    E, V, M = 64, 8, 64
    rng = np.random.default_rng(8)
    action, partner, ng, _ = random_step_inputs(E, V, rng)
    args = (action.astype(np.float32), partner.astype(np.int32), ng.astype(np.int32))
    env = _geo_env(E, V, M, seed=8)
    env.step(*args, fused=True, steer=True)                   # valid right after compute_parms()
    t = env.tensors
    put_complex(t["h_r"], c128(t["h_r"]) * np.exp(1j * rng.uniform(0, 2 * np.pi, (E, V, M))))
    env.invalidate_colsum()
    with pytest.raises(ValueError, match="steering vectors"):
        env.step(*args, fused=True, steer=True)
    with pytest.raises(ValueError, match="steering vectors"):
        env.bind_step(torch.from_numpy(args[0]).cuda(), torch.from_numpy(args[1]).cuda(),
                      torch.from_numpy(args[2]).cuda(), None, fused=True, steer=True)
    # the plain fused step reads the h_r that was written
    env.step(*args, fused=True)
    img = np.einsum("em,evm,m->ev", c128(t["theta"]), c128(t["h_r"]), c128(t["b"]))
    pl = cpu(t["pl"]).astype(np.float64)
    gain = pl * np.abs(img) ** 2
    assert (np.abs(cpu(t["gain"]) - gain) <= 1e-5 * gain + pl * 2 * np.abs(img) * (3 * 6e-8 * M)).all()
    env.compute_parms()
    env.step(*args, fused=True, steer=True)
