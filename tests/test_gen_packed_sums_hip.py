"""GPU tests of the complex sums in the row-per-lane leaf of the one-group GEN member (gen_row_lane_form, k_step_gen.hip)
on the inputs at which another way of issuing cfma's four fused multiply-adds -- two packed ones on (re, im) pairs, with
the first term of a partial added to a constant +0 -- could differ from it: the sign of a zero product against the +0 a
partial starts from, subnormal products and partial sums, large magnitudes, and partials that cancel exactly.  (The
packed leaf was built and measured, EXPERIMENTS.md 2026-10-20 (d); it gave these bits and no time, and the leaf is
cfma.  The inputs stay for whoever touches the leaf next.)  The member the rule deals (one group per wavefront) against
the reading form (h_r touched through torch); `torch.equal` on the int32 view of `gain` and of every other tensor a step
writes, after each of two steps.  No tolerance anywhere.

theta as a tensor, one kind per env (env index mod 5):
  0  every component one of +0, -0, +1, -1 or a normal draw: zero products of either sign, in either component;
  1  normal draws times 10^u, u uniform in [-45, -38]: subnormal (and flushed-to-zero) entries, subnormal products and sums;
  2  normal draws, with 1e18 (the sign alternates from env to env of this kind) in one component of one element;
  3  element 2g + 1 = -(element 2g): with b = 1 and a row of ones (hand-placed vehicle 0) every partial cancels exactly;
  4  each element of one of the kinds above, at random.
theta by index: candidate 8 (the zero entry of the table) scattered.

One element of 1e18 per env is what the step keeps finite with a factor 10 to spare (two would not):
test_special_theta_keeps_the_step_finite (no GPU) bounds the float32 intermediates from |h_r| = |b| = 1, the largest
path-loss factor of the field and P_max / noise."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests.test_gen_row_lane_hip import ROW_LANE_SHAPES, _check_launch, _compare  # noqa: E402
from tests.test_h_r_rebuild_hip import _place  # noqa: E402
from tests.test_theta_index_step_hip import DEV, STEP_KEYS, _N, _env, _inputs  # noqa: E402

STEPS = 2
BIG = 1e18
SIZES = [("1", lambda epw: 1), ("EPW+1", lambda epw: epw + 1)]


def _special_theta(E, M, seed=0):
    """[E, M, 2] float32, the kinds of the module's docstring; the same for every run of a case"""
    rng = np.random.default_rng(1000 * E + M + seed)
    normal = rng.standard_normal((E, M, 2)).astype(np.float32)

    def zeros_and_ones():
        pick = rng.integers(0, 5, (E, M, 2))
        vals = np.array([0.0, -0.0, 1.0, -1.0, 0.0], dtype=np.float32)
        return np.where(pick == 4, normal, vals[pick]).astype(np.float32)

    def subnormal():
        with np.errstate(under="ignore"):
            return (normal.astype(np.float64) * 10.0 ** rng.uniform(-45.0, -38.0, (E, M, 1))).astype(np.float32)

    def big():
        th = normal.copy()
        sign = np.where((np.arange(E) // 5) % 2 == 0, 1.0, -1.0)
        th[:, M - 5, 0] = sign * BIG
        return th

    def pairs():
        th = (normal.astype(np.float64) * 10.0 ** rng.uniform(-3.0, 3.0, (E, M, 1))).astype(np.float32)
        th[:, 1::2] = -th[:, 0::2]
        return th

    kinds = [zeros_and_ones(), subnormal(), big(), pairs()]
    th = np.empty((E, M, 2), dtype=np.float32)
    for e in range(E):
        k = e % 5
        if k < 4:
            th[e] = kinds[k][e]
        else:
            which = rng.integers(0, 3, M)                # (the pairs and the two large elements only as whole envs)
            th[e] = np.choose(which[:, None], [kinds[0][e], kinds[1][e], normal[e]])
    return th


def test_special_theta_keeps_the_step_finite():
    """|h_r| = |b| = 1, so every partial sum of an env is bounded by the sum of |re| + |im| over its theta; gain = pl |img|^2
    and the rate's P_max gain / noise must stay inside float32 at the largest path-loss factor a vehicle can see."""
    from oracle import risvec_oracle as orc
    p = orc.OracleParams()
    snr_scale = max(q.P_max / q.noise_power for q in (p, orc.OracleParams.yaml_effective()))
    d_min = abs(orc.VEH_HEIGHT - orc.RIS_XYZ[2])           # a vehicle right under the RIS
    pl_max = float(orc.pathloss_factor(np.array([max(d_min, 1.0)]))[0])
    f32_max = float(np.finfo(np.float32).max)
    for V, M in ROW_LANE_SHAPES:
        for E in (1, 64 // V + 1):
            th = _special_theta(E, M).astype(np.float64)
            assert np.isfinite(th).all()
            s = np.abs(th).sum(axis=(1, 2)).max()
            assert 2.0 * s * s < f32_max / 10                          # img.x^2 + img.y^2
            assert pl_max * 2.0 * s * s * snr_scale < f32_max / 10
            # and through the oracle: gains of these theta against the oracle's own h_r and b, one step
            rng = np.random.default_rng(E + M)
            pos = rng.uniform(0.0, 400.0, (E, V, 2))
            dist, _, h_r = orc.geometry(pos, M)
            gain = orc.gain_free(th[..., 0] + 1j * th[..., 1], h_r, orc.phase_R(M), dist)
            assert np.isfinite(gain).all() and gain.max() * snr_scale < f32_max / 10
            action = rng.uniform(0, 1, (E, 2, V))
            partner = np.full((E, V), -1, dtype=np.int32)
            out = orc.step(np.full((E, V), 5.0), np.zeros(E), gain, action, partner, np.full(E, V, dtype=np.int32),
                           np.ones((E, V), dtype=np.int32), p)
            for k, x in out.items():
                if isinstance(x, np.ndarray) and x.dtype.kind == "f":
                    assert np.isfinite(x).all(), (V, M, E, k)


def _state(E, V, M, source, heads, touch, positions, ones_b, seed):
    env = _env(E, V, M, seed=seed)
    env.Random_phase()
    _place(env, positions)
    t = env.tensors
    if source == "tensor":
        th = torch.from_numpy(_special_theta(E, M)).to(DEV)
        t["theta"].copy_(th.view_as(t["theta"]))           # a torch write: the step reads the complex64 theta
    else:
        g = torch.Generator(device=DEV); g.manual_seed(1000 * E + M)
        hit = torch.rand(E, M, device=DEV, generator=g) < 0.2
        t["theta_idx"][:, :M][hit] = 8                     # read by index in every run; the tensor is not consulted
    if ones_b:
        b = torch.zeros_like(t["b"]).view(-1, 2)
        b[:, 0] = 1.0
        t["b"].copy_(b.view_as(t["b"]))
    if not heads:
        env.steer_heads = False
    if touch:
        t["h_r"].mul_(1)                                   # ends the permission to rebuild: the reading form
    return env


def _marl_case(V, M, E, source, heads, positions, ones_b, what):
    N = _N()
    n_groups = (E + 64 // V - 1) // (64 // V)
    inp = _inputs(E, V, E + V + M)
    snaps = []
    for run, touch in (("read", True), ("gen/rule", False)):
        env = _state(E, V, M, source, heads, touch, positions, ones_b, seed=9)
        out = []
        with N.forced(lat=False, pipe_nt=False):
            for step in range(STEPS):
                env.step(*inp, fused=True, metrics=True, obs=True, power_w=True)
                _check_launch(N, V, M, source, heads, touch, None, n_groups, what + (run, step))
                out += [("%s@%d" % (k, step), env.tensors[k].clone()) for k in STEP_KEYS]
        if source == "tensor":
            assert bool(torch.isfinite(env.tensors["gain"]).all()), what
        snaps.append((run, out))
    _compare(snaps, what)


@pytest.mark.gpu
@pytest.mark.parametrize("heads", [True, False], ids=["heads", "sincospi"])
@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_marl_step_same_bits_on_zeros_subnormals_and_large_theta(V, M, size, source, heads):
    label, e_of = size
    _marl_case(V, M, e_of(64 // V), source, heads, "game", False, (V, M, label, source, heads))


@pytest.mark.gpu
@pytest.mark.parametrize("heads", [True, False], ids=["heads", "sincospi"])
@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_partials_that_cancel_exactly(V, M, heads):
    """b = 1 + 0j, vehicle 0 hand-placed at the RIS's x (a row of ones): in the envs of kind 3 the two products of every
    float4 are each other's negatives, so every partial of that row is a sum that cancels to zero"""
    _marl_case(V, M, 64 // V + 1, "tensor", heads, "hand", True, (V, M, "cancel", heads))


@pytest.mark.gpu
@pytest.mark.parametrize("heads", [True, False], ids=["heads", "sincospi"])
@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_ring_step_same_bits_on_zeros_subnormals_and_large_theta(V, M, size, source, heads):
    """the ring core's member through bind_step_store(fused=True): the env's tensors and the ring's seven arrays"""
    from ris_vec_marl_amd import VecReplayBuffer
    N = _N()
    label, e_of = size
    E = e_of(64 // V)
    n_groups = (E + 64 // V - 1) // (64 // V)
    g = torch.Generator(device=DEV); g.manual_seed(5)
    power = [torch.rand(E, V, 2, device=DEV, generator=g) * 2.4 - 1.2 for _ in range(STEPS)]
    probs = [torch.softmax(torch.randn(E, V, V, device=DEV, generator=g), -1) for _ in range(STEPS)]
    mask = (torch.rand(E, V, V, device=DEV, generator=g) < 0.6).to(torch.uint8)
    partner = torch.full((E, V), -1, dtype=torch.int32, device=DEV); partner[:, 0] = 1; partner[:, 1] = (1 << 16)
    ng = torch.full((E,), V - 1, dtype=torch.int32, device=DEV)
    snaps = []
    for run, touch in (("read", True), ("gen/rule", False)):
        env = _state(E, V, M, source, heads, touch, "game", False, seed=21)
        env.update_channel_gains()
        buf = VecReplayBuffer(max(E, (3 * E) // 2), 5, V + 2, V, device=DEV)
        pw, pr = torch.empty(E, V, 2, device=DEV), torch.empty(E, V, V, device=DEV)
        both = env.bind_step_store(buf, pw, partner, ng, pr, mask, fused=True, power_w=True)
        out = []
        with N.forced(pipe_nt=False):
            for step in range(STEPS):
                pw.copy_(power[step]); pr.copy_(probs[step])
                both(done=step == STEPS - 1, use_mask=step % 2 == 0)
                _check_launch(N, V, M, source, heads, touch, None, n_groups, (V, M, label, source, heads, run, step))
                assert N.last_kernel().endswith(",MarlCore+ring>")
                out += [("%s@%d" % (k, step), env.tensors[k].clone()) for k in STEP_KEYS]
        out += [(k, getattr(buf, k).clone()) for k in buf._ARRAYS]
        snaps.append((run, out))
    _compare(snaps, ("ring", V, M, label, source, heads))
