"""GPU tests of the row-per-lane form of the fused step's one-group GEN member (k_step_fused_gen<..., ONE>): the lane that
rebuilds a row also consumes it and adds the row's 32-odd partials in registers, in the order the reading form's treduce
adds them across lanes.  GEN as the rule deals it at these sizes (one group per wavefront: the form under test) against two
references that keep the cross-lane order -- the reading form (h_r touched through torch, so the flag is not sent) and,
where there are four groups, GEN forced onto 2 wavefronts (the loop form, which keeps the LDS stage and treduce).  Every
tensor a step writes must hold the same bits after each of two consecutive steps; no tolerance anywhere.

The inputs are those at which a wrong association or a wrong pairing changes a bit:
  * tensor source: theta of magnitudes spread over 1e-4 ... 1e4 per element, so that almost every add of the tree rounds
    and no two orders agree by luck; theta zero on one whole chunk of some envs (partials that are exact zeros) and on
    one whole env;
  * index source: candidate 8 (the zero entry of the table) on scattered elements;
  * hand-placed positions with a vehicle at the RIS's x: angle 0, a row of ones.
The sign of a zero sum cannot reach an output (gain squares it) and is not tested."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.test_h_r_rebuild_hip import _place  # noqa: E402
from tests.test_theta_index_step_hip import DEV, STEP_KEYS, _N, _env, _inputs  # noqa: E402

# the shapes whose ONE member is the row-per-lane form (GenRowLane, k_step_gen.hip); 16 x 256 keeps the stage form
ROW_LANE_SHAPES = [(8, 64), (4, 16), (16, 64)]
# E as a function of EPW = 64 / V: a partial group, a group less one env, two groups, four groups (the last of one env)
SIZES = [("1", lambda epw: 1), ("EPW-1", lambda epw: epw - 1), ("EPW+1", lambda epw: epw + 1),
         ("3EPW+1", lambda epw: 3 * epw + 1)]
STEPS = 2


def _bits(t):
    return t.contiguous().view(torch.int32) if t.element_size() == 4 else t


def _hard_theta(env, E, M, source):
    """theta after Random_phase(), made hard for the tree (see the module's docstring); the same for every run of a case"""
    t = env.tensors
    g = torch.Generator(device=DEV); g.manual_seed(1000 * E + M)
    if source == "tensor":
        mag = torch.pow(10.0, torch.rand(E, M, 1, device=DEV, generator=g) * 8.0 - 4.0)
        th = torch.randn(E, M, 2, device=DEV, generator=g) * mag
        nch = M // 16
        if nch > 1:
            th[0::3, 16 * (nch - 1):16 * nch] = 0.0        # one whole chunk of envs 0, 3, ...
        th[1::3] = 0.0                                     # envs 1, 4, ...: all of theta
        t["theta"].copy_(th.view_as(t["theta"]))           # a torch write: the step reads the complex64 theta
    else:
        hit = torch.rand(E, M, device=DEV, generator=g) < 0.2
        idx = t["theta_idx"]
        idx[:, :M][hit] = 8                                # read by index in every run; the tensor is not consulted
    return env


def _state(E, V, M, source, heads, touch, positions, seed):
    env = _env(E, V, M, seed=seed)
    env.Random_phase()
    _place(env, positions)
    _hard_theta(env, E, M, source)
    if not heads:
        env.steer_heads = False
    if touch:
        env.tensors["h_r"].mul_(1)                         # ends the permission to rebuild: the reading form
    return env


# (label, h_r touched, forced pipe_waves or None = by rule)
def _runs(n_groups):
    runs = [("read", True, None), ("gen/rule", False, None)]
    if n_groups == 4:
        runs.append(("gen/2waves", False, 2))
    return runs


def _check_launch(N, V, M, source, heads, touch, waves, n_groups, what):
    assert N.last_h_r_rebuilt() == (0 if touch else 1), what
    assert N.last_h_r_heads() == (1 if heads and not touch else 0), what
    want = 0 if touch else (1 if waves is None else (n_groups + waves - 1) // waves)
    assert N.last_gen_groups_per_wave() == want, what
    assert N.last_theta_by_index() == (1 if source == "index" else 0), what
    assert N.last_kernel().startswith("k_step_fused_pipe<%d,%d," % (V, M)), what


def _compare(snaps, what):
    ref_label, ref = snaps[0]
    for label, got in snaps[1:]:
        assert len(got) == len(ref)
        for (k, a), (k2, b) in zip(ref, got):
            assert k == k2 and torch.equal(_bits(a), _bits(b)), (what, ref_label, label, k)


def _marl_case(V, M, E, source, heads, positions, what):
    N = _N()
    epw = 64 // V
    n_groups = (E + epw - 1) // epw
    inp = _inputs(E, V, E + V + M)
    snaps = []
    for run, touch, waves in _runs(n_groups):
        env = _state(E, V, M, source, heads, touch, positions, seed=9)
        force = {} if waves is None else {"pipe_waves": waves}
        out = []
        with N.forced(lat=False, pipe_nt=False, **force):
            for step in range(STEPS):
                env.step(*inp, fused=True, metrics=True, obs=True, power_w=True)
                _check_launch(N, V, M, source, heads, touch, waves, n_groups, what + (run, step))
                assert N.last_pipe_walk() == step & 1
                out += [("%s@%d" % (k, step), env.tensors[k].clone()) for k in STEP_KEYS]
        snaps.append((run, out))
    _compare(snaps, what)


@pytest.mark.parametrize("heads", [True, False], ids=["heads", "sincospi"])
@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_marl_step_same_bits_as_the_cross_lane_forms(V, M, size, source, heads):
    label, e_of = size
    _marl_case(V, M, e_of(64 // V), source, heads, "game", (V, M, label, source, heads))


@pytest.mark.parametrize("heads", [True, False], ids=["heads", "sincospi"])
@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_rows_of_ones_same_bits_as_the_cross_lane_forms(V, M, source, heads):
    """hand-placed vehicles: vehicle 0 at the RIS's x (angle exactly 0, every element of its row 1 + 0j), the field's four
    corners, a diagonal; two groups, the second ragged"""
    _marl_case(V, M, 64 // V + 1, source, heads, "hand", (V, M, "hand", source, heads))


@pytest.mark.parametrize("heads", [True, False], ids=["heads", "sincospi"])
@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_ring_step_same_bits_as_the_cross_lane_forms(V, M, size, source, heads):
    """bind_step_store(fused=True): the env's tensors and the ring's seven arrays; the ring holds 1.5 E rows, so the second
    step's rows wrap."""
    from ris_vec_marl_amd import VecReplayBuffer
    N = _N()
    label, e_of = size
    epw = 64 // V
    E = e_of(epw)
    n_groups = (E + epw - 1) // epw
    g = torch.Generator(device=DEV); g.manual_seed(5)
    power = [torch.rand(E, V, 2, device=DEV, generator=g) * 2.4 - 1.2 for _ in range(STEPS)]
    probs = [torch.softmax(torch.randn(E, V, V, device=DEV, generator=g), -1) for _ in range(STEPS)]
    mask = (torch.rand(E, V, V, device=DEV, generator=g) < 0.6).to(torch.uint8)
    partner = torch.full((E, V), -1, dtype=torch.int32, device=DEV); partner[:, 0] = 1; partner[:, 1] = (1 << 16)
    ng = torch.full((E,), V - 1, dtype=torch.int32, device=DEV)
    snaps = []
    for run, touch, waves in _runs(n_groups):
        env = _state(E, V, M, source, heads, touch, "game", seed=21)
        env.update_channel_gains()
        buf = VecReplayBuffer(max(E, (3 * E) // 2), 5, V + 2, V, device=DEV)
        pw, pr = torch.empty(E, V, 2, device=DEV), torch.empty(E, V, V, device=DEV)
        both = env.bind_step_store(buf, pw, partner, ng, pr, mask, fused=True, power_w=True)
        force = {} if waves is None else {"pipe_waves": waves}
        out = []
        with N.forced(pipe_nt=False, **force):
            for step in range(STEPS):
                pw.copy_(power[step]); pr.copy_(probs[step])
                both(done=step == STEPS - 1, use_mask=step % 2 == 0)
                _check_launch(N, V, M, source, heads, touch, waves, n_groups, (V, M, label, source, heads, run, step))
                assert N.last_kernel().endswith(",MarlCore+ring>")
                out += [("%s@%d" % (k, step), env.tensors[k].clone()) for k in STEP_KEYS]
        out += [(k, getattr(buf, k).clone()) for k in buf._ARRAYS]
        assert len(buf._ARRAYS) == 7
        snaps.append((run, out))
    _compare(snaps, ("ring", V, M, label, source, heads))
