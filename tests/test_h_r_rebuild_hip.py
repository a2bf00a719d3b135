"""GPU tests of the fused step REBUILDING the h_r rows from their steering base (RISVEC_STEP_H_R_STEER_CURRENT,
k_step_fused_gen): after compute_parms() every row of h_r is a pure function of one float64 angle, `VecEnviron` tells the
fused step so while it knows that nothing else wrote the tensor, and the pipeline's GEN member then makes the rows with the
float64 operations k_geometry used instead of reading them.  Flag set against flag clear, everything a step writes must be
the same bits; no tolerance anywhere.  The reading side of every comparison is the same env after
`tensors["h_r"].mul_(1)`: an unannounced write through torch that changes no value and ends the permission."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.test_hip_parity import make_vec  # noqa: E402
from tests.test_theta_index_step_hip import DEV, _N, _env, _inputs, _same  # noqa: E402

GEN_SHAPES = [(4, 16), (8, 64), (16, 64), (16, 256)]
# (label, E as a function of EPW, pipe_waves): one wavefront with a partial group, with two groups and a tail, with four
# groups and a tail (the LDS stage is reused from pass to pass and from group to group), and the same split over two
SIZES = [("1", lambda epw: 1, 1), ("3", lambda epw: 3, 1), ("EPW+1/1wave", lambda epw: epw + 1, 1),
         ("EPW+1/2waves", lambda epw: epw + 1, 2), ("3EPW+1/1wave", lambda epw: 3 * epw + 1, 1),
         ("3EPW+1/2waves", lambda epw: 3 * epw + 1, 2)]


def _place(env, positions):
    """`game`: where make_new_game() and three renew_positions() leave the vehicles; `hand`: a vehicle at the RIS's x
    (angle exactly 0: a row of ones), vehicles at the field's four corners, the rest on a diagonal.  compute_parms()
    follows either."""
    if positions == "game":
        for _ in range(3):
            env.renew_positions()
    else:
        pos = env.tensors["pos"]
        E, V = pos.shape[0], pos.shape[1]
        spots = [(220.0, 37.5), (0.0, 0.0), (400.0, 0.0), (0.0, 400.0), (400.0, 400.0)]
        for v in range(V):
            x, y = spots[v % len(spots)] if v < len(spots) else (13.0 * v, 400.0 - 7.0 * v)
            pos[:, v, 0] = x
            pos[:, v, 1] = y
        pos[1::2, 0, 1] += 100.0                       # odd envs: another distance at the same x (still angle 0)
    env.compute_parms()


def _pair(E, V, M, source, positions, seed=9):
    """(gen, read): two envs in the same state; `read` has had its h_r touched through torch"""
    envs = []
    for touch in (False, True):
        env = _env(E, V, M, seed=seed)
        env.Random_phase()
        _place(env, positions)
        if source == "tensor":
            env.tensors["theta"].mul_(1)               # the step reads the complex64 theta
        if touch:
            env.tensors["h_r"].mul_(1)
        envs.append(env)
    for k in ("h_r", "steer_ang", "z_r", "theta", "theta_idx", "pl"):
        assert torch.equal(envs[0].tensors[k], envs[1].tensors[k]), k
    return envs


@pytest.mark.parametrize("positions", ["game", "hand"])
@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
@pytest.mark.parametrize("V,M", GEN_SHAPES)
def test_rebuilt_rows_give_the_reading_forms_bits(V, M, size, source, positions):
    N = _N()
    label, e_of, waves = size
    E = e_of(64 // V)
    gen, read = _pair(E, V, M, source, positions)
    inp = _inputs(E, V, E + V + M)
    with N.forced(lat=False, pipe_nt=False, pipe_waves=waves):
        for step in range(2):
            seen = []
            for env, want in ((gen, 1), (read, 0)):
                env.step(*inp, fused=True, metrics=True, obs=True, power_w=True)
                assert N.last_h_r_rebuilt() == want, (label, step, want)
                assert N.last_theta_by_index() == (1 if source == "index" else 0)
                assert N.last_pipe_walk() == step & 1                 # the walk is the pipeline's under either source
                seen.append(N.last_kernel())
            assert seen[0] == seen[1] and seen[0].startswith("k_step_fused_pipe<%d,%d," % (V, M)), seen
            _same(gen, read, (V, M, label, source, positions, step))


@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("V,M", GEN_SHAPES)
def test_ring_form_rebuilds_to_the_same_bits(V, M, source):
    """bind_step_store(fused=True), 3 EPW + 1 envs on two wavefronts, 4 steps through a ring wrap: env tensors and all
    seven ring arrays equal, flag set against flag clear."""
    from ris_vec_marl_amd import VecReplayBuffer
    N = _N()
    T = 4
    E = 3 * (64 // V) + 1
    g = torch.Generator(device=DEV); g.manual_seed(5)
    power = [torch.rand(E, V, 2, device=DEV, generator=g) * 2.4 - 1.2 for _ in range(T)]
    probs = [torch.softmax(torch.randn(E, V, V, device=DEV, generator=g), -1) for _ in range(T)]
    mask = (torch.rand(E, V, V, device=DEV, generator=g) < 0.6).to(torch.uint8)
    partner = torch.full((E, V), -1, dtype=torch.int32, device=DEV); partner[:, 0] = 1; partner[:, 1] = (1 << 16)
    ng = torch.full((E,), V - 1, dtype=torch.int32, device=DEV)
    runs = []
    for env, want in zip(_pair(E, V, M, source, "game", seed=21), (1, 0)):
        env.update_channel_gains()
        buf = VecReplayBuffer(int(2.5 * E), 5, V + 2, V, device=DEV)                     # wraps during step 3
        pw, pr = torch.empty(E, V, 2, device=DEV), torch.empty(E, V, V, device=DEV)
        both = env.bind_step_store(buf, pw, partner, ng, pr, mask, fused=True, power_w=True)
        with N.forced(pipe_nt=False, pipe_waves=2):
            for t in range(T):
                pw.copy_(power[t]); pr.copy_(probs[t])
                both(done=t == T - 1, use_mask=t % 2 == 0)
                assert N.last_kernel() == "k_step_fused_pipe<%d,%d,%d,MarlCore+ring>" % (V, M, 4 if (V, M) == (4, 16) else 2)
                assert N.last_h_r_rebuilt() == want
        runs.append((env, buf))
    _same(runs[0][0], runs[1][0], ("ring", V, M, source))
    for k in runs[0][1]._ARRAYS:
        assert torch.equal(getattr(runs[0][1], k), getattr(runs[1][1], k)), (V, M, source, k)


def _sent(env, inp):
    N = _N()
    with N.forced(lat=False, pipe_nt=False):
        env.step(*inp, fused=True)
    return N.last_h_r_rebuilt()


def test_when_the_flag_is_sent():
    V, M = 8, 64
    E = 64 // V + 1
    env = _env(E, V, M)
    env.Random_phase()
    inp = _inputs(E, V, 3)
    assert _sent(env, inp) == 1                                    # after compute_parms()
    env.tensors["h_r"].mul_(1)                                     # an unannounced write
    assert _sent(env, inp) == 0
    env.compute_parms()
    assert _sent(env, inp) == 1
    torch.view_as_complex(env.tensors["h_r"]).mul_(1)              # ... through the complex view
    assert _sent(env, inp) == 0
    env.compute_parms()
    env.invalidate_colsum()                                        # an announced one
    assert _sent(env, inp) == 0
    env.compute_parms()
    env.rebuild_colsum()
    assert _sent(env, inp) == 0
    env.compute_parms()
    sd = env.state_dict()
    env.load_state_dict(sd)                                        # a checkpoint with steer_ang keeps the permission
    assert _sent(env, inp) == 1
    old = {k: v for k, v in sd.items() if k != "steer_ang"}
    env.load_state_dict(old)                                       # one without: invalid until the next compute_parms()
    assert _sent(env, inp) == 0
    env.compute_parms()
    assert _sent(env, inp) == 1
    env.channel_model = "3gpp_umi"                                 # the RIS is not in the gain: nothing to rebuild
    assert _sent(env, inp) == 0
    env.channel_model = "free"
    assert _sent(env, inp) == 1
    with _N().forced(lat=False, pipe_nt=False):                    # steer=True is untouched: its own kernel, no rebuild
        env.step(*inp, fused=True, steer=True)
    assert _N().last_kernel().startswith("k_step_steer<") and _N().last_h_r_rebuilt() == 0


def test_moved_vehicles_without_compute_parms_keep_the_rows():
    """renew_positions() moves `pos` and nothing else: h_r and steer_ang are both of the last compute_parms(), so the flag
    stays and the outputs stay the reading form's."""
    N = _N()
    V, M = 8, 64
    E = 3 * (64 // V) + 1
    gen, read = _pair(E, V, M, "index", "game")
    inp = _inputs(E, V, 4)
    for env in (gen, read):
        env.renew_positions()
    with N.forced(lat=False, pipe_nt=False, pipe_waves=1):
        for env, want in ((gen, 1), (read, 0)):
            env.step(*inp, fused=True, metrics=True, obs=True, power_w=True)
            assert N.last_h_r_rebuilt() == want
    _same(gen, read, "moved")


@pytest.mark.parametrize("positions", ["game", "hand"])
@pytest.mark.parametrize("V", [4, 8, 16])
@pytest.mark.parametrize("M", [16, 64, 256])
def test_rows_from_steer_are_the_rows_compute_parms_wrote(V, M, positions):
    """risvec_h_r_from_steer runs the shared chunk routine from steer_ang / z_r: a contraction that differs between the
    two inlined copies shows here first, and by name."""
    N = _N()
    E = 5
    env = make_vec(E, V, M, seed=13)
    env.make_new_game()
    _place(env, positions)
    t = env.tensors
    out = torch.full_like(t["h_r"], float("nan"))
    N.check(N.load().risvec_h_r_from_steer(C.byref(env._cstate), out.data_ptr(), N.stream(env.device)))
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), t["h_r"].view(torch.int32)), (V, M, positions)
    assert torch.equal(t["steer_ang"].to(torch.float32), t["ang_r"])
    if positions == "hand":
        assert bool((t["steer_ang"][:, 0] == 0).all()) and bool((t["h_r"][:, 0, :, 0] == 1).all())
