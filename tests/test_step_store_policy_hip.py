"""GPU tests of how the GEN members of the fused step write step()'s outputs (StorePolicy, risvec_step.hpp: the kind of
store is a compile-time policy of the kernel, and the GEN family has its own).  Whatever the kind, what the launch wrote
must be what everyone downstream sees: the next launch (data_buf / mec_q carried from step to step), the host (`.cpu()`
right behind the launch), a torch kernel on another stream behind an event, and the cached step reading `gain`.  The
reference of every comparison is the reading form of the pipeline (h_r touched through torch), whose stores are plain;
every tensor a step writes must hold the same bits.  No tolerance anywhere."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.test_gen_row_lane_hip import _bits, _state  # noqa: E402
from tests.test_theta_index_step_hip import DEV, STEP_KEYS, _N, _inputs  # noqa: E402

# every shape with GEN members: the three row-per-lane ones and 16 x 256 (stage form)
GEN_SHAPES = [(8, 64), (4, 16), (16, 64), (16, 256)]
STEPS = 3


def _e(V):
    return 3 * (64 // V) + 1          # four groups, the last of one env


def _step(env, inp):
    env.step(*inp, fused=True, metrics=True, obs=True, power_w=True)


def _snap(env):
    return [(k, env.tensors[k].clone()) for k in STEP_KEYS]


def _equal(ref, got, what):
    assert len(ref) == len(got)
    for (k, a), (k2, b) in zip(ref, got):
        assert k == k2 and torch.equal(_bits(a), _bits(b)), (what, k)


def _reading_steps(V, M, E, inp, source="index"):
    """the reading form's outputs after each of STEPS steps"""
    N = _N()
    env = _state(E, V, M, source, True, True, "game", seed=9)
    out = []
    with N.forced(lat=False, pipe_nt=False):
        for _ in range(STEPS):
            _step(env, inp)
            assert N.last_h_r_rebuilt() == 0
            out.append(_snap(env))
    return out


# ---------------------------------------------------------------------------- (a) the next launch
@pytest.mark.parametrize("waves", [None, 2], ids=["rule", "2waves"])
@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("V,M", GEN_SHAPES)
def test_three_steps_carry_the_queues_from_launch_to_launch(V, M, source, waves):
    """data_buf and mec_q written by one GEN launch are read by the next: three steps, one group per wavefront (by rule) and
    the loop form on two wavefronts, against three steps of the reading form."""
    N = _N()
    E = _e(V)
    inp = _inputs(E, V, E + V + M)
    ref = _reading_steps(V, M, E, inp, source)
    env = _state(E, V, M, source, True, False, "game", seed=9)
    force = {} if waves is None else {"pipe_waves": waves}
    with N.forced(lat=False, pipe_nt=False, **force):
        for step in range(STEPS):
            _step(env, inp)
            assert N.last_h_r_rebuilt() == 1 and N.last_gen_groups_per_wave() == (1 if waves is None else 2)
            _equal(ref[step], _snap(env), (V, M, source, waves, step))


@pytest.mark.parametrize("V,M", GEN_SHAPES)
def test_three_ring_steps_carry_the_queues_from_launch_to_launch(V, M):
    """the same through bind_step_store(fused=True): the ring core's member, env tensors and the ring's seven arrays"""
    from ris_vec_marl_amd import VecReplayBuffer
    N = _N()
    E = _e(V)
    g = torch.Generator(device=DEV); g.manual_seed(5)
    power = [torch.rand(E, V, 2, device=DEV, generator=g) * 2.4 - 1.2 for _ in range(STEPS)]
    probs = [torch.softmax(torch.randn(E, V, V, device=DEV, generator=g), -1) for _ in range(STEPS)]
    mask = (torch.rand(E, V, V, device=DEV, generator=g) < 0.6).to(torch.uint8)
    partner = torch.full((E, V), -1, dtype=torch.int32, device=DEV); partner[:, 0] = 1; partner[:, 1] = (1 << 16)
    ng = torch.full((E,), V - 1, dtype=torch.int32, device=DEV)
    snaps = []
    for touch in (True, False):
        env = _state(E, V, M, "index", True, touch, "game", seed=21)
        env.update_channel_gains()
        buf = VecReplayBuffer(2 * E, 5, V + 2, V, device=DEV)
        pw, pr = torch.empty(E, V, 2, device=DEV), torch.empty(E, V, V, device=DEV)
        both = env.bind_step_store(buf, pw, partner, ng, pr, mask, fused=True, power_w=True)
        out = []
        with N.forced(pipe_nt=False):
            for step in range(STEPS):
                pw.copy_(power[step]); pr.copy_(probs[step])
                both(done=step == STEPS - 1, use_mask=step % 2 == 0)
                assert N.last_h_r_rebuilt() == (0 if touch else 1)
                assert N.last_kernel().endswith(",MarlCore+ring>")
                out += [("%s@%d" % (k, step), env.tensors[k].clone()) for k in STEP_KEYS]
        out += [(k, getattr(buf, k).clone()) for k in buf._ARRAYS]
        snaps.append(out)
    _equal(snaps[0], snaps[1], ("ring", V, M))


# ---------------------------------------------------------------------------- (b) the host, (c) another stream
@pytest.mark.parametrize("V,M", GEN_SHAPES)
def test_outputs_as_the_host_reads_them_right_after_the_launch(V, M):
    """`.cpu()` of every output tensor behind the launch, nothing in between"""
    N = _N()
    E = _e(V)
    inp = _inputs(E, V, E + V + M)
    ref = _reading_steps(V, M, E, inp)[0]
    env = _state(E, V, M, "index", True, False, "game", seed=9)
    torch.cuda.synchronize()
    with N.forced(lat=False, pipe_nt=False):
        _step(env, inp)
        got = [(k, env.tensors[k].cpu()) for k in STEP_KEYS]
        assert N.last_h_r_rebuilt() == 1
    _equal([(k, t.cpu()) for k, t in ref], got, (V, M, "host"))


@pytest.mark.parametrize("V,M", GEN_SHAPES)
def test_outputs_as_a_kernel_on_another_stream_reads_them(V, M):
    """an event behind the launch, a second stream waits for it and copies every output with a torch kernel"""
    N = _N()
    E = _e(V)
    inp = _inputs(E, V, E + V + M)
    ref = _reading_steps(V, M, E, inp)[0]
    env = _state(E, V, M, "index", True, False, "game", seed=9)
    other = torch.cuda.Stream()
    torch.cuda.synchronize()
    with N.forced(lat=False, pipe_nt=False):
        _step(env, inp)
        assert N.last_h_r_rebuilt() == 1
    done = torch.cuda.Event()
    done.record()
    other.wait_event(done)
    with torch.cuda.stream(other):
        got = [(k, env.tensors[k] + 0) for k in STEP_KEYS]      # an elementwise kernel per tensor, not a copy engine
    other.synchronize()
    _equal(ref, got, (V, M, "stream"))


# ---------------------------------------------------------------------------- (d) the cached step on the gain it wrote
@pytest.mark.parametrize("V,M", GEN_SHAPES)
def test_cached_step_on_the_gain_the_gen_launch_wrote(V, M):
    """env B, in env A's state, steps on cached gains with the `gain` A's GEN launch left: B's outputs are A's"""
    N = _N()
    E = _e(V)
    inp = _inputs(E, V, E + V + M)
    a = _state(E, V, M, "index", True, False, "game", seed=9)
    b = _state(E, V, M, "index", True, False, "game", seed=9)
    b.tensors["gain"].zero_()
    with N.forced(lat=False, pipe_nt=False):
        _step(a, inp)
        assert N.last_h_r_rebuilt() == 1 and N.last_gen_groups_per_wave() == 1
    b.tensors["gain"].copy_(a.tensors["gain"])                  # read by a torch kernel right behind the launch
    b.step(*inp, fused=False, metrics=True, obs=True, power_w=True)
    _equal(_snap(a), _snap(b), (V, M, "cached"))
