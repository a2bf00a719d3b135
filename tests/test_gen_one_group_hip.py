"""GPU tests of the two forms of the fused step's GEN member (k_step_fused_gen): the one-group form the launcher picks when
every wavefront owns one group of 64 rows, and the loop form for more.  Both read step()'s arguments from the
kernel-argument segment after the last pass.  Three runs from the same state -- the reading form (h_r touched through
torch, so the flag is not sent), GEN as the rule deals it (one group per wavefront at these sizes) and GEN on one or two
forced wavefronts (several groups each) -- must leave the same bits in everything a step writes, two steps in a row (both
walks); risvec_last_gen_groups_per_wave() says which form ran.  No tolerance anywhere."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.test_h_r_rebuild_hip import _place  # noqa: E402
from tests.test_theta_index_step_hip import DEV, STEP_KEYS, _N, _env, _inputs  # noqa: E402

GEN_SHAPES = [(8, 64), (4, 16), (16, 64), (16, 256)]
# E as a function of EPW = 64 / V: a partial group, a group less one env, two groups, four groups (the last of one env)
SIZES = [("1", lambda epw: 1), ("EPW-1", lambda epw: epw - 1), ("EPW+1", lambda epw: epw + 1),
         ("3EPW+1", lambda epw: 3 * epw + 1)]
STEPS = 2


def _bits(t):
    return t.contiguous().view(torch.int32) if t.element_size() == 4 else t


def _state(E, V, M, source, touch, seed):
    """an env after compute_parms(); touch: h_r written through torch (same values), which ends the permission to rebuild"""
    env = _env(E, V, M, seed=seed)
    env.Random_phase()
    _place(env, "game")
    if source == "tensor":
        env.tensors["theta"].mul_(1)                   # the step reads the complex64 theta
    if touch:
        env.tensors["h_r"].mul_(1)
    return env


# (label, h_r touched, forced pipe_waves or None = by rule)
def _runs(n_groups):
    runs = [("read", True, None), ("gen/rule", False, None)]
    if n_groups == 4:
        runs += [("gen/1wave", False, 1), ("gen/2waves", False, 2)]
    return runs


def _want_groups_per_wave(touch, waves, n_groups):
    if touch:
        return 0
    return 1 if waves is None else (n_groups + waves - 1) // waves


def _check_launch(N, V, M, source, touch, waves, n_groups, what):
    assert N.last_h_r_rebuilt() == (0 if touch else 1), what
    assert N.last_gen_groups_per_wave() == _want_groups_per_wave(touch, waves, n_groups), what
    assert N.last_theta_by_index() == (1 if source == "index" else 0), what
    assert N.last_kernel().startswith("k_step_fused_pipe<%d,%d," % (V, M)), what


def _compare(snaps, what):
    ref_label, ref = snaps[0]
    for label, got in snaps[1:]:
        assert len(got) == len(ref)
        for (k, a), (k2, b) in zip(ref, got):
            assert k == k2 and torch.equal(_bits(a), _bits(b)), (what, ref_label, label, k)


@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
@pytest.mark.parametrize("V,M", GEN_SHAPES)
def test_marl_step_same_bits_in_every_form(V, M, size, source):
    N = _N()
    label, e_of = size
    epw = 64 // V
    E = e_of(epw)
    n_groups = (E + epw - 1) // epw
    inp = _inputs(E, V, E + V + M)
    snaps = []
    for run, touch, waves in _runs(n_groups):
        env = _state(E, V, M, source, touch, seed=9)
        force = {} if waves is None else {"pipe_waves": waves}
        out = []
        with N.forced(lat=False, pipe_nt=False, **force):
            for step in range(STEPS):
                env.step(*inp, fused=True, metrics=True, obs=True, power_w=True)
                _check_launch(N, V, M, source, touch, waves, n_groups, (V, M, label, source, run, step))
                assert N.last_pipe_walk() == step & 1
                out += [("%s@%d" % (k, step), env.tensors[k].clone()) for k in STEP_KEYS]
        snaps.append((run, out))
    _compare(snaps, (V, M, label, source))


@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
@pytest.mark.parametrize("V,M", GEN_SHAPES)
def test_ring_step_same_bits_in_every_form(V, M, size, source):
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
        env = _state(E, V, M, source, touch, seed=21)
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
                _check_launch(N, V, M, source, touch, waves, n_groups, (V, M, label, source, run, step))
                assert N.last_kernel().endswith(",MarlCore+ring>")
                out += [("%s@%d" % (k, step), env.tensors[k].clone()) for k in STEP_KEYS]
        out += [(k, getattr(buf, k).clone()) for k in buf._ARRAYS]
        assert len(buf._ARRAYS) == 7
        snaps.append((run, out))
    _compare(snaps, ("ring", V, M, label, source))


def test_accessor_is_zero_after_a_launch_that_is_no_gen_member():
    N = _N()
    V, M = 8, 64
    E = 64 // V + 1
    env = _state(E, V, M, "index", False, seed=9)
    inp = _inputs(E, V, 3)
    with N.forced(lat=False, pipe_nt=False):
        env.step(*inp, fused=True)
    assert N.last_h_r_rebuilt() == 1 and N.last_gen_groups_per_wave() == 1
    env.update_channel_gains()
    env.step(*inp, fused=False)                                    # the cached-gain step
    assert N.last_kernel().startswith("k_step<") and N.last_gen_groups_per_wave() == 0
    with N.forced(lat=False, pipe_nt=False, pipe_waves=1):
        env.step(*inp, fused=True)
    assert N.last_gen_groups_per_wave() == 2
    env.step(*inp, fused=True)                                     # by rule at this size: the latency family
    assert N.last_kernel().startswith("k_step_fused_lat<") and N.last_gen_groups_per_wave() == 0
