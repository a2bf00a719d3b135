"""GPU tests of the GEN members READING the head of every 16-element chunk (RISVEC_STEP_STEER_HEADS_CURRENT,
k_step_fused_gen<.., HD>): compute_parms() leaves exp(-j pi ang 16 c) in float64 behind the angles
(`tensors["steer_head"]`, risvec_steer_heads), `VecEnviron` says so while the angles have not moved, and the kernel starts
each chunk's rotations from the stored pair instead of from sincospi.  The same float64 pair either way: heads member,
sincospi member and reading form must write the same bits everywhere.  No tolerance anywhere."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.test_h_r_rebuild_hip import GEN_SHAPES, _place  # noqa: E402
from tests.test_hip_parity import make_vec  # noqa: E402
from tests.test_theta_index_step_hip import DEV, _N, _env, _inputs, _same  # noqa: E402


# ---------------------------------------------------------------------------- 1. the heads are the rows' own
@pytest.mark.parametrize("positions", ["game", "hand"])
@pytest.mark.parametrize("V", [4, 8, 16])
@pytest.mark.parametrize("M", [16, 64, 256])
def test_heads_are_the_first_element_of_every_chunk(V, M, positions):
    """h_r[e,v,16c] is the head rounded once to float32; the m0 = 0 head is exactly 1 - j sin(pi ang 0) = (1, -/+0) for
    ang >= 0 / ang < 0.  `hand` has a vehicle at the RIS's x (angle exactly 0) and angles of both signs."""
    E = 5
    env = make_vec(E, V, M, seed=13)
    env.make_new_game()
    _place(env, positions)
    t = env.tensors
    head, ang = t["steer_head"], t["steer_ang"]
    assert tuple(head.shape) == (E, V, M // 16, 2) and head.dtype == torch.float64 and head.data_ptr() % 16 == 0
    assert head.data_ptr() == ang.data_ptr() + 8 * E * V          # directly behind the angles
    got = head.to(torch.float32).contiguous().view(torch.int32)
    want = t["h_r"][:, :, ::16, :].contiguous().view(torch.int32)
    assert torch.equal(got, want), (V, M, positions)
    assert bool((head[:, :, 0, 0] == 1).all()) and bool((head[:, :, 0, 1] == 0).all())
    assert torch.equal(torch.signbit(head[:, :, 0, 1]), ~torch.signbit(ang))
    if positions == "hand":
        assert bool((ang[:, 0] == 0).all()) and bool((ang > 0).any()) and bool((ang < 0).any())


# ---------------------------------------------------------------------------- 2. three members, bit for bit
def _trio(E, V, M, source, seed=9):
    """(heads, sincospi, read): three envs in the same state.  `sincospi` does not send the heads bit, `read` has had its
    h_r touched through torch (an unannounced write that changes no value)."""
    envs = []
    for kind in ("heads", "sincospi", "read"):
        env = _env(E, V, M, seed=seed)
        env.Random_phase()
        _place(env, "game")
        if source == "tensor":
            env.tensors["theta"].mul_(1)               # the step reads the complex64 theta
        if kind == "sincospi":
            env.steer_heads = False
        if kind == "read":
            env.tensors["h_r"].mul_(1)
        envs.append(env)
    for k in ("h_r", "steer_ang", "steer_head", "z_r", "theta", "theta_idx", "pl"):
        assert torch.equal(envs[0].tensors[k], envs[1].tensors[k]) and torch.equal(envs[0].tensors[k], envs[2].tensors[k]), k
    return envs


WANT = ((1, 1), (1, 0), (0, 0))                        # (rebuilt, heads) of the three
SIZES = [("1", lambda epw: 1), ("EPW-1", lambda epw: epw - 1), ("EPW+1", lambda epw: epw + 1),
         ("3EPW+1", lambda epw: 3 * epw + 1)]


@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
@pytest.mark.parametrize("V,M", GEN_SHAPES)
def test_heads_sincospi_and_reading_members_agree(V, M, size, source):
    """By rule (one group per wavefront: the ONE form) and with the pipeline forced onto 1 and 2 wavefronts (the loop form
    wherever there are more groups than that), two consecutive steps each: both walks."""
    N = _N()
    label, e_of = size
    E = e_of(64 // V)
    envs = _trio(E, V, M, source)
    inp = _inputs(E, V, E + V + M)
    step = 0
    for waves in (0, 1, 2):
        n_groups = (E + 64 // V - 1) // (64 // V)
        per_wave = 1 if waves == 0 else (n_groups + min(waves, n_groups) - 1) // min(waves, n_groups)
        with N.forced(lat=False, pipe_nt=False, pipe_waves=waves):
            for _ in range(2):
                seen = []
                for env, (rebuilt, heads) in zip(envs, WANT):
                    env.step(*inp, fused=True, metrics=True, obs=True, power_w=True)
                    what = (label, waves, step, rebuilt, heads)
                    assert (N.last_h_r_rebuilt(), N.last_h_r_heads()) == (rebuilt, heads), what
                    assert N.last_gen_groups_per_wave() == (per_wave if rebuilt else 0), what
                    assert N.last_theta_by_index() == (1 if source == "index" else 0), what
                    assert N.last_pipe_walk() == step & 1, what
                    seen.append(N.last_kernel())
                assert seen[0] == seen[1] == seen[2] and seen[0].startswith("k_step_fused_pipe<%d,%d," % (V, M)), seen
                _same(envs[0], envs[1], (V, M, label, source, waves, step, "heads / sincospi"))
                _same(envs[0], envs[2], (V, M, label, source, waves, step, "heads / read"))
                step += 1


@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("V,M", GEN_SHAPES)
def test_ring_form_reads_heads_to_the_same_bits(V, M, source):
    """bind_step_store(fused=True), 3 EPW + 1 envs on two wavefronts, 4 steps through a ring wrap: env tensors and all
    seven ring arrays equal among the three members."""
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
    for env, want in zip(_trio(E, V, M, source, seed=21), WANT):
        env.update_channel_gains()
        buf = VecReplayBuffer(int(2.5 * E), 5, V + 2, V, device=DEV)                     # wraps during step 3
        pw, pr = torch.empty(E, V, 2, device=DEV), torch.empty(E, V, V, device=DEV)
        both = env.bind_step_store(buf, pw, partner, ng, pr, mask, fused=True, power_w=True)
        with N.forced(pipe_nt=False, pipe_waves=2):
            for t in range(T):
                pw.copy_(power[t]); pr.copy_(probs[t])
                both(done=t == T - 1, use_mask=t % 2 == 0)
                assert N.last_kernel() == "k_step_fused_pipe<%d,%d,%d,MarlCore+ring>" % (V, M, 4 if (V, M) == (4, 16) else 2)
                assert (N.last_h_r_rebuilt(), N.last_h_r_heads()) == want
        runs.append((env, buf))
    for other in (1, 2):
        _same(runs[0][0], runs[other][0], ("ring", V, M, source, other))
        for k in runs[0][1]._ARRAYS:
            assert torch.equal(getattr(runs[0][1], k), getattr(runs[other][1], k)), (V, M, source, other, k)


# ---------------------------------------------------------------------------- 3. when the bit is sent
def _sent(env, inp):
    N = _N()
    with N.forced(lat=False, pipe_nt=False):
        env.step(*inp, fused=True)
    return N.last_h_r_rebuilt(), N.last_h_r_heads()


def test_when_the_bit_is_sent():
    V, M = 8, 64
    E = 64 // V + 1
    env = _env(E, V, M)
    env.Random_phase()
    inp = _inputs(E, V, 3)
    assert _sent(env, inp) == (1, 1)                               # after compute_parms()
    env.tensors["steer_ang"].mul_(1)                               # a torch write to the angles: the heads may be stale
    assert _sent(env, inp) == (1, 0)                               # ... and the GEN bit's own rule is untouched
    env.compute_parms()
    assert _sent(env, inp) == (1, 1)
    sd = env.state_dict()
    assert "steer_head" not in sd                                  # a function of steer_ang: not part of a checkpoint
    before = env.tensors["steer_head"].clone()
    env.tensors["steer_head"].fill_(float("nan"))
    env.load_state_dict(sd)                                        # a checkpoint with steer_ang: heads recomputed
    assert torch.equal(env.tensors["steer_head"].view(torch.int64), before.view(torch.int64))
    assert _sent(env, inp) == (1, 1)
    env.load_state_dict({k: v for k, v in sd.items() if k != "steer_ang"})
    assert _sent(env, inp) == (0, 0)                               # one without: neither bit until the next compute_parms()
    env.compute_parms()
    assert _sent(env, inp) == (1, 1)
    env.steer_heads = False
    assert _sent(env, inp) == (1, 0)
