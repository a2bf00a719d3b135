"""GPU tests of the fused step reading theta as candidate indices inside the software pipeline
(RISVEC_STEP_THETA_IDX_CURRENT): `Random_phase` leaves the index of every element next to the tensor, `VecEnviron` tells
the fused step so while it knows the two match, and k_step_fused_pipe then reads one byte per element instead of eight.
The two sources must give the same bits everywhere, and every theta write that bypasses the indices must make the very
next step read the tensor again."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.test_hip_parity import make_vec, random_step_inputs  # noqa: E402

DEV = "cuda:0"
FIXED_SHAPES = [(8, 64), (8, 36), (8, 40), (4, 16), (16, 64), (16, 256)]
STEP_KEYS = ("gain", "reward", "data_buf", "mec_q", "rate", "data_t", "data_p", "over_power", "metrics", "obs", "power_w")


def _N():
    from ris_vec_marl_amd import _native as N
    return N


def _env(E, V, M, b=3, seed=9):
    env = make_vec(E, V, M, b=b, seed=seed, yaml=True)
    env.make_new_game(); env.renew_positions(); env.compute_parms()
    return env


def _inputs(E, V, seed):
    """step inputs for E envs on the device: 64 random envs' worth (pairs, singles, dropped vehicles), tiled"""
    rng = np.random.default_rng(seed)
    action, partner, ng, arrivals = random_step_inputs(64, V, rng)
    rep = (E + 63) // 64
    tile = lambda x, dt: torch.from_numpy(np.concatenate([x] * rep)[:E].astype(dt)).to(DEV)   # noqa: E731
    return tile(action, np.float32), tile(partner, np.int32), tile(ng, np.int32), tile(arrivals, np.int32)


def _bits(theta):
    return theta.contiguous().view(torch.int32)


def _same(a, b, what):
    for k in STEP_KEYS:
        assert torch.equal(a.tensors[k], b.tensors[k]), (what, k)


def _fused_steps(env, inp, n=3):
    """n fused steps with metrics, obs and power_w on -> (query, kernel name) of each"""
    N = _N()
    seen = []
    for _ in range(n):
        env.step(*inp, fused=True, metrics=True, obs=True, power_w=True)
        seen.append((N.last_theta_by_index(), N.last_kernel()))
    return seen


# ---------------------------------------------------------------------------- 1. Random_phase writes the indices
@pytest.mark.parametrize("V,M", [(8, 64), (8, 36), (4, 16), (16, 64)])
@pytest.mark.parametrize("inject", [False, True])
def test_random_phase_writes_the_indices_of_what_it_wrote(V, M, inject):
    """theta_idx after Random_phase expands (risvec_theta_from_index: the by-index table's entries) to the tensor
    Random_phase wrote, as int32 bit patterns -- signs of zero included."""
    N = _N()
    E = 130
    env = _env(E, V, M)
    idx = torch.randint(0, 8, (E, M), dtype=torch.int32, device=DEV, generator=torch.Generator(DEV).manual_seed(V + M))
    env.Random_phase(idx if inject else None)
    t = env.tensors
    wrote = t["theta"].clone()
    ti = t["theta_idx"][:, :M]
    assert int(ti.max()) <= 7 and len(torch.unique(ti)) == 8
    if inject:
        assert torch.equal(ti.to(torch.int32), idx)
    t["theta"].zero_()
    N.check(N.load().risvec_theta_from_index(C.byref(env._cstate), N.stream(env.device)))
    assert torch.equal(_bits(t["theta"]), _bits(wrote))
    assert env._idx_current


def test_other_control_bits_write_no_indices_and_never_send_the_bit():
    N = _N()
    E, V, M = 130, 8, 64
    env = _env(E, V, M, b=2)
    env.tensors["theta_idx"].fill_(77)
    env.Random_phase()
    assert bool((env.tensors["theta_idx"] == 77).all()) and not env._idx_current
    with N.forced(lat=False):
        seen = _fused_steps(env, _inputs(E, V, 1), n=1)
    assert seen == [(0, "k_step_fused_pipe<8,64,2,MarlCore>")], seen


# ---------------------------------------------------------------------------- 2. the two sources, bit for bit
def _two_sources(E, V, M, prepare=None):
    """env A steps with current indices, env B (same seed) after `tensors["theta"].mul_(1)`: an unannounced write through
    torch that changes no value, so B reads the tensor.  Three fused steps each; everything a step writes must be equal."""
    N = _N()
    inp = _inputs(E, V, E + V + M)
    envs = []
    for touch in (False, True):
        env = _env(E, V, M)
        env.Random_phase()
        if prepare:
            prepare(env)
        if touch:
            env.tensors["theta"].mul_(1)
        envs.append(env)
    a, b = envs
    assert torch.equal(_bits(a.tensors["theta"]), _bits(b.tensors["theta"]))
    # pipe_nt=False: 16 x 256 at this batch size is past the Infinity Cache, where the rules take the NT pipeline (which
    # has no by-index copy); the forced plain pipeline is the kernel under test at every shape
    with N.forced(lat=False, pipe_nt=False):
        seen_a = _fused_steps(a, inp)
        seen_b = _fused_steps(b, inp)
    assert [q for q, _ in seen_a] == [1, 1, 1] and [q for q, _ in seen_b] == [0, 0, 0], (seen_a, seen_b)
    assert [n for _, n in seen_a] == [n for _, n in seen_b], (seen_a, seen_b)
    assert seen_a[0][1].startswith("k_step_fused_pipe<%d,%d," % (V, M)) and seen_a[0][1].endswith("MarlCore>"), seen_a
    _same(a, b, (E, V, M))
    return a, b


def _e_two_to_three_groups(V):
    """EPW * 8 * CUs * 2 + 3 * EPW + 1 envs: every wavefront of the pipeline owns 2-3 groups (the ring crosses group
    boundaries, the last group prefetches group 0) and the last group is ragged."""
    epw = 64 // V
    return epw * 8 * torch.cuda.get_device_properties(0).multi_processor_count * 2 + 3 * epw + 1


@pytest.mark.parametrize("V,M", FIXED_SHAPES)
@pytest.mark.parametrize("size", ["groups", "3", "EPW+1"])
def test_index_and_tensor_sources_are_bit_identical(V, M, size):
    E = {"groups": _e_two_to_three_groups(V), "3": 3, "EPW+1": 64 // V + 1}[size]
    _two_sources(E, V, M)


# ---------------------------------------------------------------------------- 3. indices left by a sweep
@pytest.mark.parametrize("V,M", [(8, 64), (16, 64)])
def test_indices_left_by_a_sweep(V, M):
    """A non-lazy optimize_phase_shift() writes the tensor and the indices: the fused step may read either."""
    a, b = _two_sources(515, V, M, prepare=lambda env: env.optimize_phase_shift())
    assert a._idx_current and not a.lazy_theta and not a._theta_stale


# ---------------------------------------------------------------------------- 4. invalidation
def _discrete_theta(E, M, seed):
    """an [E, M, 2] float32 theta of candidate phasors other than the env's (exact values: +-1, +-0.70710677, 0)"""
    k = torch.randint(0, 8, (E, M), device=DEV, generator=torch.Generator(DEV).manual_seed(seed))
    r = 0.70710677
    re = torch.tensor([1, r, 0, -r, -1, -r, 0, r], dtype=torch.float32, device=DEV)[k]
    im = torch.tensor([0, r, 1, r, 0, -r, -1, -r], dtype=torch.float32, device=DEV)[k]
    return torch.stack([re, im], -1).contiguous()


@pytest.mark.parametrize("how", ["copy_", "get_next_phase", "load_state_dict", "invalidate_theta", "invalidate_colsum"])
def test_theta_writes_drop_the_indices(how):
    """After each kind of theta write the next fused step reads the tensor (query 0) and its outputs are those of a fresh
    env that got the same theta through the announced route; a following Random_phase() restores the by-index read."""
    N = _N()
    E, V, M = 515, 8, 64
    inp = _inputs(E, V, 5)
    other = _discrete_theta(E, M, 3)
    angle = torch.rand(E, M, device=DEV, generator=torch.Generator(DEV).manual_seed(4)) * 6.0

    env = _env(E, V, M)
    env.Random_phase()
    fresh = _env(E, V, M)
    fresh.Random_phase()
    with N.forced(lat=False):
        assert _fused_steps(env, inp, n=1)[0][0] == 1
        assert _fused_steps(fresh, inp, n=1)[0][0] == 1
        if how == "copy_":                                     # unannounced: only the tensor's version tells
            env.tensors["theta"].copy_(other)
        elif how == "get_next_phase":
            env.get_next_phase(angle)
        elif how == "load_state_dict":
            sd = env.state_dict()
            sd["theta"] = other.cpu()
            env.load_state_dict(sd)
        else:                                                  # announced: written through `.data`, which has a version
            v0 = env._t["theta"]._version                      # counter of its own, so only the announcement tells
            env._t["theta"].data.copy_(other)
            assert env._t["theta"]._version == v0 and env._idx_current
            env.invalidate_theta() if how == "invalidate_theta" else env.invalidate_colsum()
        # the announced route into the fresh env
        if how == "get_next_phase":
            fresh.get_next_phase(angle)
        else:
            fresh.tensors["theta"].copy_(other)
            fresh.invalidate_theta()
        assert torch.equal(_bits(env.tensors["theta"]), _bits(fresh.tensors["theta"]))
        got = _fused_steps(env, inp, n=1)[0]
        want = _fused_steps(fresh, inp, n=1)[0]
        assert got[0] == 0 and want[0] == 0 and got[1] == want[1] == "k_step_fused_pipe<8,64,2,MarlCore>", (got, want)
        _same(env, fresh, how)
        env.Random_phase()
        assert _fused_steps(env, inp, n=1)[0][0] == 1


# ---------------------------------------------------------------------------- 5. the ring form
@pytest.mark.parametrize("V,M", [(8, 64), (4, 16)])
def test_ring_form_reads_either_source(V, M):
    """bind_step_store(fused=True): 4 steps through a ring wrap; env tensors and all seven ring arrays equal between the
    index and the tensor source, the kernel name the same."""
    from ris_vec_marl_amd import VecReplayBuffer
    N = _N()
    E, T = 777, 4
    gen = torch.Generator(device=DEV); gen.manual_seed(11 + V + M)
    power = [torch.rand(E, V, 2, device=DEV, generator=gen) * 2.4 - 1.2 for _ in range(T)]
    probs = [torch.softmax(torch.randn(E, V, V, device=DEV, generator=gen), -1) for _ in range(T)]
    mask = (torch.rand(E, V, V, device=DEV, generator=gen) < 0.6).to(torch.uint8)
    partner = torch.full((E, V), -1, dtype=torch.int32, device=DEV); partner[:, 0] = 1; partner[:, 1] = (1 << 16)
    ng = torch.full((E,), V - 1, dtype=torch.int32, device=DEV)
    runs = []
    for touch in (False, True):
        env = _env(E, V, M, seed=21)
        env.Random_phase(); env.update_channel_gains()
        if touch:
            env.tensors["theta"].mul_(1)
        buf = VecReplayBuffer(int(2.5 * E), 5, V + 2, V, device=DEV)                 # wraps during step 3
        pw, pr = torch.empty(E, V, 2, device=DEV), torch.empty(E, V, V, device=DEV)
        both = env.bind_step_store(buf, pw, partner, ng, pr, mask, fused=True, power_w=True)
        for t in range(T):
            pw.copy_(power[t]); pr.copy_(probs[t])
            both(done=t == T - 1, use_mask=t % 2 == 0)
            assert N.last_kernel().endswith("MarlCore+ring>"), N.last_kernel()
            assert N.last_theta_by_index() == (0 if touch else 1)
        runs.append((env, buf, N.last_kernel()))
    (a, buf_a, name_a), (b, buf_b, name_b) = runs
    assert name_a == name_b
    _same(a, b, "ring")
    for k in buf_a._ARRAYS:
        assert torch.equal(getattr(buf_a, k), getattr(buf_b, k)), k
