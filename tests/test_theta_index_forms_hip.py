"""GPU tests of RISVEC_STEP_THETA_IDX_CURRENT in every byte-bound form of the fused step: the software pipeline with the
non-temporal hint (and its ring form), and the latency-shaped kernels' NT and ALT members.  In each of them the index
source (one byte per theta element) and the tensor source (complex64) must give the same bits in everything a step
writes, under the same kernel name; the latency members with the default cache policy must go on ignoring the bit.
Forms are forced at the smallest sizes that reach the code; no tolerance: both sources feed the same arithmetic the same
bits."""
import re

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.test_theta_index_step_hip import (DEV, FIXED_SHAPES, _N, _bits, _discrete_theta, _e_two_to_three_groups,  # noqa: E402
                                             _env, _fused_steps, _inputs, _same)

LAT_EMAX = {(8, 64): 4, (8, 36): 4, (8, 40): 4, (4, 16): 4, (16, 256): 1, (8, 100): 4}   # envs per wavefront of the NT / ALT member


def _two_sources(E, V, M, force, by_index=True):
    """env A steps with current indices, env B (same seed) after `tensors["theta"].mul_(1)`, three fused steps each under
    the forced forms -> the kernel names of A.  Everything a step writes is equal, the names are equal, and the query
    says A read the indices (where `by_index`) and B the tensor."""
    N = _N()
    inp = _inputs(E, V, E + V + M)
    envs = []
    for touch in (False, True):
        env = _env(E, V, M)
        env.Random_phase()
        if touch:
            env.tensors["theta"].mul_(1)
        envs.append(env)
    a, b = envs
    assert a._idx_current and a._idx_current_flag() == N.STEP_THETA_IDX_CURRENT      # the bit is sent for A ...
    assert b._idx_current_flag() == 0                                                # ... and not for B
    assert torch.equal(_bits(a.tensors["theta"]), _bits(b.tensors["theta"]))
    with N.forced(**force):
        seen_a = _fused_steps(a, inp)
        seen_b = _fused_steps(b, inp)
    assert [q for q, _ in seen_a] == [1 if by_index else 0] * 3 and [q for q, _ in seen_b] == [0, 0, 0], (seen_a, seen_b)
    assert [n for _, n in seen_a] == [n for _, n in seen_b], (seen_a, seen_b)
    _same(a, b, (E, V, M, force))
    return [n for _, n in seen_a]


# ---------------------------------------------------------------------------- 1. the NT pipeline
def _pipe_nt_cases():
    for V, M in FIXED_SHAPES:
        yield V, M, "3"
        yield V, M, "EPW+1"
        if (V, M) in ((8, 64), (4, 16)):
            yield V, M, "groups"


@pytest.mark.parametrize("V,M,size", list(_pipe_nt_cases()))
def test_nt_pipeline_reads_either_source(V, M, size):
    E = {"groups": _e_two_to_three_groups(V) if size == "groups" else 0, "3": 3, "EPW+1": 64 // V + 1}[size]
    names = _two_sources(E, V, M, dict(lat=False, pipe_nt=True))
    for n in names:
        assert n.startswith("k_step_fused_pipe<%d,%d," % (V, M)) and n.endswith("MarlCore,NT>"), names


# ---------------------------------------------------------------------------- 2. the latency family, NT
@pytest.mark.parametrize("V,M", [(8, 64), (8, 36), (8, 40), (4, 16), (16, 256), (8, 100)])
@pytest.mark.parametrize("size", ["3", "EMAX+1", "515"])
def test_latency_nt_reads_either_source(V, M, size):
    emax = LAT_EMAX[(V, M)]
    E = {"3": 3, "EMAX+1": emax + 1, "515": 515}[size]
    names = _two_sources(E, V, M, dict(lat=True, lat_nt=True))
    for n in names:
        assert n.startswith("k_step_fused_lat<%d," % V) and n.endswith(",%d,NT>" % emax), names


# ---------------------------------------------------------------------------- 3. the latency family, ALT
@pytest.mark.parametrize("V,M", [(8, 64), (8, 36), (4, 16)])
def test_latency_alt_reads_either_source(V, M):
    """three consecutive steps: a.ping is the step counter's parity, so both walk directions run"""
    names = _two_sources(515, V, M, dict(lat=True, lat_alt=True))
    assert names == ["k_step_fused_lat<%d,%d,4,ALT>" % (V, M)] * 3, names


# ---------------------------------------------------------------------------- 4. the latency family, default policy
@pytest.mark.parametrize("force", [dict(lat=True), dict(lat=True, lat_epw=4)], ids=["rules", "EMAX"])
def test_latency_default_policy_ignores_the_bit(force):
    """The bit is sent, and the default-policy members read the tensor all the same.  `forced(lat=True)` alone leaves the
    envs per wavefront to the rules, which give 515 envs one each (`k_step_fused_lat<8,64,1>`); `lat_epw=4` makes it the
    EMAX member `k_step_fused_lat<8,64,4>`, the one whose by-index instantiation exists and must not be taken."""
    names = _two_sources(515, 8, 64, force, by_index=False)
    for n in names:
        assert re.fullmatch(r"k_step_fused_lat<8,64,[124]>", n), names
    if "lat_epw" in force:
        assert names == ["k_step_fused_lat<8,64,4>"] * 3, names


# ---------------------------------------------------------------------------- 5. the ring form under the NT pipeline
def test_ring_form_under_the_nt_pipeline_reads_either_source():
    """The body of test_theta_index_step_hip.test_ring_form_reads_either_source at (8, 64) with the NT pipeline forced."""
    from ris_vec_marl_amd import VecReplayBuffer
    N = _N()
    V, M = 8, 64
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
        with N.forced(pipe_nt=True):
            for t in range(T):
                pw.copy_(power[t]); pr.copy_(probs[t])
                both(done=t == T - 1, use_mask=t % 2 == 0)
                assert N.last_kernel() == "k_step_fused_pipe<8,64,2,MarlCore+ring,NT>", N.last_kernel()
                assert N.last_theta_by_index() == (0 if touch else 1)
        runs.append((env, buf))
    (a, buf_a), (b, buf_b) = runs
    _same(a, b, "ring,NT")
    for k in buf_a._ARRAYS:
        assert torch.equal(getattr(buf_a, k), getattr(buf_b, k)), k


# ---------------------------------------------------------------------------- 6. invalidation under a forced NT form
def test_a_theta_write_drops_the_indices_under_a_forced_nt_form():
    """One by-index step in the latency NT member, then an unannounced `copy_` of another discrete theta: the next step
    reads the tensor, and writes what a fresh env writes that got the same theta through invalidate_theta()."""
    N = _N()
    E, V, M = 515, 8, 64
    inp = _inputs(E, V, 5)
    other = _discrete_theta(E, M, 3)
    env = _env(E, V, M)
    env.Random_phase()
    fresh = _env(E, V, M)
    fresh.Random_phase()
    with N.forced(lat=True, lat_nt=True):
        assert _fused_steps(env, inp, n=1) == [(1, "k_step_fused_lat<8,64,4,NT>")]
        assert _fused_steps(fresh, inp, n=1) == [(1, "k_step_fused_lat<8,64,4,NT>")]
        env.tensors["theta"].copy_(other)
        fresh.tensors["theta"].copy_(other)
        fresh.invalidate_theta()
        assert torch.equal(_bits(env.tensors["theta"]), _bits(fresh.tensors["theta"]))
        got = _fused_steps(env, inp, n=1)
        want = _fused_steps(fresh, inp, n=1)
    assert got == want == [(0, "k_step_fused_lat<8,64,4,NT>")], (got, want)
    _same(env, fresh, "copy_")
