"""GPU tests of the backward walk of the software pipeline (k_step_fused_pipe<..., REV>): the fused MARL step with the
default cache policy serves its envs front to back on even steps and back to front on odd ones, so that a launch starts
on the lines the launch before read last.  The walk is an order of service only: everything a step writes must be the
same bits whether the env is forced forward, forced backward or left to the rule, and risvec_last_pipe_walk() says which
walk a launch took.  No tolerance anywhere."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.test_theta_index_step_hip import (DEV, FIXED_SHAPES, STEP_KEYS, _N, _bits, _e_two_to_three_groups, _env,  # noqa: E402
                                             _inputs, _same)

# (label, E as a function of EPW, pipe_waves): 3 envs and EPW + 1 envs by the rule's wavefront count; 3 EPW + 1 envs are
# four groups with a ragged last one -- one wavefront walks all four, or two wavefronts walk 2 EPW and EPW + 1 envs, both
# refilling the ring across group boundaries
SIZES = [("3", lambda epw: 3, 0), ("EPW+1", lambda epw: epw + 1, 0),
         ("3EPW+1/1wave", lambda epw: 3 * epw + 1, 1), ("3EPW+1/2waves", lambda epw: 3 * epw + 1, 2)]


def _walks():
    N = _N()
    return (("forward", N.FORCE_OFF), ("reverse", N.FORCE_ON), ("rule", N.BY_RULE))


def _three_walks(E, V, M, source, pipe_waves=0, pipe_nt=False, n=3):
    """One env per walk (same seed, same inputs), n fused steps each -> {walk: (env, [(query, by_index, name, parity)])}"""
    N = _N()
    inp = _inputs(E, V, E + V + M)
    out = {}
    for label, rev in _walks():
        env = _env(E, V, M)
        env.Random_phase()
        if source == "tensor":
            env.tensors["theta"].mul_(1)                   # an unannounced write: the step reads the tensor
        seen = []
        with N.forced(lat=False, pipe_nt=pipe_nt, pipe_rev=rev, pipe_waves=pipe_waves):
            for _ in range(n):
                parity = env._steps & 1
                env.step(*inp, fused=True, metrics=True, obs=True, power_w=True)
                seen.append((N.last_pipe_walk(), N.last_theta_by_index(), N.last_kernel(), parity))
        out[label] = (env, seen)
    return out


def _check(out, V, M, source, what, nt=False):
    by_index = 1 if source == "index" else 0
    name = "k_step_fused_pipe<%d,%d," % (V, M)
    for label, (env, seen) in out.items():
        assert all(s[1] == by_index for s in seen), (what, label, seen)
        assert all(s[2].startswith(name) and s[2].endswith("MarlCore,NT>" if nt else "MarlCore>") for s in seen), (what, label, seen)
    assert len({s[2] for _, seen in out.values() for s in seen}) == 1, (what, out)         # one name under every walk
    assert [s[0] for s in out["forward"][1]] == [0, 0, 0], (what, out["forward"][1])
    assert [s[0] for s in out["reverse"][1]] == ([0, 0, 0] if nt else [1, 1, 1]), (what, out["reverse"][1])
    rule = out["rule"][1]
    assert [s[0] for s in rule] == ([0, 0, 0] if nt else [s[3] for s in rule]), (what, rule)
    if not nt:
        assert {s[0] for s in rule} == {0, 1}, (what, rule)                                 # three steps: both parities
    _same(out["forward"][0], out["reverse"][0], (what, "forward vs reverse"))
    _same(out["forward"][0], out["rule"][0], (what, "forward vs rule"))


@pytest.mark.parametrize("source", ["tensor", "index"])
@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
@pytest.mark.parametrize("V,M", FIXED_SHAPES)
def test_walks_are_bit_identical(V, M, size, source):
    label, e_of, waves = size
    E = e_of(64 // V)
    _check(_three_walks(E, V, M, source, pipe_waves=waves), V, M, source, (V, M, label, source))


@pytest.mark.parametrize("source", ["tensor", "index"])
def test_walks_are_bit_identical_at_the_rules_own_grid(source):
    """8 x 64 with every wavefront of the rule's grid owning 2-3 groups a whole grid apart (the headline's layout, where
    the forced wavefront counts above give contiguous runs) and a ragged last group."""
    V, M = 8, 64
    _check(_three_walks(_e_two_to_three_groups(V), V, M, source), V, M, source, ("grid", source))


def test_non_temporal_pipeline_walks_forward_whatever_is_forced():
    """No NT + REV kernel is built: forced(pipe_nt=True, pipe_rev=ON) runs the forward non-temporal kernel."""
    V, M = 8, 64
    E = 3 * (64 // V) + 1
    out = _three_walks(E, V, M, "index", pipe_waves=1, pipe_nt=True)
    _check(out, V, M, "index", "NT", nt=True)
    plain = _three_walks(E, V, M, "index", pipe_waves=1)
    _same(out["reverse"][0], plain["reverse"][0], "NT vs default policy")


def test_ring_form_walks_are_bit_identical():
    """bind_step_store(fused=True) at 8 x 64, 3 EPW + 1 envs on one wavefront, 4 steps through a ring wrap: env tensors
    and all seven ring arrays equal under every walk, for both theta sources."""
    from ris_vec_marl_amd import VecReplayBuffer
    N = _N()
    V, M, T = 8, 64, 4
    E = 3 * (64 // V) + 1
    gen = torch.Generator(device=DEV); gen.manual_seed(5)
    power = [torch.rand(E, V, 2, device=DEV, generator=gen) * 2.4 - 1.2 for _ in range(T)]
    probs = [torch.softmax(torch.randn(E, V, V, device=DEV, generator=gen), -1) for _ in range(T)]
    mask = (torch.rand(E, V, V, device=DEV, generator=gen) < 0.6).to(torch.uint8)
    partner = torch.full((E, V), -1, dtype=torch.int32, device=DEV); partner[:, 0] = 1; partner[:, 1] = (1 << 16)
    ng = torch.full((E,), V - 1, dtype=torch.int32, device=DEV)
    for touch in (False, True):
        runs = {}
        for label, rev in _walks():
            env = _env(E, V, M, seed=21)
            env.Random_phase(); env.update_channel_gains()
            if touch:
                env.tensors["theta"].mul_(1)
            buf = VecReplayBuffer(int(2.5 * E), 5, V + 2, V, device=DEV)                 # wraps during step 3
            pw, pr = torch.empty(E, V, 2, device=DEV), torch.empty(E, V, V, device=DEV)
            both = env.bind_step_store(buf, pw, partner, ng, pr, mask, fused=True, power_w=True)
            walks = []
            with N.forced(pipe_rev=rev, pipe_waves=1):
                for t in range(T):
                    pw.copy_(power[t]); pr.copy_(probs[t])
                    parity = env._steps & 1
                    both(done=t == T - 1, use_mask=t % 2 == 0)
                    assert N.last_kernel() == "k_step_fused_pipe<8,64,2,MarlCore+ring>", N.last_kernel()
                    assert N.last_theta_by_index() == (0 if touch else 1)
                    walks.append((N.last_pipe_walk(), parity))
            runs[label] = (env, buf, walks)
        assert [w for w, _ in runs["forward"][2]] == [0] * T and [w for w, _ in runs["reverse"][2]] == [1] * T, runs
        assert [w for w, _ in runs["rule"][2]] == [p for _, p in runs["rule"][2]], runs["rule"][2]
        for other in ("reverse", "rule"):
            _same(runs["forward"][0], runs[other][0], ("ring", touch, other))
            for k in runs["forward"][1]._ARRAYS:
                assert torch.equal(getattr(runs["forward"][1], k), getattr(runs[other][1], k)), (touch, other, k)
