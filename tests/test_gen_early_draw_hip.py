"""GPU tests of what the row-per-lane GEN members (k_step_fused_gen<..., ONE>, gen_row_lane_form) take out of the span behind
their chains: the Philox arrival draw is made while the lane's loads are in flight and handed to step_pre, and step()'s loads
and stores go through RowLaneAddr -- a wave-uniform base per array plus a small lane offset -- instead of a 64-bit index per
lane.  Both are exact integer / address work, so GEN as the rule deals it must leave the bits of the reading form (h_r touched
through torch: the flag is not sent, k_step_fused_pipe reads the rows and draws inside step_pre with the per-lane index) in
every tensor a step writes, after each of three consecutive steps with data_buf / mec_q carried.  No tolerance anywhere.

What is varied is what the two parts depend on:
  * env_offset 0, 2^31 - 3 (the sign bit of the draw's 32-bit counter word flips inside the batch) and 2^32 - 1 - E (the
    batch ends on the highest env id the library admits).  Offsets past that -- 2^32 - 3, where the word would wrap inside
    the batch, or 5 2^32 + 7 -- cannot be tested: every entry point refuses a state whose env_offset + n_envs does not fit 32
    bits (check_common, risvec_api.hip), so no launch ever sees one;
  * arrival rate 1 (the shipped one) and 12, where almost every draw exceeds 7 and the table loop behind cdf[7] runs inside
    the load shadow -- asserted on the CPU with the oracle's Philox and the same table;
  * injected arrivals (a ramp that differs from the draw in every lane): the early draw must not be what is added;
  * the oracle's own draw injected: the two paths tied together;
  * partial groups: every output has a guard row behind E prefilled with a NaN pattern, which must stay unwritten."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import risvec_oracle as orc  # noqa: E402
from tests.test_gen_row_lane_hip import ROW_LANE_SHAPES, SIZES, _bits, _hard_theta  # noqa: E402
from tests.test_hip_parity import make_vec  # noqa: E402
from tests.test_theta_index_step_hip import DEV, STEP_KEYS, _N, _inputs  # noqa: E402

STEPS = 3
SEED = 9
GUARD_BITS = 0x7FC0BEEF                                    # a quiet NaN no kernel produces
OFFSETS = {"0": lambda E: 0, "sign": lambda E: 2 ** 31 - 3, "top": lambda E: 2 ** 32 - 1 - E}
RATES = [1.0, 12.0]
DRAWS = [(o, r) for o in OFFSETS for r in RATES]
CORES = ["marl", "ring"]


def _e_of(V, label):
    return dict((s[0], s[1]) for s in SIZES)[label](64 // V)


def _guard(env):
    """re-seat every output of step() on an allocation of its own with one more env row, that row a NaN pattern"""
    E = env.n_envs
    big = {}
    for k, (_, shp) in env._out_offsets.items():
        g = torch.empty((E + 1,) + tuple(shp[1:]), dtype=torch.float32, device=DEV)
        g[:E].copy_(env._t[k])
        g[E:].view(torch.int32).fill_(GUARD_BITS)
        env._t[k] = g[:E]
        setattr(env._cstate, k, g.data_ptr())
        big[k] = g
    return big


def _guard_intact(big, E, what):
    for k, g in big.items():
        assert bool((g[E:].view(torch.int32) == GUARD_BITS).all()), (what, "guard row written", k)


def _state(E, V, M, source, touch, env_offset, rate):
    env = make_vec(E, V, M, b=3, seed=SEED, env_offset=env_offset, yaml=True)
    env.rate = rate
    env.make_new_game(); env.renew_positions(); env.compute_parms()
    env.Random_phase()
    _hard_theta(env, E, M, source)
    if touch:
        env.tensors["h_r"].mul_(1)                         # ends the permission to rebuild: the reading form
    return env, _guard(env)


def _check_launch(N, V, M, source, touch, what):
    assert N.last_h_r_rebuilt() == (0 if touch else 1), what
    assert N.last_gen_groups_per_wave() == (0 if touch else 1), what       # 1: the row-per-lane member ran
    assert N.last_theta_by_index() == (1 if source == "index" else 0), what
    assert N.last_kernel().startswith("k_step_fused_pipe<%d,%d," % (V, M)), what


def _run(V, M, E, core, source, touch, env_offset, rate, arrivals, what):
    """three steps of one form -> [(key@step, tensor)], plus the ring's arrays behind the last"""
    N = _N()
    env, big = _state(E, V, M, source, touch, env_offset, rate)
    out = []
    if core == "marl":
        action, partner, ng, _ = _inputs(E, V, E + V + M)
        with N.forced(lat=False, pipe_nt=False):
            for step in range(STEPS):
                env.step(action, partner, ng, arrivals, fused=True, metrics=True, obs=True, power_w=True)
                _check_launch(N, V, M, source, touch, what + (step,))
                out += [("%s@%d" % (k, step), env.tensors[k].clone()) for k in STEP_KEYS]
    else:
        from ris_vec_marl_amd import VecReplayBuffer
        g = torch.Generator(device=DEV); g.manual_seed(5)
        power = [torch.rand(E, V, 2, device=DEV, generator=g) * 2.4 - 1.2 for _ in range(STEPS)]
        probs = [torch.softmax(torch.randn(E, V, V, device=DEV, generator=g), -1) for _ in range(STEPS)]
        mask = (torch.rand(E, V, V, device=DEV, generator=g) < 0.6).to(torch.uint8)
        partner = torch.full((E, V), -1, dtype=torch.int32, device=DEV); partner[:, 0] = 1; partner[:, 1] = (1 << 16)
        ng = torch.full((E,), V - 1, dtype=torch.int32, device=DEV)
        env.update_channel_gains()
        buf = VecReplayBuffer(max(E, (3 * E) // 2), 5, V + 2, V, device=DEV)      # the second step's rows wrap
        pw, pr = torch.empty(E, V, 2, device=DEV), torch.empty(E, V, V, device=DEV)
        both = env.bind_step_store(buf, pw, partner, ng, pr, mask, arrivals=arrivals, fused=True, power_w=True)
        with N.forced(pipe_nt=False):
            for step in range(STEPS):
                pw.copy_(power[step]); pr.copy_(probs[step])
                both(done=step == STEPS - 1, use_mask=step % 2 == 0)
                _check_launch(N, V, M, source, touch, what + (step,))
                assert N.last_kernel().endswith(",MarlCore+ring>")
                out += [("%s@%d" % (k, step), env.tensors[k].clone()) for k in STEP_KEYS]
        out += [(k, getattr(buf, k).clone()) for k in buf._ARRAYS]
    _guard_intact(big, E, what)
    return out


def _same_bits(ref, got, what):
    assert len(ref) == len(got)
    for (k, a), (k2, b) in zip(ref, got):
        assert k == k2 and torch.equal(_bits(a), _bits(b)), (what, k)


def _oracle_draws(E, V, env_offset, rate):
    """[STEPS, E, V] int32: the counts the kernels draw at (env id, vehicle, step counter 0 ..., seed)"""
    ids = np.arange(E, dtype=np.uint64) + np.uint64(env_offset)
    return np.stack([orc.philox_arrivals(ids, V, s, SEED, rate) for s in range(STEPS)])


def _philox_case(V, M, E, core, source, env_offset, rate):
    env_offset = OFFSETS[env_offset](E)
    what = (V, M, E, core, source, env_offset, rate)
    if rate == 12.0:
        assert (_oracle_draws(E, V, env_offset, rate) > 7).mean() > 0.5, what       # the table loop really runs
    read = _run(V, M, E, core, source, True, env_offset, rate, None, what + ("read",))
    gen = _run(V, M, E, core, source, False, env_offset, rate, None, what + ("gen",))
    _same_bits(read, gen, what)
    return gen


# every shape, size and core with theta by index; the (env_offset, rate) pairs are dealt round so that each shape and each
# core meets all six
@pytest.mark.parametrize("core", CORES)
@pytest.mark.parametrize("size", [s[0] for s in SIZES])
@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_philox_path_same_bits_as_the_reading_form(V, M, size, core):
    i = ROW_LANE_SHAPES.index((V, M)) + 2 * [s[0] for s in SIZES].index(size) + 3 * CORES.index(core)
    env_offset, rate = DRAWS[i % len(DRAWS)]
    _philox_case(V, M, _e_of(V, size), core, "index", env_offset, rate)


# all six pairs at the size with four groups, where the sign bit flips inside the first group
@pytest.mark.parametrize("env_offset,rate", DRAWS, ids=["%s-rate%d" % (o, r) for o, r in DRAWS])
@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_every_offset_and_rate_at_four_groups(V, M, env_offset, rate):
    _philox_case(V, M, _e_of(V, "3EPW+1"), "marl", "index", env_offset, rate)


@pytest.mark.parametrize("core", CORES)
@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_theta_by_tensor(V, M, core):
    _philox_case(V, M, _e_of(V, "EPW+1"), core, "tensor", "sign", 12.0)


@pytest.mark.parametrize("core", CORES)
@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_injected_arrivals_win_over_the_early_draw(V, M, core):
    E, rate = _e_of(V, "EPW+1"), 1.0
    env_offset = OFFSETS["top"](E)
    what = (V, M, E, core, "injected")
    draws = _oracle_draws(E, V, env_offset, rate)
    ramp = np.arange(E * V, dtype=np.int32).reshape(E, V) % 5 + 20                 # 20 ... 24: no draw at rate 1 gets there
    assert (ramp[None] != draws).all()
    arr = torch.from_numpy(ramp).to(DEV)
    read = _run(V, M, E, core, "index", True, env_offset, rate, arr, what + ("read",))
    gen = _run(V, M, E, core, "index", False, env_offset, rate, arr, what + ("gen",))
    _same_bits(read, gen, what)
    philox = _run(V, M, E, core, "index", False, env_offset, rate, None, what + ("philox",))
    for (k, a), (_, b) in zip(gen, philox):
        if k.startswith("data_buf@"):
            assert not torch.equal(_bits(a), _bits(b)), (what, k)


@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_injecting_the_oracles_draw_gives_the_philox_bits(V, M):
    """one launch per step (the arrivals change from step to step), so through step(), which marshals per call"""
    N = _N()
    E, rate = _e_of(V, "3EPW+1"), 12.0
    env_offset = OFFSETS["sign"](E)
    what = (V, M, E, "tied")
    draws = _oracle_draws(E, V, env_offset, rate)
    philox = _run(V, M, E, "marl", "index", False, env_offset, rate, None, what + ("philox",))
    env, big = _state(E, V, M, "index", False, env_offset, rate)
    action, partner, ng, _ = _inputs(E, V, E + V + M)
    out = []
    with N.forced(lat=False, pipe_nt=False):
        for step in range(STEPS):
            env.step(action, partner, ng, torch.from_numpy(draws[step]).to(DEV), fused=True, metrics=True, obs=True,
                     power_w=True)
            _check_launch(N, V, M, "index", False, what + (step,))
            out += [("%s@%d" % (k, step), env.tensors[k].clone()) for k in STEP_KEYS]
    _guard_intact(big, E, what)
    _same_bits(philox, out, what)
