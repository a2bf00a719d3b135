"""GPU tests of when the HD row-per-lane GEN members (k_step_fused_gen<..., ONE, HD>, gen_row_lane_form) request the chunk
heads of their rows and step()'s inputs (GenRowSchedule, gen_head_rank() in k_step_gen.hip).  The headline member (plain
MARL core, 8 x 64) requests the head of the first leaf with the entry batch, every other head at the top of the leaf before
its own, and step()'s inputs at the top of the second leaf; the ring core and the other shapes request everything in the
entry batch.  Where a value is requested changes no value: GEN as the rule deals it (risvec_last_gen_groups_per_wave() ==
1, heads read) must leave the bits of the reading form (h_r touched through torch: k_step_fused_pipe reads the rows) in
every tensor a step writes, after each of three steps with data_buf / mec_q carried.  No tolerance anywhere.

  * shapes 8 x 64 and 16 x 64 (four leaves) and 4 x 16 (NCH = 1: nothing can be deferred, it must simply still be equal);
  * E in {1, EPW - 1, EPW + 1, 3 EPW + 1}: a deferred request on an inactive lane goes through the clamped row, and every
    output has a guard row behind E prefilled with a NaN pattern, which must stay unwritten;
  * MARL core and ring core; theta by index, and theta by tensor at EPW + 1;
  * renew_positions() + compute_parms() between steps two and three: the heads are rewritten there and the third step's
    requests, entry and deferred, must read the new ones."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.test_gen_early_draw_hip import _guard, _guard_intact, _same_bits  # noqa: E402
from tests.test_gen_row_lane_hip import ROW_LANE_SHAPES, SIZES, _hard_theta  # noqa: E402
from tests.test_hip_parity import make_vec  # noqa: E402
from tests.test_theta_index_step_hip import DEV, STEP_KEYS, _N, _inputs  # noqa: E402

STEPS = 3
SEED = 9
CORES = ["marl", "ring"]
SIZE_OF = dict((s[0], s[1]) for s in SIZES)
assert list(SIZE_OF) == ["1", "EPW-1", "EPW+1", "3EPW+1"]
assert sorted(ROW_LANE_SHAPES) == [(4, 16), (8, 64), (16, 64)]


def _check_launch(N, V, M, source, touch, what):
    assert N.last_h_r_rebuilt() == (0 if touch else 1), what
    assert N.last_h_r_heads() == (0 if touch else 1), what                 # the HD member: the heads are what is read
    assert N.last_gen_groups_per_wave() == (0 if touch else 1), what       # 1: the row-per-lane member ran
    assert N.last_theta_by_index() == (1 if source == "index" else 0), what
    assert N.last_kernel().startswith("k_step_fused_pipe<%d,%d," % (V, M)), what


def _run(V, M, E, core, source, touch, renew, what):
    """three steps of one form -> [(key@step, tensor)], plus the ring's arrays behind the last.  renew: new positions and
    geometry (and with it new heads) in front of the third step."""
    N = _N()
    env = make_vec(E, V, M, b=3, seed=SEED, yaml=True)
    env.make_new_game(); env.renew_positions(); env.compute_parms()
    env.Random_phase()
    _hard_theta(env, E, M, source)
    if touch:
        env.tensors["h_r"].mul_(1)                         # ends the permission to rebuild: the reading form
    big = _guard(env)
    out = []

    def before(step):
        if renew and step == STEPS - 1:
            env.renew_positions(); env.compute_parms()
            if touch:
                env.tensors["h_r"].mul_(1)

    if core == "marl":
        action, partner, ng, _ = _inputs(E, V, E + V + M)
        with N.forced(lat=False, pipe_nt=False):
            for step in range(STEPS):
                before(step)
                env.step(action, partner, ng, None, fused=True, metrics=True, obs=True, power_w=True)
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
        both = env.bind_step_store(buf, pw, partner, ng, pr, mask, fused=True, power_w=True)
        with N.forced(pipe_nt=False):
            for step in range(STEPS):
                before(step)
                pw.copy_(power[step]); pr.copy_(probs[step])
                both(done=step == STEPS - 1, use_mask=step % 2 == 0)
                _check_launch(N, V, M, source, touch, what + (step,))
                assert N.last_kernel().endswith(",MarlCore+ring>")
                out += [("%s@%d" % (k, step), env.tensors[k].clone()) for k in STEP_KEYS]
        out += [(k, getattr(buf, k).clone()) for k in buf._ARRAYS]
    _guard_intact(big, E, what)
    return out


def _case(V, M, size, core, source, renew=False):
    E = SIZE_OF[size](64 // V)
    what = (V, M, E, core, source, renew)
    read = _run(V, M, E, core, source, True, renew, what + ("read",))
    gen = _run(V, M, E, core, source, False, renew, what + ("gen",))
    assert len(gen) >= STEPS * len(STEP_KEYS)
    _same_bits(read, gen, what)
    if renew:                                              # the new geometry really changed what the third step wrote
        still = _run(V, M, E, core, source, False, False, what + ("still",))
        assert not all(torch.equal(a, b) for (k, a), (_, b) in zip(gen, still) if k.endswith("@%d" % (STEPS - 1))), what


INDEX_CASES = [(V, M, s, c) for V, M in ROW_LANE_SHAPES for s in SIZE_OF for c in CORES]
TENSOR_CASES = [(V, M, "EPW+1", c) for V, M in ROW_LANE_SHAPES for c in CORES]
RENEW_CASES = [(V, M, "EPW+1", "marl") for V, M in ROW_LANE_SHAPES]


@pytest.mark.parametrize("V,M,size,core", INDEX_CASES)
def test_theta_by_index_same_bits_as_the_reading_form(V, M, size, core):
    _case(V, M, size, core, "index")


@pytest.mark.parametrize("V,M,size,core", TENSOR_CASES)
def test_theta_by_tensor_same_bits_as_the_reading_form(V, M, size, core):
    _case(V, M, size, core, "tensor")


@pytest.mark.parametrize("V,M,size,core", RENEW_CASES)
def test_new_geometry_before_the_third_step_is_what_the_requests_read(V, M, size, core):
    _case(V, M, size, core, "index", renew=True)
