"""GPU tests of the row-per-lane GEN members (k_step_fused_gen<..., ONE>, gen_row_lane_form) as the library ships them -- the
headline member with its wave-priority schedule (GenRowSchedule, k_step_gen.hip) -- and of the DIAGNOSTIC build that stamps
them (librisvec_gen_stamps.so, make -C ris_vec_marl_amd/csrc gen_stamps; tools/gen_wave_timeline.py).

A priority level changes when a wavefront issues, never what: GEN as the rule deals it (risvec_last_gen_groups_per_wave()
== 1) must leave the bits of the reading form (h_r touched through torch: k_step_fused_pipe reads the rows) in every tensor
a step writes, after each of two steps with data_buf / mec_q carried.  Shapes 8 x 64, 4 x 16 (one leaf: the schedules
collapse) and 16 x 64; E = 1 (one partial group) and E = 64 / V + 1 (two wavefronts, the second ragged); MARL core, theta
by index.  No tolerance anywhere.

Where the stamps library has been built, a child process (a library is chosen once per process, RISVEC_LIB) runs the same
cases at E = 64 / V + 1 on it with a stamp buffer handed over: its outputs are the shipped library's bit for bit, every
wavefront's stamps are non-decreasing and as many as the shape has (entry, first wait, a stamp per leaf, tree, late
arguments, last store), and the SIMD ids lie in 0 ... 3."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.test_gen_row_lane_hip import ROW_LANE_SHAPES, _bits, _hard_theta  # noqa: E402
from tests.test_hip_parity import make_vec  # noqa: E402
from tests.test_theta_index_step_hip import DEV, STEP_KEYS, _N, _inputs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAMPS_LIB = os.path.join(ROOT, "ris_vec_marl_amd", "csrc", "librisvec_gen_stamps.so")
STEPS = 2
SEED = 9
SLOTS = 16                                                 # uint64 per wavefront (kGenStampSlots, k_step_gen.hip)
SIZES = {"1": lambda epw: 1, "EPW+1": lambda epw: epw + 1}


def _leaves(V, M):
    """leaves of row_tree that run chains: min(G, M / 2) / 8, G the lane group of the reading form"""
    return max(M // 16, 1)


def _run(V, M, E, touch, what):
    """two steps of one form -> [(key@step, tensor)]"""
    N = _N()
    env = make_vec(E, V, M, b=3, seed=SEED, yaml=True)
    env.make_new_game(); env.renew_positions(); env.compute_parms()
    env.Random_phase()
    _hard_theta(env, E, M, "index")
    if touch:
        env.tensors["h_r"].mul_(1)                         # ends the permission to rebuild: the reading form
    action, partner, ng, _ = _inputs(E, V, E + V + M)
    out = []
    with N.forced(lat=False, pipe_nt=False):
        for step in range(STEPS):
            env.step(action, partner, ng, None, fused=True, metrics=True, obs=True, power_w=True)
            assert N.last_h_r_rebuilt() == (0 if touch else 1), what + (step,)
            assert N.last_gen_groups_per_wave() == (0 if touch else 1), what + (step,)     # 1: the row-per-lane member ran
            assert N.last_theta_by_index() == 1, what + (step,)
            assert N.last_kernel().startswith("k_step_fused_pipe<%d,%d," % (V, M)), what + (step,)
            out += [("%s@%d" % (k, step), env.tensors[k].clone()) for k in STEP_KEYS]
    return out


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_shipped_row_lane_member_has_the_reading_forms_bits(V, M, size):
    E = SIZES[size](64 // V)
    what = (V, M, E)
    read = _run(V, M, E, True, what + ("read",))
    gen = _run(V, M, E, False, what + ("gen",))
    assert len(read) == len(gen) == STEPS * len(STEP_KEYS)
    for (k, a), (k2, b) in zip(read, gen):
        assert k == k2 and torch.equal(_bits(a), _bits(b)), (what, k)


def _child(path):
    """(the stamps library is loaded: RISVEC_LIB) the three shapes at E = EPW + 1 with a stamp buffer -> an .npz"""
    import ctypes as C
    N = _N()
    set_buf = N.load().risvec_gen_stamps_buffer
    set_buf.restype, set_buf.argtypes = C.c_int, [C.c_void_p, C.c_longlong]
    res = {}
    for V, M in ROW_LANE_SHAPES:
        E = SIZES["EPW+1"](64 // V)
        n_waves = (E * V + 63) // 64
        buf = torch.zeros(n_waves * SLOTS, dtype=torch.int64, device=DEV)
        assert set_buf(buf.data_ptr(), n_waves) == 0
        for k, t in _run(V, M, E, False, (V, M, E, "stamps")):
            res["%dx%d/%s" % (V, M, k)] = _bits(t).cpu().numpy()
        torch.cuda.synchronize()
        res["%dx%d/stamps" % (V, M)] = buf.cpu().numpy().view(np.uint64).reshape(n_waves, SLOTS)
        assert set_buf(None, 0) == 0
    np.savez(path, **res)


@pytest.fixture(scope="module")
def stamped(tmp_path_factory):
    if not os.path.isfile(STAMPS_LIB):
        pytest.skip("librisvec_gen_stamps.so is not built (make -C ris_vec_marl_amd/csrc gen_stamps)")
    path = str(tmp_path_factory.mktemp("gen_stamps") / "out.npz")
    env = dict(os.environ, RISVEC_LIB=STAMPS_LIB, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, env=env, check=True, timeout=300)
    return np.load(path)


@pytest.mark.parametrize("V,M", ROW_LANE_SHAPES)
def test_stamps_library_same_bits_and_sane_stamps(stamped, V, M):
    E = SIZES["EPW+1"](64 // V)
    what = (V, M, E)
    tag = "%dx%d/" % (V, M)
    for k, t in _run(V, M, E, False, what + ("shipped",)):
        assert np.array_equal(stamped[tag + k], _bits(t).cpu().numpy()), (what, k)
    raw = stamped[tag + "stamps"]
    assert raw.shape == (2, SLOTS)                                              # two wavefronts
    n = _leaves(V, M) + 5
    assert ((raw[:, 15] >> np.uint64(32)) == n).all(), what                     # both wrote, this many stamps each
    t = raw[:, :n].astype(np.int64)
    assert (t[:, 0] > 0).all() and (np.diff(t, axis=1) >= 0).all(), (what, t)
    assert (raw[:, 13] >= raw[:, 12]).all(), what                               # s_memrealtime at entry and end
    hw = raw[:, 15].astype(np.int64) & 0xFFFFFFFF
    simd = (hw >> 4) & 0x3                                                      # HW_REG_HW_ID [5:4]
    assert ((simd >= 0) & (simd <= 3)).all(), what
    xcc = raw[:, 14].astype(np.int64) & 0xF                                     # HW_REG_XCC_ID [3:0]
    assert (xcc <= 7).all(), what
    # the two wavefronts are one workgroup's: one XCC, one CU (SE [15:13], SH [12], CU [11:8])
    assert xcc[0] == xcc[1] and (hw[0] >> 8) & 0xFF == (hw[1] >> 8) & 0xFF, (what, hex(hw[0]), hex(hw[1]))


if __name__ == "__main__":
    _child(sys.argv[1])
