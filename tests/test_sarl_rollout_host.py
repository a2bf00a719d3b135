"""CPU-side tests of the SARL rollout entry points: which shapes have a kernel, argument validation without a GPU, the
struct the binding hands over, and the float64 oracle alone on the inputs the GPU tests use."""
import ctypes as C
import math

import numpy as np
import pytest

import ris_vec_marl_amd as rv
from ris_vec_marl_amd import _native as N
from oracle import risvec_oracle as orc


def test_supported_truth_table():
    lib = N.load()
    for V in range(1, 20):
        for M in range(1, 262):
            want = V in (4, 8, 16) and M % 2 == 0 and V <= M <= 256
            assert bool(lib.risvec_sarl_rollout_supported(V, M)) == want, (V, M)
    assert not lib.risvec_sarl_rollout_supported(8, 258) and not lib.risvec_sarl_rollout_supported(5, 21)
    assert not lib.risvec_sarl_rollout_supported(-8, 40) and not lib.risvec_sarl_rollout_supported(8, 0)


def test_abi_version_and_struct_bytes():
    lib = N.load()
    assert lib.risvec_abi_version() == N.ABI_VERSION == 17
    # 4-byte header pair, 3 + 3 + 5 pointers, 4 floats, 4 eight-byte scalars: no padding on an LP64 target
    assert C.sizeof(N.RisVecSarlRollout) == 8 + 11 * 8 + 4 * 4 + 4 * 8 == 144
    names = [n for n, _ in N.RisVecSarlRollout._fields_]
    for n in ("mu", "ou_x", "z", "ou_theta", "ou_mu", "ou_sigma", "ou_dt", "action", "phase", "obs_full", "state_memory",
              "action_memory", "reward_memory", "new_state_memory", "terminal_memory", "mem_size", "mem_cntr", "done"):
        assert n in names, n
    assert {"OUNoise", "SarlReplayBuffer"} <= set(rv.__all__)
    assert {"risvec_sarl_rollout", "risvec_sarl_rollout_supported", "risvec_sarl_replay_sample"} <= set(N.EXPORTS)


def _state(V=8, M=40, E=4):
    s = N.RisVecState()
    s.abi_version, s.struct_bytes = N.ABI_VERSION, C.sizeof(N.RisVecState)
    s.n_envs, s.n_veh, s.n_ris, s.control_bit = E, V, M, 3
    return s


def test_rollout_rejects_bad_arguments_without_touching_a_gpu():
    """Nothing here owns device memory: every call must fail in the argument checks (fake, never dereferenced addresses
    stand in for device pointers)."""
    lib = N.load()
    err = lambda: lib.risvec_last_error().decode()      # noqa: E731
    p = rv.SarlParams().to_c()
    r = N.RisVecSarlRollout()
    s = _state()
    call = lambda ss=s, pp=p, rr=r, flags=0: lib.risvec_sarl_rollout(C.byref(ss), C.byref(pp) if pp else None,   # noqa: E731
                                                                    C.byref(rr) if rr else None, None, 0, 0, flags, None)
    assert call(pp=None) == N.ERR_ARG and "params is NULL" in err()
    assert call(rr=None) == N.ERR_ARG and "rollout is NULL" in err()
    assert call() == N.ERR_ARG and "RisVecSarlRollout ABI mismatch" in err()          # struct_bytes = 0
    r.struct_bytes = C.sizeof(N.RisVecSarlRollout)
    bad = rv.SarlParams().to_c()
    bad.struct_bytes += 4
    assert call(pp=bad) == N.ERR_ARG and "RisVecSarlParams ABI mismatch" in err()
    assert call(ss=N.RisVecState()) == N.ERR_ARG and "RisVecState ABI mismatch" in err()
    assert call(flags=N.STEP_METRICS) == N.ERR_ARG and "flag" in err()
    for V, M in ((5, 21), (8, 258), (8, 41), (16, 8)):
        assert call(ss=_state(V, M)) == N.ERR_UNSUPPORTED and "staged path" in err(), (V, M)
    assert call() == N.ERR_ARG and "rollout.mu is NULL" in err()
    fake = 0x7F0000001000                                 # 16-byte aligned, never dereferenced
    r.mu = fake + 8
    assert call() == N.ERR_ARG and "rollout.mu is not 16-byte aligned" in err()
    r.mu, r.action, r.phase, r.obs_full = fake, fake, fake, fake
    r.z = fake
    assert call() == N.ERR_ARG and "needs rollout.ou_x" in err()
    r.ou_x, r.ou_dt = fake, -1.0
    assert call() == N.ERR_ARG and "ou_dt" in err()
    r.ou_dt, r.ou_env_offset = 0.01, -1
    assert call() == N.ERR_SHAPE and "ou_env_offset" in err()
    r.ou_env_offset = 0
    assert call() == N.ERR_ARG and "state.h_r is NULL" in err()
    for k in ("h_r", "theta", "b", "pl", "gain", "data_buf", "rate", "data_t", "data_p", "reward", "over_power",
              "over_data", "metrics", "obs"):
        setattr(s, k, fake)
    # the ring: all five arrays or none, aligned, and room for one step's transitions
    r.state_memory = fake
    assert call() == N.ERR_ARG and "ring.action_memory is NULL" in err()
    r.action_memory, r.reward_memory, r.new_state_memory, r.terminal_memory = fake, fake + 4, fake, fake
    assert call() == N.ERR_ARG and "ring.reward_memory is not 16-byte aligned" in err()
    r.reward_memory, r.mem_size = fake, 3
    assert call() == N.ERR_SHAPE and "do not fit mem_size" in err()
    r.mem_size, r.mem_cntr = 4, -1
    assert call() == N.ERR_ARG and "mem_cntr" in err()
    with pytest.raises(ValueError):
        N.check(N.ERR_SHAPE)


def test_replay_sample_rejects_bad_arguments_without_touching_a_gpu():
    lib = N.load()
    err = lambda: lib.risvec_last_error().decode()      # noqa: E731
    fake = 0x7F0000001000
    r = N.RisVecSarlRollout()
    call = lambda rr=r, S=10, A=56, mm=8, B=4, out=fake: lib.risvec_sarl_replay_sample(   # noqa: E731
        C.byref(rr) if rr else None, S, A, mm, B, None, 0, 0, out, out, out, out, out, None, None)
    assert call(rr=None) == N.ERR_ARG and "ring is NULL" in err()
    assert call() == N.ERR_ARG and "ABI mismatch" in err()
    r.struct_bytes = C.sizeof(N.RisVecSarlRollout)
    assert call() == N.ERR_ARG and "ring.state_memory is NULL" in err()
    for k in ("state_memory", "action_memory", "reward_memory", "new_state_memory", "terminal_memory"):
        setattr(r, k, fake)
    assert call() == N.ERR_SHAPE and "mem_size" in err()
    r.mem_size = 8
    assert call(S=0) == N.ERR_SHAPE and call(B=0) == N.ERR_SHAPE
    assert call(mm=0) == N.ERR_ARG and "empty buffer" in err()
    assert call(mm=9) == N.ERR_ARG
    assert call(out=None) == N.ERR_ARG and "states is NULL" in err()


def test_python_surface_without_a_gpu():
    n = rv.OUNoise(3, 6, device="cpu", seed=4, env_offset=2)
    assert tuple(n.x.shape) == (3, 6) and n.x.dtype.is_floating_point and not n.x.any()
    assert (n.sigma, n.theta, n.dt, n.mu) == (0.15, 0.2, 1e-2, 0.0)            # noise.py:4
    n.x += 1
    sd = n.state_dict()
    n.reset()
    assert not n.x.any()
    m = rv.OUNoise(3, 6, device="cpu")
    m.load_state_dict(sd)
    assert (m.x == 1).all() and (m.seed, m.env_offset) == (4, 2)
    with pytest.raises(RuntimeError):
        rv.SarlReplayBuffer(16, 10, 56, 8, device="cpu")                          # no CPU fallback


# The GPU tests leave out samples within 2e-5 of a branch of step() (DataBuf hitting zero, over_data crossing 2) and
# demand that at least 98 % stay.  How many does the float64 oracle alone put there, on the same distribution of inputs
# (reset by the same Philox draws, mu ~ U(-1, 1), OU noise, six steps)?  The margins are O(1) kbit quantities with a
# smooth density, so about 2 x 4e-5 x (samples) / (a few kbit): a handful at most, far below the 2 % allowance.
@pytest.mark.parametrize("E,V,M", [(777, 8, 40), (130, 4, 16), (301, 8, 22), (97, 16, 120), (33, 8, 256), (65, 16, 64)])
def test_oracle_alone_leaves_out_next_to_nothing(E, V, M):
    rng = np.random.default_rng(1000 * V + M)
    A, sp = 2 * V + M, orc.SarlParams()
    ids = np.arange(E)
    spawn, buf0 = orc.philox_reset(ids, V, 1, 21)
    pos, _, _, buf = orc.reset(spawn, buf0, orc.default_lanes())
    dist, _, h_r = orc.geometry(pos, M)
    b = orc.phase_R(M)
    x = np.zeros((E, A))
    near = total = 0
    for k in range(6):
        mu = rng.uniform(-1, 1, (E, A)).astype(np.float32).astype(np.float64)
        x = x + 0.2 * (0.0 - x) * 1e-2 + 0.15 * math.sqrt(1e-2) * rng.standard_normal((E, A))
        power, phase = orc.sarl_action_map(mu + x, V, M)
        gain = orc.gain_free(np.exp(1j * phase), h_r, b, dist)
        o = orc.sarl_step(buf, gain, power, orc.philox_arrivals(ids, V, k, 21, sp.rate), sp)
        near += int(((np.abs(o["margin"]["buf"]) < 2e-5) | (np.abs(o["margin"]["over"]) < 2e-5)).sum())
        total += o["reward"].size
        buf = o["data_buf"]
        assert np.isfinite(o["reward_mean"]).all()
    assert near <= max(2, 1e-3 * total), (near, total)
