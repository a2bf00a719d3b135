"""CPU-side tests (no GPU): the C-ABI library loads and exports every symbol
include/risvec.h declares, host logic (YAML key map, NOMA-group encoding, facade
surface, sharding) behaves like the reference's driver expects, and the product
fails loudly without a HIP device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ris_vec_marl_amd as rv
from ris_vec_marl_amd import _native as N
from oracle import risvec_oracle as orc
from oracle import noma_oracle as orc_noma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_YAML_EFFECTIVE = dict(w_d=1.0, w_e=1.0, rate=1.0, f_local_max=3.0e9, cycles_per_bit=300.0, bandwidth=5.0,
                          P_max=2.0, power_scale=0.7, cpu_share_floor=0.10, f_edge_max=2.0e9, k=1e-28,
                          qos_enable=True, R_min_bpsHz=0.15, D_max_s=0.12, qos_penalty=1.5)
# the shipped config.yaml keys that reach the env (data, not reference source)
SHIPPED_YAML = dict(mec=dict(f_local_max=3.0e9, cycles_per_bit=300), phy=dict(bandwidth_MHz=5, P_max=2.0),
                    env=dict(rate=1), reward=dict(sample=False, w_d_fixed=1.0, w_e_fixed=1.0, norm_beta=0.9),
                    qos_enable=True, qos_penalty=1.5, env_refresh_every=5, seed=42, entropy_scale=0.5)


def make_facade(V=8, M=40):
    L = rv.reference_lanes()
    return rv.Environ(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3)


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "risvec.h")).read()
    declared = set(re.findall(r"\b(risvec_[a-z0-9_]+)\s*\(", header))
    declared.discard("risvec_stream_t")
    assert declared == set(N.EXPORTS), declared ^ set(N.EXPORTS)
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name)
    assert lib.risvec_abi_version() == N.ABI_VERSION
    m = re.search(r"#define RISVEC_ABI_VERSION (\d+)", header)
    assert int(m.group(1)) == N.ABI_VERSION


def test_struct_layout_and_default_params_match_python():
    lib = N.load()
    p = N.RisVecParams()
    lib.risvec_default_params(C.byref(p))
    assert p.struct_bytes == C.sizeof(N.RisVecParams)
    L = rv.reference_lanes()
    q = rv.EnvParams().to_c(L, 400, 400)
    for name, _ in N.RisVecParams._fields_:
        a, b = getattr(p, name), getattr(q, name)
        if hasattr(a, "__len__"):
            np.testing.assert_allclose(list(a), list(b), rtol=2e-6, err_msg=name)
        else:
            assert a == pytest.approx(b, rel=1e-6), name
    # product table == oracle table, bit for bit (the GPU arrivals test relies on it)
    for lam in (1.0, 3.0, 0.25, 7.5):
        assert np.array_equal(rv.poisson_cdf_table(lam), orc.poisson_cdf_table(lam))
    with pytest.raises(ValueError):
        rv.poisson_cdf_table(40.0)


def test_api_rejects_bad_arguments_without_touching_a_gpu():
    lib = N.load()
    p = N.RisVecParams()
    lib.risvec_default_params(C.byref(p))
    s = N.RisVecState()
    assert lib.risvec_step(C.byref(s), C.byref(p), None, None, None, None, 0, 0, 0, None) == N.ERR_ARG
    s.abi_version, s.struct_bytes = N.ABI_VERSION, C.sizeof(N.RisVecState)
    s.n_envs, s.n_veh, s.n_ris, s.control_bit = 4, 100, 16, 3
    assert lib.risvec_gain(C.byref(s), C.byref(p), None) == N.ERR_SHAPE
    assert b"n_veh" in lib.risvec_last_error()
    s.n_veh = 8
    assert lib.risvec_gain(C.byref(s), C.byref(p), None) == N.ERR_ARG          # NULL device pointers
    assert b"NULL" in lib.risvec_last_error()
    with pytest.raises(ValueError):
        N.check(N.ERR_ARG)
    # the two T-step entry points validate before they launch: n_steps, flags, NULL inputs
    for fn in (lib.risvec_step_fused_multi, lib.risvec_step_multi):
        assert fn(C.byref(s), None, 4, None, None, None, None, 0, 0, 0, None, None) == N.ERR_ARG       # params NULL
        assert fn(C.byref(s), C.byref(p), 0, None, None, None, None, 0, 0, 0, None, None) == N.ERR_ARG
        assert b"n_steps" in lib.risvec_last_error()
        assert fn(C.byref(s), C.byref(p), 4, None, None, None, None, 0, 0, N.STEP_REUSE_IDX, None, None) == N.ERR_ARG
        assert fn(C.byref(s), C.byref(p), 4, None, None, None, None, 0, 0, 0, None, None) == N.ERR_ARG  # NULL actions
        assert b"NULL" in lib.risvec_last_error()


def test_yaml_key_map_matches_reference_effective_values():
    env = make_facade()
    # class defaults first (Environment.py:57-190)
    assert (env.w_d, env.w_e, env.rate, env.P_max, env.bandwidth) == (0.5, 3.0, 3, 1.0, 1.0)
    assert env.noise_power == pytest.approx(3.981071705534986e-15, rel=1e-12)
    rv.apply_yaml_config(env, SHIPPED_YAML)
    for k, v in REF_YAML_EFFECTIVE.items():
        assert getattr(env, k) == pytest.approx(v), k
    assert env.noise_power == pytest.approx(1.990535852767493e-14, rel=1e-12)
    assert env.bandwidth_hz == 5e6 and env.channel_model == "free"
    # without a YAML the driver's Config defaults apply (marl_train_bcd.py:426-427, 505-508, 750-753)
    env2 = make_facade()
    rv.apply_yaml_config(env2, None)
    assert (env2.w_d, env2.w_e, env2.qos_penalty, env2.R_min_bpsHz, env2.D_max_s) == (1.0, 2.0, 5.0, 0.15, 0.12)
    # oracle's notion of the effective parameters agrees with the product's
    p = orc.OracleParams.yaml_effective()
    for a, b in (("bandwidth", "bandwidth"), ("noise_power", "noise_power"), ("P_max", "P_max"), ("w_d", "w_d"),
                 ("w_e", "w_e"), ("rate", "rate"), ("f_local_max", "f_local_max"), ("cycles_per_bit", "cycles_per_bit"),
                 ("R_min_bpsHz", "R_min_bpsHz"), ("D_max_s", "D_max_s"), ("qos_penalty", "qos_penalty")):
        assert getattr(p, a) == pytest.approx(getattr(env, b)), a


def test_params_reach_the_c_struct():
    env = make_facade()
    rv.apply_yaml_config(env, SHIPPED_YAML)
    c = env._vec._p()
    assert c.bandwidth_mhz == 5.0 and c.p_max == 2.0 and c.cycles_per_bit == 300.0
    assert c.noise_power == pytest.approx(1.990535852767493e-14, rel=1e-6)
    v0 = env.params.version
    env.w_d = 0.25
    assert env.params.version > v0 and env._vec._p().w_d == 0.25
    assert list(c.lanes_up)[:4] == rv.reference_lanes()["up_lanes"]


def test_encode_noma_groups():
    groups = [[0, 3], [5, 2], [1], [4], [6, 7, 1]]           # the last group is ignored but counted
    partner, ng = rv.encode_noma_groups([groups], 8)
    want, n = orc.encode_groups(groups[:-1], 8)
    assert ng[0] == 5 and n == 4
    assert np.array_equal(partner[0], want)
    assert partner[0, 0] == 3 and partner[0, 3] == 0 + (1 << 16) and partner[0, 1] == -1 and partner[0, 6] == -2
    # a vehicle listed twice: the last group that lists it decides (Environment.py:344-369; pinned by
    # tests/golden/facade_groups_8.npz), its earlier partner keeps the pair entry
    p1, n1 = rv.encode_noma_groups([[[0, 1], [1]]], 8)
    assert p1[0, 0] == 1 and p1[0, 1] == -1 and n1[0] == 2
    with pytest.raises(ValueError):
        rv.encode_noma_groups([[[0, 9]]], 8)
    p2, n2 = rv.encode_noma_groups([[], [[2]]], 4)
    assert n2.tolist() == [0, 1] and (p2[0] == -2).all()


def test_facade_surface_matches_reference_inventory():
    """names a driver may touch on `Environ`."""
    env = make_facade()
    methods = ["Random_phase", "add_new_vehicles", "add_new_vehicles_by_number", "compute_data_rate", "compute_parms",
               "get_channel_gains", "get_next_phase", "get_path_loss", "get_shadowing", "localProcRev", "make_new_game",
               "optimize_compute_objective_function", "optimize_phase_shift", "renew_positions", "step",
               "update_channel_gains"]
    for m in methods:
        assert callable(getattr(env, m)), m
    host_attrs = ["down_lanes", "up_lanes", "left_lanes", "right_lanes", "width", "height", "n_veh", "M", "control_bit",
                  "possible_angles", "distance_B_R", "angle_B_R", "channel_model", "fc_GHz", "bandwidth", "bandwidth_hz",
                  "N0_dBm_per_Hz", "N0_W_per_Hz", "noise_power", "P_max", "shadow_std_los", "shadow_std_nlos",
                  "rician_K_dB", "Decorrelation_distance", "V2I_Shadowing", "V2I_pathloss", "V2I_channels_abs",
                  "delta_distance", "sig2_dB", "sig2", "bsAntGain", "bsNoiseFigure", "vehAntGain", "vehNoiseFigure",
                  "time_slow", "time_fast", "k", "L", "f_local_max", "f_edge_max", "cycles_per_bit", "cpu_share_floor",
                  "power_scale", "qos_enable", "R_min_bpsHz", "D_max_s", "qos_penalty", "w_d", "w_e", "reward_clip",
                  "sample_weights", "w_d_range", "w_e_range", "w_fair_range", "w_fair", "reward_scale",
                  "reward_norm_beta", "delay_mean", "delay_var", "energy_mean", "energy_var", "rate", "data_buf_size",
                  "data_r", "phase_R", "elements_phase_shift_real", "last_off_kbit_sum", "last_local_kbit_sum",
                  "last_mec_queue_cycles"]
    for a in host_attrs:
        assert hasattr(env, a), a
    assert env.distance_B_R == pytest.approx(311.1269837220809) and env.angle_B_R == pytest.approx(0.7071067811865475)
    assert len(env.possible_angles) == 8 and env.phase_R.shape == (40,)
    np.testing.assert_allclose(env.phase_R, orc.phase_R(40), atol=1e-15)
    # device-backed names exist on the class (they need a GPU to be read)
    for a in ["DataBuf", "data_t", "data_p", "over_data", "vehicle_rate", "channel_gains", "distances_R_i",
              "angles_R_i", "mec_queue_cycles", "elements_phase_shift_complex", "phases_R_i", "vehicles"]:
        assert isinstance(getattr(type(env), a), property), a
    # created lazily by step() in the reference: absent until then (driver uses getattr(..., None))
    assert getattr(env, "last_delay_mean", None) is None
    assert getattr(env, "last_qos_violation", None) is None


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_cpu_fallback():
    env = make_facade()
    for call in (env.make_new_game, env.renew_positions, env.compute_parms, env.optimize_phase_shift,
                 env.update_channel_gains, lambda: env.step(np.zeros((2, 8)), [[0]]), lambda: env.DataBuf):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for dead in (lambda: env.get_path_loss([0, 0]), lambda: env.localProcRev(1.0)):
        with pytest.raises(NotImplementedError):
            dead()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "ris_vec_marl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f
                assert "/root/reference" not in src, f


def test_shard_range():
    for n, w in ((65536, 8), (10, 3), (7, 8), (32768, 1)):
        spans = [rv.dist.shard_range(n, r, w) for r in range(w)]
        assert spans[0][0] == 0 and sum(c for _, c in spans) == n
        for (s0, c0), (s1, _) in zip(spans, spans[1:]):
            assert s0 + c0 == s1
        assert max(c for _, c in spans) - min(c for _, c in spans) <= 1
    with pytest.raises(ValueError):
        rv.dist.shard_range(8, 8, 8)


def test_noma_and_replay_abi_without_a_gpu():
    """f2 / f3 entry points: struct layouts agree between ctypes and the library (the C defaults land
    in the right Python fields), and bad arguments are rejected before anything is launched."""
    lib = N.load()
    for V in (4, 8, 16):
        p = N.RisVecNomaParams()
        lib.risvec_noma_default_params(C.byref(p), V)
        q = rv.NomaConfig(V).to_c(noise_power=10 ** (-174 / 10) / 1000 * 1e6, P_max=1.0)
        for name, _ in N.RisVecNomaParams._fields_:
            a, b = getattr(p, name), getattr(q, name)
            assert a == pytest.approx(b, rel=1e-6) or (a == b), (V, name, a, b)
    ns = N.RisVecNomaState()
    p = rv.NomaConfig(8).to_c(1e-14, 1.0)
    assert lib.risvec_noma_begin_episode(None, None) == N.ERR_ARG
    ns.n_envs, ns.n_veh = 4, 17
    assert lib.risvec_noma_mask(C.byref(ns), None, None, 0.5, 3, None) == N.ERR_SHAPE
    assert b"n_veh" in lib.risvec_last_error()
    ns.n_veh = 8
    assert lib.risvec_noma_mask(C.byref(ns), None, None, 0.5, 3, None) == N.ERR_ARG        # NULL gain
    assert lib.risvec_noma_group(C.byref(ns), C.byref(p), None, None, None, 0, 3, None, None, 1, 0, None, 0, 0, None,
                                 None) == N.ERR_ARG
    assert lib.risvec_noma_flush(C.byref(ns), None, None) == N.ERR_ARG
    # scratch: none up to 8 vehicles; beyond, the list of envs the first launch leaves to the second (16 B + an int per env)
    assert lib.risvec_noma_scratch_bytes(32768, 8) == 0
    assert lib.risvec_noma_scratch_bytes(32768, 16) == 16 + 4 * 32768 + 240
    assert lib.risvec_noma_scratch_bytes(17, 9) == 256
    assert lib.risvec_noma_scratch_bytes(0, 16) == 0 and lib.risvec_noma_scratch_bytes(8, 17) == 0
    rb = N.RisVecReplay()
    assert lib.risvec_replay_store(C.byref(rb), 0, 1, None, None, None, 1, None, None, None, 0, None, None, None) \
        == N.ERR_SHAPE
    rb.n_agents, rb.input_shape, rb.n_actions, rb.mem_size = 8, 5, 10, 100
    assert lib.risvec_replay_store(C.byref(rb), 0, 1, None, None, None, 1, None, None, None, 0, None, None, None) \
        == N.ERR_ARG
    assert lib.risvec_replay_sample(C.byref(rb), 0, 4, None, 0, 0, None, None, None, None, None, None, None, None,
                                    None) == N.ERR_ARG
    assert lib.risvec_marshal_actions(0, 8, None, None, 0.1, None, None, None, None) == N.ERR_SHAPE
    assert lib.risvec_marshal_actions(4, 8, None, None, 0.1, None, None, None, None) == N.ERR_ARG
    with pytest.raises(NotImplementedError):
        c = rv.NomaConfig(8); c.use_mwm_primary = False; c.to_c(1e-14, 1.0)


def test_noma_config_reads_the_drivers_yaml_keys():
    """NomaConfig.apply_yaml takes the same keys from the same places as marl_train_bcd.py:575,
    639-660, 716-741; values below are the shipped config.yaml's (its lines 39-44, 53, 78-83, 116-120, 144-148)."""
    y = {"min_pair_target": 3, "use_mwm_primary": True, "mwm_accept_quantile": 0.10, "mwm_backoff_rounds": 3,
         "mwm_accept_q_step": 0.05, "qos_enable": True, "freeze_group_in_episode": True, "freeze_recalc_every": 0,
         "freeze_unstick_prob": 0.0, "freeze_reward_drop_ratio": 0.05,
         "reward": {"mask_enable": True, "mask_topk_start": 7, "mask_topk_end": 7, "mask_tau_q_start": 0.10,
                    "mask_tau_q_end": 0.25, "pairing_threshold_quantile": 0.25}}
    c = rv.NomaConfig(8).apply_yaml(y)
    o = orc_noma.NomaParams.yaml_effective(8)
    for k in ("min_pair_target", "mwm_accept_quantile", "mwm_backoff_rounds", "mwm_accept_q_step", "qos_enable",
              "qos_R_min_bpsHz", "mask_topk_start", "mask_topk_end", "mask_tau_q_start", "mask_tau_q_end",
              "pairing_threshold_quantile", "freeze_group_in_episode", "freeze_recalc_every"):
        assert getattr(c, k) == getattr(o, k), k
    assert c.mask_schedule(50) == orc_noma.mask_schedule(o, 50, 8)
    assert rv.anneal_topk(37, 8, 7, 4, 200) == orc_noma.anneal_topk(37, 8, 7, 4, 200)


def test_policy_abi_without_a_gpu():
    lib = N.load()
    assert lib.risvec_policy_sample(0, 8, 0, None, None, None, None, None, None, 0, 0, 0.1, None, None, None, None, None,
                                    None, None) == N.ERR_SHAPE
    assert lib.risvec_policy_sample(4, 8, 0, None, None, None, None, None, None, 0, 0, 0.1, None, None, None, None, None,
                                    None, None) == N.ERR_ARG
    assert lib.risvec_policy_layer1(4, 8, 5, 4096, None, None, None, None, None, None, None) == N.ERR_SHAPE
    assert b"f1" in lib.risvec_last_error()
    assert lib.risvec_policy_layer1(4, 8, 5, 512, None, None, None, None, None, None, None) == N.ERR_ARG
    assert lib.risvec_policy_heads(4, 8, 256, 12, None, None, None, None, None, None, None, None) == N.ERR_ARG
    assert lib.risvec_policy_heads(4, 8, 1024, 68, None, None, None, None, None, None, None, None) == N.ERR_SHAPE   # > 64 KB of LDS


def test_episode_abi_without_a_gpu():
    lib = N.load()
    assert lib.risvec_episode_partial_rows(0) == 0 and lib.risvec_episode_partial_rows(1) == 1
    assert lib.risvec_episode_partial_rows(256) == 1 and lib.risvec_episode_partial_rows(32768 + 1) == 129
    assert lib.risvec_episode_clear(0, 8, None, None) == N.ERR_SHAPE
    assert lib.risvec_episode_clear(4, 65, None, None) == N.ERR_SHAPE
    assert lib.risvec_episode_clear(4, 8, None, None) == N.ERR_ARG and b"acc" in lib.risvec_last_error()
    assert lib.risvec_episode_clear(1 << 27, 8, None, None) == N.ERR_SHAPE          # E * (17 + V) >= 2^31
    assert lib.risvec_episode_accumulate(4, 8, None, None, None, 5.0, None, None) == N.ERR_ARG
    assert lib.risvec_episode_accumulate(4, 8, 16, 16, None, 5.0, 8, None) == N.ERR_ARG      # acc not 16-byte aligned
    assert lib.risvec_episode_accumulate(4, 8, 16, 16, None, -1.0, 16, None) == N.ERR_ARG and b"user_clip" in lib.risvec_last_error()
    assert lib.risvec_episode_accumulate(4, 8, 16, 16, None, float("nan"), 16, None) == N.ERR_ARG
    assert lib.risvec_episode_summary(4, 8, 0, 16, 16, None, 16, 16, None) == N.ERR_ARG and b"n_steps" in lib.risvec_last_error()
    assert lib.risvec_episode_summary(4, 8, 3, 16, 16, None, None, 16, None) == N.ERR_ARG


def test_policy_split16_abi_without_a_gpu():
    lib = N.load()
    assert lib.risvec_policy_layer1_split16(4, 8, 5, 510, None, None, None, None, None, None, None) == N.ERR_SHAPE
    assert lib.risvec_policy_layer1_split16(4, 8, 9, 512, None, None, None, None, None, None, None) == N.ERR_SHAPE
    assert lib.risvec_policy_layer1_split16(4, 8, 5, 512, None, None, None, None, None, None, None) == N.ERR_ARG


def _kernel(E, V, M, flags=0, form=N.FORM_FUSED):
    s = N.RisVecState(abi_version=N.ABI_VERSION, struct_bytes=C.sizeof(N.RisVecState), n_envs=E, n_veh=V, n_ris=M,
                      control_bit=3)
    return N.step_kernel(s, flags, form)


# DESIGN.md 3.1 / plan_step(): each rule on both sides of its boundary.  Without a device tuning() takes the MI355X
# values: 256 CUs, a 256 MiB Infinity Cache (IC).  Stream = h_r + theta per step = E (8VM + 8M): 4 608 B per env at 8 x 64.
DISPATCH_TABLE = [
    # lat vs pipe at 8 x 64 and 4 x 16: 24 wavefronts of 4 envs per CU; 16 x 64: 8
    ((24576, 8, 64), "k_step_fused_lat<8,64,4>"),
    ((24577, 8, 64), "k_step_fused_pipe<8,64,2,MarlCore>"),
    ((24576, 4, 16), "k_step_fused_lat<4,16,4>"),
    ((24577, 4, 16), "k_step_fused_pipe<4,16,4,MarlCore>"),
    ((8192, 16, 64), "k_step_fused_lat<16,64,4>"),
    ((8193, 16, 64), "k_step_fused_pipe<16,64,2,MarlCore>"),
    ((100000, 8, 36), "k_step_fused_lat<8,36,4>"),                # M = 36 / 40: the latency-shaped kernel at every size
    ((90000, 8, 40), "k_step_fused_lat<8,40,4>"),
    # envs per wavefront: the largest of {4, 2, 1} with >= 8 wavefronts per CU (2 048 on 256 CUs)
    ((8192, 8, 36), "k_step_fused_lat<8,36,4>"),
    ((8191, 8, 36), "k_step_fused_lat<8,36,2>"),
    ((4096, 8, 36), "k_step_fused_lat<8,36,2>"),
    ((4095, 8, 36), "k_step_fused_lat<8,36,1>"),
    ((4095, 16, 256), "k_step_fused_lat<16,256,1>"),              # 16 x 256: one env per wavefront at every size
    ((4096, 16, 256), "k_step_fused_lat<16,256,1>"),
    # the stream against the IC (58 254 envs = 268 434 432 B <= 256 MiB < 58 255 envs) and 1.29 IC (75 147 / 75 148 envs)
    ((58254, 8, 64), "k_step_fused_pipe<8,64,2,MarlCore>"),
    ((58255, 8, 64), "k_step_fused_lat<8,64,4,ALT>"),
    ((75147, 8, 64), "k_step_fused_lat<8,64,4,ALT>"),
    ((75148, 8, 64), "k_step_fused_lat<8,64,4,NT>"),
    ((262144, 8, 64), "k_step_fused_lat<8,64,4,NT>"),
    ((58254, 8, 36), "k_step_fused_lat<8,36,4>"),                 # 8 x 36: 2 592 B per env -> IC at 103 563 / 103 564 envs
    ((103563, 8, 36), "k_step_fused_lat<8,36,4>"),
    ((103564, 8, 36), "k_step_fused_lat<8,36,4,ALT>"),
    ((133598, 8, 36), "k_step_fused_lat<8,36,4,NT>"),
    ((32768, 16, 256), "k_step_fused_lat<16,256,1,NT>"),
    # run-time M: the (V, G, NIT) member, envs per wavefront clamped to it
    ((32768, 8, 20), "k_step_fused_lat<8,M=20(G=16,NIT=1),4>"),
    ((3001, 8, 20), "k_step_fused_lat<8,M=20(G=16,NIT=1),2>"),
    ((2049, 8, 256), "k_step_fused_lat<8,M=256(G=64,NIT=2),2>"),
    ((16384, 16, 120), "k_step_fused_lat<16,M=120(G=64,NIT=1),2>"),
    ((515, 16, 120), "k_step_fused_lat<16,M=120(G=64,NIT=1),1>"),
    ((1027, 16, 200), "k_step_fused_lat<16,M=200(G=64,NIT=2),1>"),
    ((4100, 4, 100), "k_step_fused_lat<4,M=100(G=64,NIT=1),2>"),
    ((16384, 8, 120), "k_step_fused_lat<8,M=120(G=64,NIT=1),4>"),
    ((32768, 8, 120), "k_step_fused_lat<8,M=120(G=64,NIT=1),4,ALT>"),
    # outside the family: the generic kernel
    ((130, 5, 21), "k_step_fused<8,32,1>"),
    ((1000, 8, 63), "k_step_fused<8,64,1>"),
    ((1000, 8, 300), "k_step_fused<8,64,2>"),
    ((1000, 32, 64), "k_step_fused<32,32,2>"),
    ((1000, 2, 64), "k_step_fused<2,32,2>"),
]


@pytest.mark.parametrize("shape,name", DISPATCH_TABLE)
def test_dispatch_table(shape, name):
    assert _kernel(*shape) == name


def test_dispatch_table_forms_flags_and_overrides():
    K = _kernel
    # theta by index: the EMAX member's TK form, NT / ALT by stream size as the plain step
    assert K(300, 8, 64, N.STEP_THETA_BY_INDEX) == "k_step_fused_lat<8,64,4,TK>"
    assert K(32768, 8, 64, N.STEP_THETA_BY_INDEX) == "k_step_fused_lat<8,64,4,TK>"
    assert K(58255, 8, 64, N.STEP_THETA_BY_INDEX) == "k_step_fused_lat<8,64,4,ALT,TK>"
    assert K(75148, 8, 64, N.STEP_THETA_BY_INDEX) == "k_step_fused_lat<8,64,4,NT,TK>"
    assert K(32768, 16, 256, N.STEP_THETA_BY_INDEX) == "k_step_fused_lat<16,256,1,NT,TK>"
    assert K(257, 8, 100, N.STEP_THETA_BY_INDEX) == "k_step_fused_lat<8,M=100(G=64,NIT=1),4,TK>"
    assert K(40000, 16, 64, N.STEP_THETA_BY_INDEX) == "k_step_fused_lat<16,64,4,TK>"         # 16 x 64 never NT
    assert K(300, 8, 300, N.STEP_THETA_BY_INDEX) is None
    # steering: while one wavefront's theta rows fit 64 KB of LDS (8 envs x (M + 1) at V = 8: float64 up to M = 79)
    assert K(1000, 8, 79, N.STEP_STEER) == "k_step_steer<8,wide>"
    assert K(1000, 8, 80, N.STEP_STEER) == "k_step_steer<8,narrow>"
    assert K(1000, 8, 1023, N.STEP_STEER) == "k_step_steer<8,narrow>"
    assert K(1000, 8, 1024, N.STEP_STEER) == "k_step_fused<8,64,2>"
    assert K(32768, 16, 256, N.STEP_STEER) == "k_step_steer<16,narrow>"
    assert K(1000, 1, 128, N.STEP_STEER) == "k_step_fused<1,64,2>"                          # 64 envs x 129 > 64 KB
    # cached, ring and T-step forms
    assert K(32768, 8, 64, form=N.FORM_CACHED) == "k_step<8>"
    assert K(130, 5, 21, form=N.FORM_CACHED) == "k_step<8>"
    assert K(1000, 16, 64, form=N.FORM_CACHED_RING) == "k_step<16,RING>"
    assert K(1000, 5, 21, form=N.FORM_CACHED_RING) == "k_step<8,RING>"
    assert K(1000, 2, 64, form=N.FORM_CACHED_RING) is None
    assert K(32768, 8, 64, form=N.FORM_FUSED_RING) == "k_step_fused_pipe<8,64,2,MarlCore+ring>"
    assert K(1000, 4, 16, form=N.FORM_FUSED_RING) == "k_step_fused_pipe<4,16,4,MarlCore+ring>"
    assert K(61458, 8, 64, form=N.FORM_FUSED_RING) == "k_step_fused_pipe<8,64,2,MarlCore+ring>"   # 1.055 IC
    assert K(61459, 8, 64, form=N.FORM_FUSED_RING) == "k_step_fused_pipe<8,64,2,MarlCore+ring,NT>"
    assert K(1000, 8, 100, form=N.FORM_FUSED_RING) is None
    assert K(8192, 8, 64, form=N.FORM_FUSED_MULTI) == "k_step_fused_lat<8,64,8,MULTI>"
    assert K(8191, 8, 64, form=N.FORM_FUSED_MULTI) == "k_step_fused_lat<8,64,4,MULTI>"
    assert K(4096, 8, 36, form=N.FORM_FUSED_MULTI) == "k_step_fused_lat<8,36,4,MULTI>"
    assert K(4095, 8, 36, form=N.FORM_FUSED_MULTI) == "k_step_fused_lat<8,36,2,MULTI>"
    assert K(1024, 8, 40, form=N.FORM_FUSED_MULTI) == "k_step_fused_lat<8,40,1,MULTI>"
    assert K(8192, 4, 16, form=N.FORM_FUSED_MULTI) == "k_step_fused_lat<4,16,8,MULTI>"
    assert K(8192, 16, 64, form=N.FORM_FUSED_MULTI) is None
    assert K(8192, 8, 20, form=N.FORM_FUSED_MULTI) is None
    # the test / A/B override, and the rules again after it
    with N.forced(lat=False):
        assert K(2100, 8, 64) == "k_step_fused_pipe<8,64,2,MarlCore>"
        assert K(300, 16, 256) == "k_step_fused_pipe<16,256,2,MarlCore>"
        assert K(262144, 8, 64) == "k_step_fused_pipe<8,64,2,MarlCore,NT>"
        assert K(1500, 8, 80) == "k_step_fused_lat<8,M=80(G=64,NIT=1),2>"              # no pipeline: stays
        assert K(300, 8, 64, N.STEP_THETA_BY_INDEX) == "k_step_fused_lat<8,64,4,TK>"
    with N.forced(lat=True):
        assert K(32768, 8, 64) == "k_step_fused_lat<8,64,4>"
    with N.forced(lat=False, pipe_nt=True):
        assert K(2100, 8, 64) == "k_step_fused_pipe<8,64,2,MarlCore,NT>"
    with N.forced(pipe_nt=False):
        assert K(61459, 8, 64, form=N.FORM_FUSED_RING) == "k_step_fused_pipe<8,64,2,MarlCore+ring>"
    with N.forced(lat_epw=1):
        assert K(3001, 8, 20) == "k_step_fused_lat<8,M=20(G=16,NIT=1),2>"             # clamped to the member
        assert K(9000, 8, 40) == "k_step_fused_lat<8,40,1>"
    with N.forced(lat_epw=4):
        assert K(3001, 8, 20) == "k_step_fused_lat<8,M=20(G=16,NIT=1),4>"
    with N.forced(lat_nt=True):
        assert K(1500, 8, 36) == "k_step_fused_lat<8,36,4,NT>"
        assert K(2050, 16, 64) == "k_step_fused_lat<16,64,1>"
    with N.forced(lat_nt=False):
        assert K(262144, 8, 64) == "k_step_fused_pipe<8,64,2,MarlCore,NT>"             # above the band: the pipeline
    with N.forced(lat_alt=True):
        assert K(2100, 8, 64) == "k_step_fused_lat<8,64,4,ALT>"
    with N.forced(lat_alt=False):
        assert K(65536, 8, 64) == "k_step_fused_pipe<8,64,2,MarlCore,NT>"
    assert K(2100, 8, 64) == "k_step_fused_lat<8,64,1>"
    with pytest.raises(TypeError):
        with N.forced(lat_ept=1):
            pass
    with pytest.raises(ValueError):
        with N.forced(lat_epw=3):
            pass
    assert K(0, 8, 64) is None and b"n_envs" in N.load().risvec_last_error()
    assert K(100, 8, 64, form=7) is None
