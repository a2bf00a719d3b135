"""The fused 3GPP step family on the host (no GPU): ABI version, exports, argument rejection of
risvec_step_fused_3gpp / _multi before any launch, and the selector's names for the 3GPP members
(risvec_step_kernel with RISVEC_STEP_3GPP) next to the unchanged answers without that bit."""
import ctypes as C
import os
import re

import pytest

from ris_vec_marl_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20            # a 16-byte aligned address the host never dereferences (every call below fails before a launch)


def _state(E=64, V=8, M=64):
    s = N.RisVecState(abi_version=N.ABI_VERSION, struct_bytes=C.sizeof(N.RisVecState), n_envs=E, n_veh=V, n_ris=M,
                      control_bit=3)
    for name, _ in N.RisVecState._fields_:
        if name not in ("abi_version", "struct_bytes", "n_envs", "n_veh", "n_ris", "control_bit", "env_offset"):
            setattr(s, name, FAKE)
    return s


def _params():
    p = N.RisVecParams()
    N.load().risvec_default_params(C.byref(p))
    return p


def _step3(s, p, model=N.CH_3GPP_UMI, fading=None, flags=N.STEP_METRICS, ring=None):
    return N.load().risvec_step_fused_3gpp(C.byref(s), C.byref(p) if p is not None else None, model, FAKE, FAKE, FAKE,
                                           None, C.byref(fading) if fading is not None else None, 7, 0, 1, flags,
                                           C.byref(ring) if ring is not None else None, None)


def _multi3(s, p, n_steps=3, model=N.CH_3GPP_UMI, fading=None, flags=N.STEP_METRICS):
    return N.load().risvec_step_fused_3gpp_multi(C.byref(s), C.byref(p), model, n_steps, FAKE, FAKE, FAKE, None,
                                                 C.byref(fading) if fading is not None else None, 7, 0, 1, None, flags,
                                                 None)


def _err():
    return N.load().risvec_last_error().decode()


def test_abi_version_17_everywhere():
    header = open(os.path.join(ROOT, "include", "risvec.h")).read()
    assert int(re.search(r"#define RISVEC_ABI_VERSION (\d+)", header).group(1)) == 17 == N.ABI_VERSION
    assert N.load().risvec_abi_version() == 17
    assert re.search(r"RISVEC_STEP_3GPP = (\d+)", header).group(1) == str(N.STEP_3GPP) == "512"


def test_new_symbols_are_exported():
    lib = N.load()
    for name in ("risvec_step_fused_3gpp", "risvec_step_fused_3gpp_multi"):
        assert name in N.EXPORTS
        assert hasattr(lib, name)
    assert [f for f, _ in N.RisVecFading._fields_] == ["u_los", "z_shadow", "small"]


def test_argument_rejection_without_a_gpu():
    s, p = _state(), _params()
    assert _step3(s, None) == N.ERR_ARG and "params is NULL" in _err()
    assert _step3(s, p, model=N.CH_FREE) == N.ERR_ARG and "model=0" in _err()
    assert _step3(s, p, model=7) == N.ERR_ARG
    for part in ((FAKE, None, None), (FAKE, FAKE, None), (None, None, FAKE)):
        assert _step3(s, p, fading=N.RisVecFading(*part)) == N.ERR_ARG and "all be given" in _err()
        assert _multi3(s, p, fading=N.RisVecFading(*part)) == N.ERR_ARG
    for bad in (N.STEP_STEER, N.STEP_THETA_BY_INDEX, N.STEP_REUSE_COLSUM, N.STEP_REUSE_SSUM, N.STEP_REUSE_IDX,
                N.STEP_3GPP, 1 << 12):
        assert _step3(s, p, flags=N.STEP_METRICS | bad) == N.ERR_ARG and "flags" in _err()
        assert _multi3(s, p, flags=N.STEP_METRICS | bad) == N.ERR_ARG
    assert _multi3(s, p, n_steps=0) == N.ERR_ARG and "n_steps" in _err()
    assert _multi3(s, p, n_steps=(1 << 20) + 1) == N.ERR_ARG
    ring = N.RisVecStepRing()
    for flags in (N.STEP_METRICS, N.STEP_OBS, N.STEP_POLICY_ACTION):
        assert _step3(s, p, flags=flags, ring=ring) == N.ERR_ARG and "POLICY_ACTION | RISVEC_STEP_OBS" in _err()
    s5 = _state(V=5)
    assert _step3(s5, p, flags=N.STEP_POLICY_ACTION | N.STEP_OBS, ring=ring) == N.ERR_UNSUPPORTED
    s.pos = None
    assert _step3(s, p) == N.ERR_ARG and "state.pos" in _err()


def test_existing_step_entry_points_reject_the_3gpp_bit():
    lib = N.load()
    s, p = _state(), _params()
    args = (C.byref(s), C.byref(p), FAKE, FAKE, FAKE, None, 7, 0, N.STEP_METRICS | N.STEP_3GPP, None)
    assert lib.risvec_step(*args) == N.ERR_ARG and "unknown flag" in _err()
    assert lib.risvec_step_fused(*args) == N.ERR_ARG and "unknown flag" in _err()


def _kernel(E, V, M, flags=0, form=N.FORM_FUSED):
    s = N.RisVecState(abi_version=N.ABI_VERSION, struct_bytes=C.sizeof(N.RisVecState), n_envs=E, n_veh=V, n_ris=M,
                      control_bit=3)
    return N.step_kernel(s, flags, form)


@pytest.mark.parametrize("E,V,M,vp", [(32768, 8, 64, 8), (301, 5, 21, 8), (4097, 16, 256, 16), (1000, 4, 16, 4)])
def test_selector_names_the_3gpp_members(E, V, M, vp):
    G = N.STEP_3GPP
    assert _kernel(E, V, M, G, N.FORM_FUSED) == "k_step_3gpp<%d>" % vp
    assert _kernel(E, V, M, G | N.STEP_OBS | N.STEP_POLICY_ACTION, N.FORM_FUSED) == "k_step_3gpp<%d>" % vp
    assert _kernel(E, V, M, G, N.FORM_FUSED_MULTI) == "k_step_3gpp<%d,MULTI>" % vp
    ring = _kernel(E, V, M, G, N.FORM_FUSED_RING)
    assert ring == (None if V == 5 else "k_step_3gpp<%d,RING>" % vp)
    assert _kernel(E, V, M, G, N.FORM_CACHED) is None           # the cached step does not depend on the channel model
    assert _kernel(E, V, M, G, N.FORM_CACHED_RING) is None


def test_any_shape_has_a_3gpp_member():
    for V, M in ((1, 1), (3, 20), (8, 120), (64, 2048), (33, 77)):
        assert _kernel(100, V, M, N.STEP_3GPP) == "k_step_3gpp<%d>" % (1 << (V - 1).bit_length())


def test_answers_without_the_3gpp_bit_are_unchanged():
    # rows of test_host_cpu.DISPATCH_TABLE and of its forms test
    assert _kernel(24576, 8, 64) == "k_step_fused_lat<8,64,4>"
    assert _kernel(24577, 8, 64) == "k_step_fused_pipe<8,64,2,MarlCore>"
    assert _kernel(4095, 16, 256) == "k_step_fused_lat<16,256,1>"
    assert _kernel(75148, 8, 64) == "k_step_fused_lat<8,64,4,NT>"
    assert _kernel(300, 8, 64, N.STEP_THETA_BY_INDEX) == "k_step_fused_lat<8,64,4,TK>"
    assert _kernel(1000, 8, 79, N.STEP_STEER) == "k_step_steer<8,wide>"
    assert _kernel(1000, 8, 64, 0, N.FORM_CACHED) == "k_step<8>"
    assert _kernel(1000, 5, 21, 0, N.FORM_CACHED_RING) == "k_step<8,RING>"
    assert _kernel(100, 8, 64, 0, 7) is None
