"""RISVEC_STEP_THETA_IDX_CURRENT on the host (no GPU): the bit never changes what the selector answers, the entry points
that do not take it -- or take it without what it needs -- refuse it before any launch, and the ABI version stays."""
import ctypes as C
import os
import re

import pytest

from ris_vec_marl_amd import _native as N
from tests.test_host_cpu import DISPATCH_TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20            # a 16-byte aligned address the host never dereferences (every call below fails before a launch)
CUR = N.STEP_THETA_IDX_CURRENT


def _state(E=64, V=8, M=64, control_bit=3, fake=True):
    s = N.RisVecState(abi_version=N.ABI_VERSION, struct_bytes=C.sizeof(N.RisVecState), n_envs=E, n_veh=V, n_ris=M,
                      control_bit=control_bit)
    if fake:
        for name, _ in N.RisVecState._fields_:
            if name not in ("abi_version", "struct_bytes", "n_envs", "n_veh", "n_ris", "control_bit", "env_offset"):
                setattr(s, name, FAKE)
    return s


def _params():
    p = N.RisVecParams()
    N.load().risvec_default_params(C.byref(p))
    return p


def _err():
    return N.load().risvec_last_error().decode()


def test_abi_version_and_the_bit():
    header = open(os.path.join(ROOT, "include", "risvec.h")).read()
    assert N.load().risvec_abi_version() == 17 == N.ABI_VERSION
    assert int(re.search(r"#define RISVEC_ABI_VERSION (\d+)", header).group(1)) == 17
    assert re.search(r"RISVEC_STEP_THETA_IDX_CURRENT = (\d+)", header).group(1) == str(CUR) == "1024"
    assert "risvec_last_theta_by_index" in N.EXPORTS and hasattr(N.load(), "risvec_last_theta_by_index")
    assert N.last_theta_by_index() in (0, 1)


SHAPES = sorted({shape for shape, _ in DISPATCH_TABLE})
FLAGS = (0, N.STEP_METRICS | N.STEP_OBS, N.STEP_STEER, N.STEP_THETA_BY_INDEX, N.STEP_3GPP)
FORMS = (N.FORM_CACHED, N.FORM_FUSED, N.FORM_CACHED_RING, N.FORM_FUSED_RING, N.FORM_FUSED_MULTI)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_bit_never_changes_the_plan(shape):
    """risvec_step_kernel(state, flags | CURRENT, form) == the answer without the bit: every (E, V, M) row of the dispatch
    table, every form (the ring forms included), with and without the flags that do select, under the rules and with the
    forms forced."""
    s = _state(*shape, fake=False)
    for force in (None, dict(lat=False), dict(lat=True), dict(lat=False, pipe_nt=True), dict(lat=False, pipe_nt=False)):
        for form in FORMS:
            for flags in FLAGS:
                if force is None:
                    a, b = N.step_kernel(s, flags, form), N.step_kernel(s, flags | CUR, form)
                else:
                    with N.forced(**force):
                        a, b = N.step_kernel(s, flags, form), N.step_kernel(s, flags | CUR, form)
                assert a == b, (shape, force, form, flags, a, b)


@pytest.mark.parametrize("shape,name", [(sh, nm) for sh, nm in DISPATCH_TABLE if "pipe" in nm])
def test_pipeline_rows_keep_their_name(shape, name):
    s = _state(*shape, fake=False)
    assert N.step_kernel(s, CUR, N.FORM_FUSED) == name


def test_the_bit_is_refused_where_it_does_not_apply():
    lib = N.load()
    p = _params()
    flags = N.STEP_METRICS | CUR

    def step_args(s, fl=flags):
        return (C.byref(s), C.byref(p), FAKE, FAKE, FAKE, None, 7, 0, fl, None)

    # theta_idx is NULL
    s = _state()
    s.theta_idx = None
    assert lib.risvec_step_fused(*step_args(s)) == N.ERR_ARG and "theta_idx" in _err()
    # control_bit != 3
    for cb in (0, 1, 2, 4):
        assert lib.risvec_step_fused(*step_args(_state(control_bit=cb))) == N.ERR_ARG and "control_bit" in _err()
    # the cached entry point
    assert lib.risvec_step(*step_args(_state())) == N.ERR_ARG and "unknown flag" in _err()
    # the T-step entry points
    s = _state()
    for fn in (lib.risvec_step_fused_multi, lib.risvec_step_multi):
        assert fn(C.byref(s), C.byref(p), 3, FAKE, FAKE, FAKE, None, 7, 0, flags, None, None) == N.ERR_ARG
        assert "unknown flag" in _err()
    # the sweep + step entry point and the 3GPP entry point
    assert lib.risvec_step_fused_bcd(*step_args(s)) == N.ERR_ARG and "unknown flag" in _err()
    assert lib.risvec_step_fused_3gpp(C.byref(s), C.byref(p), N.CH_3GPP_UMI, FAKE, FAKE, FAKE, None, None, 7, 0, 1, flags, None,
                                      None) == N.ERR_ARG
    # the ring entry point: its cached form refuses the bit, its fused form wants theta_idx and control_bit = 3 as well
    ring = N.RisVecStepRing()
    rflags = N.STEP_POLICY_ACTION | N.STEP_OBS | CUR

    def ring_call(s, fused):
        return lib.risvec_step_ring(C.byref(s), C.byref(p), C.byref(ring), FAKE, FAKE, FAKE, None, 7, 0, rflags, fused, None)

    assert ring_call(_state(), 0) == N.ERR_ARG and "THETA_IDX_CURRENT" in _err()
    s = _state()
    s.theta_idx = None
    assert ring_call(s, 1) == N.ERR_ARG and "theta_idx" in _err()
    assert ring_call(_state(control_bit=2), 1) == N.ERR_ARG and "control_bit" in _err()
