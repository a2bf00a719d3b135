"""RISVEC_STEP_H_R_STEER_CURRENT on the host (no GPU): the two entry points that take the bit accept it, it never changes
what the selector answers, it is ignored without steer_ang, refused together with RISVEC_STEP_STEER and by every other
entry point, and the ABI version stays while RisVecState grows by one pointer."""
import ctypes as C
import os
import re

import pytest

from ris_vec_marl_amd import _native as N
from tests.test_host_cpu import DISPATCH_TABLE
from tests.test_theta_index_host import FAKE, _err, _params, _state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = N.STEP_H_R_STEER_CURRENT


def test_abi_version_the_bit_and_the_struct():
    header = open(os.path.join(ROOT, "include", "risvec.h")).read()
    assert N.load().risvec_abi_version() == 17 == N.ABI_VERSION
    assert int(re.search(r"#define RISVEC_ABI_VERSION (\d+)", header).group(1)) == 17
    assert re.search(r"RISVEC_STEP_H_R_STEER_CURRENT = (\d+)", header).group(1) == str(GEN) == "2048"
    # 6 int32 + 1 int64 + 27 pointers: steer_ang is the last field, behind theta_idx
    assert N.RisVecState._fields_[-1][0] == "steer_ang" and N.RisVecState._fields_[-2][0] == "theta_idx"
    assert C.sizeof(N.RisVecState) == 4 * 6 + 8 + 8 * 27 == 248
    # the library checks struct_bytes against ITS sizeof: the new size passes, the old one (one pointer less) is refused
    s = _state(fake=False)
    assert N.step_kernel(s, 0, N.FORM_CACHED) is not None
    s.struct_bytes = 240
    assert N.step_kernel(s, 0, N.FORM_CACHED) is None and "ABI mismatch" in _err()


def test_the_header_declares_what_the_library_exports():
    header = open(os.path.join(ROOT, "include", "risvec.h")).read()
    lib = N.load()
    for name in ("risvec_last_h_r_rebuilt", "risvec_h_r_from_steer"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in N.EXPORTS and hasattr(lib, name)
    assert N.last_h_r_rebuilt() in (0, 1)


SHAPES = sorted({shape for shape, _ in DISPATCH_TABLE})
FLAGS = (0, N.STEP_METRICS | N.STEP_OBS, N.STEP_STEER, N.STEP_THETA_BY_INDEX, N.STEP_THETA_IDX_CURRENT, N.STEP_3GPP)
FORMS = (N.FORM_CACHED, N.FORM_FUSED, N.FORM_CACHED_RING, N.FORM_FUSED_RING, N.FORM_FUSED_MULTI)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_bit_never_changes_the_plan(shape):
    """risvec_step_kernel(state, flags | GEN, form) == the answer without the bit at every batch size of the dispatch table,
    for every form, with and without the flags that do select, under the rules and with the forms forced."""
    s = _state(*shape, fake=False)
    for force in (None, dict(lat=False), dict(lat=True), dict(lat=False, pipe_nt=True), dict(lat=False, pipe_waves=2)):
        for form in FORMS:
            for flags in FLAGS:
                if force is None:
                    a, b = N.step_kernel(s, flags, form), N.step_kernel(s, flags | GEN, form)
                else:
                    with N.forced(**force):
                        a, b = N.step_kernel(s, flags, form), N.step_kernel(s, flags | GEN, form)
                assert a == b, (shape, force, form, flags, a, b)


@pytest.mark.parametrize("shape,name", DISPATCH_TABLE)
def test_every_row_keeps_its_name(shape, name):
    assert N.step_kernel(_state(*shape, fake=False), GEN, N.FORM_FUSED) == name


def _step_args(s, p, fl):
    return (C.byref(s), C.byref(p), FAKE, FAKE, FAKE, None, 7, 0, fl, None)


def _ring_call(s, p, fl, fused):
    ring = N.RisVecStepRing()
    return N.load().risvec_step_ring(C.byref(s), C.byref(p), C.byref(ring), FAKE, FAKE, FAKE, None, 7, 0, fl, fused, None)


def test_the_two_entry_points_accept_the_bit():
    """Nothing may launch here (the pointers are fake), so each call is made to fail on a check that runs AFTER the flag
    checks: a NULL state.gain for the fused step, the ring's shape for the ring form.  The same calls with an unknown bit
    in place of this one fail on the bit."""
    lib, p = N.load(), _params()
    s = _state()
    s.h_r = None
    assert lib.risvec_step_fused(*_step_args(s, p, N.STEP_METRICS | GEN)) == N.ERR_ARG and "state.h_r is NULL" in _err()
    assert lib.risvec_step_fused(*_step_args(s, p, N.STEP_METRICS | GEN | N.STEP_THETA_IDX_CURRENT)) == N.ERR_ARG
    assert "state.h_r is NULL" in _err()
    assert lib.risvec_step_fused(*_step_args(s, p, N.STEP_METRICS | 4096)) == N.ERR_ARG and "unknown flag" in _err()
    rflags = N.STEP_POLICY_ACTION | N.STEP_OBS
    assert _ring_call(_state(), p, rflags | GEN, 1) == N.ERR_SHAPE and "the ring must have" in _err()
    assert _ring_call(_state(), p, rflags | 4096, 1) == N.ERR_ARG and "unknown flag" in _err()


def test_the_bit_is_ignored_without_steer_ang_or_z_r():
    """steer_ang / z_r NULL: no complaint about them -- the calls get as far as they do with the pointers given."""
    lib, p = N.load(), _params()
    for missing in ("steer_ang", "z_r"):
        s = _state()
        setattr(s, missing, None)
        s.h_r = None
        assert lib.risvec_step_fused(*_step_args(s, p, N.STEP_METRICS | GEN)) == N.ERR_ARG and "state.h_r is NULL" in _err()
        s = _state()
        setattr(s, missing, None)
        assert _ring_call(s, p, N.STEP_POLICY_ACTION | N.STEP_OBS | GEN, 1) == N.ERR_SHAPE and "the ring must have" in _err()


def test_the_bit_is_refused_where_it_does_not_apply():
    lib, p = N.load(), _params()
    flags = N.STEP_METRICS | GEN
    # together with the Horner form
    assert lib.risvec_step_fused(*_step_args(_state(), p, flags | N.STEP_STEER)) == N.ERR_ARG and "exclude each other" in _err()
    # the cached entry point, the T-step entry points, sweep + step, 3GPP
    s = _state()
    assert lib.risvec_step(*_step_args(s, p, flags)) == N.ERR_ARG and "unknown flag" in _err()
    for fn in (lib.risvec_step_fused_multi, lib.risvec_step_multi):
        assert fn(C.byref(s), C.byref(p), 3, FAKE, FAKE, FAKE, None, 7, 0, flags, None, None) == N.ERR_ARG
        assert "unknown flag" in _err()
    assert lib.risvec_step_fused_bcd(*_step_args(s, p, flags)) == N.ERR_ARG and "unknown flag" in _err()
    assert lib.risvec_step_fused_3gpp(C.byref(s), C.byref(p), N.CH_3GPP_UMI, FAKE, FAKE, FAKE, None, None, 7, 0, 1, flags, None,
                                      None) == N.ERR_ARG
    # the ring entry point's cached form
    assert _ring_call(s, p, N.STEP_POLICY_ACTION | N.STEP_OBS | GEN, 0) == N.ERR_ARG and "H_R_STEER_CURRENT" in _err()


def test_h_r_from_steer_checks_its_arguments():
    lib = N.load()
    s = _state()
    assert lib.risvec_h_r_from_steer(C.byref(s), None, None) == N.ERR_ARG and "out is NULL" in _err()
    s.steer_ang = None
    assert lib.risvec_h_r_from_steer(C.byref(s), FAKE, None) == N.ERR_ARG and "steer_ang" in _err()
    assert lib.risvec_h_r_from_steer(C.byref(_state(M=36)), FAKE, None) == N.ERR_UNSUPPORTED and "multiple of 16" in _err()
