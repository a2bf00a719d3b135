"""RISVEC_STEP_STEER_HEADS_CURRENT on the host (no GPU): the bit rides on RISVEC_STEP_H_R_STEER_CURRENT and nowhere else --
the two entry points that take that bit accept this one with it and refuse it alone, every other entry point refuses it as
it refuses the GEN bit, it is dropped where the GEN bit is dropped, it never changes what the selector answers, and
risvec_steer_heads checks its arguments."""
import ctypes as C
import os
import re

import pytest

from ris_vec_marl_amd import _native as N
from tests.test_h_r_rebuild_host import FLAGS, FORMS, SHAPES, _ring_call, _step_args
from tests.test_host_cpu import DISPATCH_TABLE
from tests.test_theta_index_host import FAKE, _err, _params, _state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = N.STEP_H_R_STEER_CURRENT
HD = N.STEP_STEER_HEADS_CURRENT


def test_the_bit_the_exports_and_the_abi():
    header = open(os.path.join(ROOT, "include", "risvec.h")).read()
    assert re.search(r"RISVEC_STEP_STEER_HEADS_CURRENT = (\d+)", header).group(1) == str(HD) == "8192"
    assert N.load().risvec_abi_version() == 17 == N.ABI_VERSION
    assert C.sizeof(N.RisVecState) == 248                      # the heads travel without a state field
    lib = N.load()
    for name in ("risvec_last_h_r_heads", "risvec_steer_heads"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in N.EXPORTS and hasattr(lib, name)
    assert N.last_h_r_heads() in (0, 1)


def test_the_two_entry_points_accept_the_bit_with_the_gen_bit():
    """As in test_h_r_rebuild_host: nothing may launch, so each call fails on a check that runs AFTER the flag checks."""
    lib, p = N.load(), _params()
    s = _state()
    s.h_r = None
    for extra in (0, N.STEP_THETA_IDX_CURRENT):
        assert lib.risvec_step_fused(*_step_args(s, p, N.STEP_METRICS | GEN | HD | extra)) == N.ERR_ARG
        assert "state.h_r is NULL" in _err()
    rflags = N.STEP_POLICY_ACTION | N.STEP_OBS
    assert _ring_call(_state(), p, rflags | GEN | HD, 1) == N.ERR_SHAPE and "the ring must have" in _err()


def test_the_bit_is_refused_without_the_gen_bit():
    lib, p = N.load(), _params()
    assert lib.risvec_step_fused(*_step_args(_state(), p, N.STEP_METRICS | HD)) == N.ERR_ARG
    assert "RISVEC_STEP_STEER_HEADS_CURRENT" in _err() and "RISVEC_STEP_H_R_STEER_CURRENT" in _err()
    assert _ring_call(_state(), p, N.STEP_POLICY_ACTION | N.STEP_OBS | HD, 1) == N.ERR_ARG
    assert "RISVEC_STEP_STEER_HEADS_CURRENT" in _err() and "RISVEC_STEP_H_R_STEER_CURRENT" in _err()


def test_the_bit_is_dropped_without_steer_ang_or_z_r():
    """steer_ang / z_r NULL: no complaint -- the calls get as far as they do with the pointers given."""
    lib, p = N.load(), _params()
    for missing in ("steer_ang", "z_r"):
        s = _state()
        setattr(s, missing, None)
        s.h_r = None
        assert lib.risvec_step_fused(*_step_args(s, p, N.STEP_METRICS | GEN | HD)) == N.ERR_ARG and "state.h_r is NULL" in _err()
        s = _state()
        setattr(s, missing, None)
        assert _ring_call(s, p, N.STEP_POLICY_ACTION | N.STEP_OBS | GEN | HD, 1) == N.ERR_SHAPE and "the ring must have" in _err()


@pytest.mark.parametrize("with_gen", [False, True])
def test_the_bit_is_unknown_everywhere_else(with_gen):
    lib, p = N.load(), _params()
    flags = N.STEP_METRICS | HD | (GEN if with_gen else 0)
    s = _state()
    assert lib.risvec_step(*_step_args(s, p, flags)) == N.ERR_ARG and "unknown flag" in _err()
    for fn in (lib.risvec_step_fused_multi, lib.risvec_step_multi):
        assert fn(C.byref(s), C.byref(p), 3, FAKE, FAKE, FAKE, None, 7, 0, flags, None, None) == N.ERR_ARG
        assert "unknown flag" in _err()
    assert lib.risvec_step_fused_bcd(*_step_args(s, p, flags)) == N.ERR_ARG and "unknown flag" in _err()
    assert lib.risvec_step_fused_3gpp(C.byref(s), C.byref(p), N.CH_3GPP_UMI, FAKE, FAKE, FAKE, None, None, 7, 0, 1, flags, None,
                                      None) == N.ERR_ARG
    # the ring entry point's cached form: a hint to the fused forms, like the GEN bit there
    rflags = N.STEP_POLICY_ACTION | N.STEP_OBS | HD | (GEN if with_gen else 0)
    assert _ring_call(s, p, rflags, 0) == N.ERR_ARG and "STEER_HEADS_CURRENT" in _err()


@pytest.mark.parametrize("shape", SHAPES)
def test_the_bit_never_changes_the_plan(shape):
    """risvec_step_kernel(state, flags | GEN | HEADS, form) == the answer without the two bits at every batch size of the
    dispatch table, for every form, with and without the flags that do select, under the rules and with forms forced."""
    s = _state(*shape, fake=False)
    for force in (None, dict(lat=False), dict(lat=True), dict(lat=False, pipe_nt=True), dict(lat=False, pipe_waves=2)):
        for form in FORMS:
            for flags in FLAGS:
                if force is None:
                    a, b = N.step_kernel(s, flags, form), N.step_kernel(s, flags | GEN | HD, form)
                else:
                    with N.forced(**force):
                        a, b = N.step_kernel(s, flags, form), N.step_kernel(s, flags | GEN | HD, form)
                assert a == b, (shape, force, form, flags, a, b)


@pytest.mark.parametrize("shape,name", DISPATCH_TABLE)
def test_every_row_keeps_its_name(shape, name):
    assert N.step_kernel(_state(*shape, fake=False), GEN | HD, N.FORM_FUSED) == name


def test_steer_heads_checks_its_arguments():
    lib = N.load()
    s = _state()
    assert lib.risvec_steer_heads(C.byref(s), None, None) == N.ERR_ARG and "heads is NULL" in _err()
    assert lib.risvec_steer_heads(C.byref(s), FAKE + 8, None) == N.ERR_ARG and "heads is not 16-byte aligned" in _err()
    s.steer_ang = None
    assert lib.risvec_steer_heads(C.byref(s), FAKE, None) == N.ERR_ARG and "state.steer_ang is NULL" in _err()
    assert lib.risvec_steer_heads(C.byref(_state(M=36)), FAKE, None) == N.ERR_UNSUPPORTED and "multiple of 16" in _err()
