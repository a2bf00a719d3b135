"""RISVEC_STEP_THETA_IDX_CURRENT and the forced forms, on the host (no GPU): now that the NT pipeline and the latency
family's NT / ALT members honour the bit, it still selects nothing -- the selector's answer is the same with and without
it under every forced combination the GPU tests use -- and it is still refused without state.theta_idx before any launch."""
import ctypes as C

import pytest

from ris_vec_marl_amd import _native as N
from tests.test_host_cpu import DISPATCH_TABLE
from tests.test_theta_index_host import CUR, FAKE, FLAGS, _err, _params, _state

FORCES = (None, dict(lat=False, pipe_nt=True), dict(lat=True, lat_nt=True), dict(lat=True, lat_alt=True), dict(lat=True),
          dict(lat=True, lat_epw=4), dict(pipe_nt=True))


def _answers(s, flags, form, force):
    if force is None:
        return N.step_kernel(s, flags, form), N.step_kernel(s, flags | CUR, form)
    with N.forced(**force):
        return N.step_kernel(s, flags, form), N.step_kernel(s, flags | CUR, form)


@pytest.mark.parametrize("shape", sorted({shape for shape, _ in DISPATCH_TABLE}))
def test_the_bit_changes_no_plan_under_the_forced_forms(shape):
    s = _state(*shape, fake=False)
    for force in FORCES:
        for form in (N.FORM_FUSED, N.FORM_FUSED_RING):
            for flags in FLAGS:
                a, b = _answers(s, flags, form, force)
                assert a == b, (shape, force, form, flags, a, b)


def test_the_forced_forms_are_the_ones_the_gpu_tests_name():
    s = _state(515, 8, 64, fake=False)
    for force, name in ((dict(lat=False, pipe_nt=True), "k_step_fused_pipe<8,64,2,MarlCore,NT>"),
                        (dict(lat=True, lat_nt=True), "k_step_fused_lat<8,64,4,NT>"),
                        (dict(lat=True, lat_alt=True), "k_step_fused_lat<8,64,4,ALT>"),
                        (dict(lat=True, lat_epw=4), "k_step_fused_lat<8,64,4>")):
        assert _answers(s, 0, N.FORM_FUSED, force) == (name, name), force
    with N.forced(pipe_nt=True):
        assert N.step_kernel(s, CUR, N.FORM_FUSED_RING) == "k_step_fused_pipe<8,64,2,MarlCore+ring,NT>"


@pytest.mark.parametrize("force", [dict(lat=True, lat_nt=True), dict(lat=True, lat_alt=True), dict(lat=False, pipe_nt=True)],
                         ids=["lat_nt", "lat_alt", "pipe_nt"])
def test_the_bit_without_indices_is_refused_under_a_forced_form(force):
    """theta_idx = NULL: risvec_step_fused refuses the call in its argument checks (every other pointer is a fake address
    the host never dereferences, so a launch would not return RISVEC_ERR_ARG)."""
    lib = N.load()
    p = _params()
    s = _state()
    s.theta_idx = None
    with N.forced(**force):
        rc = lib.risvec_step_fused(C.byref(s), C.byref(p), FAKE, FAKE, FAKE, None, 7, 0, N.STEP_METRICS | CUR, None)
        assert rc == N.ERR_ARG and "theta_idx" in _err()
