"""CPU-side tests of the device weight packing of the DDPG actor (`risvec_sarl_actor_pack`, `pack_actor_weights_device`,
`BatchedActor(pack=...)`, `share_state_dict`): the exported symbols, the workspace rule, the argument checks of the C
entry point (which must answer before touching a device) and the Python surface."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from ris_vec_marl_amd import _native as N
from ris_vec_marl_amd import actor as ACT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (80, 512, 256, 56)
# the truth table of test_sarl_actor_host.py
TABLE = [((80, 512, 256, 56), 1), ((104, 512, 256, 80), 1), ((36, 64, 128, 24), 1), ((128, 1024, 256, 96), 1),
         ((144, 512, 256, 56), 0), ((80, 500, 256, 56), 0), ((80, 512, 64, 56), 0), ((80, 512, 256, 288), 0),
         ((0, 512, 256, 56), 0), ((80, 1056, 256, 56), 0), ((80, 512, 256, 97), 0), ((129, 512, 256, 56), 0)]


def test_symbols_are_exported_and_declared_and_the_abi_stays_17():
    lib = N.load()
    header = open(os.path.join(ROOT, "include", "risvec.h")).read()
    for name in ("risvec_sarl_actor_pack_workspace", "risvec_sarl_actor_pack"):
        assert name in N.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert lib.risvec_abi_version() == 17 == N.ABI_VERSION
    assert "#define RISVEC_ABI_VERSION 17" in header


@pytest.mark.parametrize("dims,ok", TABLE)
def test_workspace_is_nonzero_exactly_where_the_actor_kernel_is_built(dims, ok):
    lib = N.load()
    need = lib.risvec_sarl_actor_pack_workspace(*dims)
    assert (need != 0) == bool(ok) == bool(lib.risvec_sarl_actor_supported(*dims))
    assert need % 16 == 0 and need < 4096                       # "small": the row means and three factors


def test_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf = (C.c_float * 64)()                                  # host memory: never dereferenced, only checked
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    g = ACT.actor_geom(*DIMS)
    nbytes = g.items * g.rows * 1024
    need = lib.risvec_sarl_actor_pack_workspace(*DIMS)
    ptrs = ("W1", "b1", "lw", "lb", "W2", "Wmu", "ws", "sc", "wk")

    def call(dims=DIMS, wb=nbytes, kb=need, **kw):
        a = {n: kw.get(n, p) for n in ptrs}
        return lib.risvec_sarl_actor_pack(*dims, a["W1"], a["b1"], a["lw"], a["lb"], a["W2"], a["Wmu"], a["ws"], wb, a["sc"],
                                          a["wk"], kb, None)
    for dims, ok in TABLE:
        if not ok:
            assert call(dims=dims) == N.ERR_UNSUPPORTED, dims
            assert b"risvec_sarl_actor_pack" in lib.risvec_last_error()
    for name in ptrs:
        assert call(**{name: None}) == N.ERR_ARG, name
        assert b"NULL" in lib.risvec_last_error()
    assert call(wb=nbytes - 1024) == N.ERR_ARG and b"wstream_bytes" in lib.risvec_last_error()
    assert call(wb=nbytes + 1024) == N.ERR_ARG
    assert call(kb=need - 1) == N.ERR_ARG and b"workspace_bytes" in lib.risvec_last_error()
    assert call(kb=0) == N.ERR_ARG
    assert call(ws=p + 4) == N.ERR_ARG and b"wstream is not 16-byte aligned" in lib.risvec_last_error()
    assert call(wk=p + 8) == N.ERR_ARG and call(W2=p + 4) == N.ERR_ARG


def test_python_surface():
    import ris_vec_marl_amd as rv
    sig = inspect.signature(ACT.BatchedActor.__init__)
    assert "pack" in sig.parameters and sig.parameters["pack"].default is None
    assert ACT.BatchedActor.PACK_MODES == ("host", "device")
    assert callable(ACT.pack_actor_weights_device) and callable(ACT.BatchedActor.share_state_dict)
    assert rv.pack_actor_weights_device is ACT.pack_actor_weights_device and "pack_actor_weights_device" in rv.__all__
    assert list(inspect.signature(ACT.pack_actor_weights_device).parameters)[:7] == ["W1", "b1", "ln1_w", "ln1_b", "W2", "Wmu", "out"]
    if not torch.cuda.is_available():                         # the kernels have no CPU form
        z = torch.zeros
        with pytest.raises(RuntimeError):
            ACT.pack_actor_weights_device(z(64, 21), z(64), z(64), z(64), z(128, 64), z(6, 128))
