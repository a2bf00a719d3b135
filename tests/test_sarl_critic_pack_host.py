"""CPU-side tests of the device-side target-network update of the DDPG learner: the device weight packing of the critic
(`risvec_sarl_critic_pack`, `pack_critic_weights_device`, `BatchedCritic(pack=...)`) and the Polyak blend
(`risvec_soft_update`, `soft_update_from`, `ddpg_soft_update`) -- the exported symbols, the workspace rule, the argument
checks of the C entry points (which must answer before touching a device) and the Python surface."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from ris_vec_marl_amd import _native as N
from ris_vec_marl_amd import actor as ACT
from ris_vec_marl_amd import critic as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (80, 1024, 512, 256, 56)
# the shapes of test_sarl_critic_host.py: SHAPES (built) and the refused ones of its argument test
TABLE = [((80, 1024, 512, 256, 56), 1), ((104, 1024, 512, 256, 80), 1), ((80, 96, 128, 128, 56), 1), ((36, 64, 128, 128, 24), 1),
         ((128, 1024, 512, 256, 96), 1), ((5, 32, 128, 128, 1), 1), ((79, 160, 256, 128, 33), 1),
         ((144, 1024, 512, 256, 56), 0), ((80, 1000, 512, 256, 56), 0), ((80, 1024, 384, 256, 56), 0),
         ((80, 1024, 512, 512, 56), 0), ((80, 1024, 512, 256, 97), 0), ((0, 1024, 512, 256, 56), 0), ((80, 1056, 512, 256, 56), 0)]


def aligned_host_pointer():
    buf = (C.c_float * 64)()                                  # host memory: never dereferenced, only checked
    return buf, C.addressof(buf) + (-C.addressof(buf)) % 16


def test_symbols_are_exported_and_declared_and_the_abi_stays_17():
    lib = N.load()
    header = open(os.path.join(ROOT, "include", "risvec.h")).read()
    for name in ("risvec_sarl_critic_pack_workspace", "risvec_sarl_critic_pack", "risvec_soft_update"):
        assert name in N.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert lib.risvec_abi_version() == 17 == N.ABI_VERSION
    assert "#define RISVEC_ABI_VERSION 17" in header


@pytest.mark.parametrize("dims,ok", TABLE)
def test_workspace_is_nonzero_exactly_where_the_critic_kernel_is_built(dims, ok):
    lib = N.load()
    need = lib.risvec_sarl_critic_pack_workspace(*dims)
    assert (need != 0) == bool(ok) == bool(lib.risvec_sarl_critic_supported(*dims))
    assert need % 16 == 0 and need < 4096                       # "small": the row means and the slots of the maxima


def test_pack_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf, p = aligned_host_pointer()
    nbytes = lib.risvec_sarl_critic_stream_bytes(*DIMS)
    assert nbytes == CR.critic_geom(*DIMS).rows * 1024
    need = lib.risvec_sarl_critic_pack_workspace(*DIMS)
    ptrs = ("W1", "b1", "W2", "Wav", "W3", "ws", "sc", "wk")

    def call(dims=DIMS, wb=nbytes, kb=need, **kw):
        a = {n: kw.get(n, p) for n in ptrs}
        return lib.risvec_sarl_critic_pack(*dims, a["W1"], a["b1"], a["W2"], a["Wav"], a["W3"], a["ws"], wb, a["sc"], a["wk"], kb, None)
    for dims, ok in TABLE:
        if not ok:
            assert call(dims=dims) == N.ERR_UNSUPPORTED, dims
            assert b"risvec_sarl_critic_pack" in lib.risvec_last_error()
    for name in ptrs:
        assert call(**{name: None}) == N.ERR_ARG, name
        assert b"NULL" in lib.risvec_last_error()
    assert call(wb=nbytes - 1024) == N.ERR_ARG and b"wstream_bytes" in lib.risvec_last_error()
    assert call(wb=nbytes + 1024) == N.ERR_ARG
    assert call(kb=need - 1) == N.ERR_ARG and b"workspace_bytes" in lib.risvec_last_error()
    assert call(kb=0) == N.ERR_ARG
    assert call(ws=p + 4) == N.ERR_ARG and b"wstream is not 16-byte aligned" in lib.risvec_last_error()
    assert call(wk=p + 8) == N.ERR_ARG and b"workspace is not 16-byte aligned" in lib.risvec_last_error()
    for name in ("W1", "b1", "W2", "Wav", "W3"):                # float alignment is all the weights need
        assert call(**{name: p + 2}) == N.ERR_ARG and b"4-byte aligned" in lib.risvec_last_error(), name
        assert call(**{name: p + 1}) == N.ERR_ARG


def test_soft_update_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf, p = aligned_host_pointer()

    def call(n=2, on=(p, p + 64), tg=(p + 128, p + 192), ne=(3, 7), tau=0.005, omt=0.995, arrays=(True, True, True)):
        k = max(len(on), 1)
        a = (C.c_void_p * k)(*on) if arrays[0] else None
        b = (C.c_void_p * k)(*tg) if arrays[1] else None
        c = (C.c_int64 * k)(*ne) if arrays[2] else None
        return lib.risvec_soft_update(n, a, b, c, tau, omt, None)
    many = tuple(p for _ in range(33))
    assert call(n=0) == N.ERR_SHAPE and b"risvec_soft_update" in lib.risvec_last_error()
    assert call(n=-1) == N.ERR_SHAPE
    assert call(n=33, on=many, tg=tuple(p + 128 for _ in range(33)), ne=(1,) * 33) == N.ERR_SHAPE
    assert call(ne=(3, 0)) == N.ERR_SHAPE and call(ne=(-5, 7)) == N.ERR_SHAPE
    for i in range(3):
        assert call(arrays=tuple(j != i for j in range(3))) == N.ERR_ARG
        assert b"NULL" in lib.risvec_last_error()
    assert call(on=(p, None)) == N.ERR_ARG and call(tg=(None, p + 192)) == N.ERR_ARG
    assert call(on=(p + 2, p + 64)) == N.ERR_ARG and b"4-byte aligned" in lib.risvec_last_error()
    assert call(tg=(p + 128, p + 193)) == N.ERR_ARG
    assert call(tg=(p + 128, p + 64)) == N.ERR_ARG and b"same tensor" in lib.risvec_last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(tau=bad) == N.ERR_ARG and call(omt=bad) == N.ERR_ARG


def test_python_surface():
    import ris_vec_marl_amd as rv
    sig = inspect.signature(CR.BatchedCritic.__init__)
    assert "pack" in sig.parameters and sig.parameters["pack"].default is None
    assert CR.BatchedCritic.PACK_MODES == ("host", "device")
    for name in ("pack_critic_weights_device", "ddpg_soft_update"):
        assert getattr(rv, name) is getattr(CR, name) and name in rv.__all__
    assert list(inspect.signature(CR.pack_critic_weights_device).parameters) == ["W1", "b1", "W2", "Wav", "W3", "out", "workspace"]
    assert list(inspect.signature(CR.ddpg_soft_update).parameters) == ["actor", "target_actor", "critic", "target_critic", "tau"]
    for cls in (ACT.BatchedActor, CR.BatchedCritic):
        assert list(inspect.signature(cls.soft_update_from).parameters) == ["self", "online", "tau"]
        assert "version counters" in cls.soft_update_from.__doc__
    assert "version counters" in CR.ddpg_soft_update.__doc__
    if not torch.cuda.is_available():                         # the kernels have no CPU form
        z = torch.zeros
        with pytest.raises(RuntimeError):
            CR.pack_critic_weights_device(z(64, 21), z(64), z(128, 64), z(128, 6), z(128, 128))


ACTOR_DIMS = dict(W1=(96, 80), b1=(96,), ln1_w=(96,), ln1_b=(96,), W2=(128, 96), b2=(128,), ln2_w=(128,), ln2_b=(128,),
                  Wmu=(56, 128), bmu=(56,))
CRITIC_DIMS = dict(W1=(96, 80), b1=(96,), ln1_w=(96,), ln1_b=(96,), W2=(128, 96), b2=(128,), ln2_w=(128,), ln2_b=(128,),
                   W3=(128, 128), b3=(128,), ln3_w=(128,), ln3_b=(128,), Wav=(128, 56), bav=(128,), Wq=(1, 128), bq=(1,))


def bare(cls, dims, device):
    """A target network built without a device, as test_load_state_dict_rejects_a_wrong_shape does: the checks come before
    any use (test_weight_set_host.py has the refusals of `soft_update_from`, for every class)."""
    t = cls.__new__(cls)
    t.device = torch.device(device)
    for k, s in dims.items():
        setattr(t, k, torch.full(s, 3.0))
    t._packed = ("key", "stream")
    t.packs = 0
    return t


def test_ddpg_soft_update_refuses_and_changes_nothing():
    ta, tc = bare(ACT.BatchedActor, ACTOR_DIMS, "cpu"), bare(CR.BatchedCritic, CRITIC_DIMS, "cpu")
    sa = {k: torch.ones(ACTOR_DIMS[a]) for k, a in ACT.BatchedActor._SD.items()}
    sc = {k: torch.ones(CRITIC_DIMS[a]) for k, a in CR.BatchedCritic._SD.items()}
    with pytest.raises(ValueError):
        CR.ddpg_soft_update(sa, ta, {**sc, "q.weight": torch.ones(128, 1).T.double()}, tc, 0.005)
    with pytest.raises(KeyError):
        CR.ddpg_soft_update({k: v for k, v in sa.items() if k != "mu.bias"}, ta, sc, tc, 0.005)
    with pytest.raises(ValueError):
        CR.ddpg_soft_update(sa, ta, sc, tc, 2.0)
    with pytest.raises(RuntimeError):                         # no CPU form
        CR.ddpg_soft_update(sa, ta, sc, tc, 0.005)
    for t, dims in ((ta, ACTOR_DIMS), (tc, CRITIC_DIMS)):
        assert all(bool((getattr(t, a) == 3.0).all()) for a in dims) and t._packed == ("key", "stream")
