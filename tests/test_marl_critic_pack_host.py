"""CPU-side tests of the device pack of the SAC twin critic's weight streams (`risvec_marl_critic_pack`,
`pack_marl_critic_weights_device`, `BatchedTwinCritic.pack`): the exported symbols, the workspace rule against the shape
rule, the argument checks of the C entry point (which must answer before touching a device; every pointer here is host
memory that is never dereferenced), and the Python surface."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from ris_vec_marl_amd import _native as N
from ris_vec_marl_amd import marl_critic as MC

# the built and the refused shapes of test_marl_critic_host.py
BUILT = [(20, 24, 1024, 512, 256), (40, 80, 1024, 512, 256), (40, 80, 64, 128, 128), (20, 24, 64, 128, 128),
         (127, 1, 1024, 512, 256), (1, 127, 32, 128, 128), (1, 1, 32, 128, 256), (33, 46, 160, 256, 128)]
REFUSED = [(80, 288, 1024, 512, 256), (49, 80, 1024, 512, 256), (40, 80, 1000, 512, 256), (40, 80, 1024, 384, 256),
           (40, 80, 1024, 512, 512), (0, 80, 1024, 512, 256)]
DIMS = (40, 80, 1024, 512, 256)
NAMES = ("risvec_marl_critic_pack_workspace", "risvec_marl_critic_pack")


def test_library_declares_and_exports_the_pack():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "risvec.h")).read()
    lib = N.load()
    for name in NAMES:
        assert name in N.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, header)
    assert "RisVecMarlCriticPackNet" in header and hasattr(N, "RisVecMarlCriticPackNet")
    m = re.search(r"#define RISVEC_ABI_VERSION (\d+)", header)
    assert int(m.group(1)) == N.ABI_VERSION == lib.risvec_abi_version() == 17      # additions only: the ABI version stays
    # the POD struct as the header lays it out: 6 fields of 8 bytes
    assert C.sizeof(N.RisVecMarlCriticPackNet) == 48
    assert [f for f, _ in N.RisVecMarlCriticPackNet._fields_] == ["W1", "W2", "W3", "wstream", "wstream_bytes", "scales"]


def test_workspace_is_nonzero_exactly_where_the_kernel_is_built():
    lib = N.load()
    for dims in BUILT + REFUSED:
        ok = bool(lib.risvec_marl_critic_supported(*dims))
        assert ok == (dims in BUILT), dims
        for n_nets in (1, 2):
            need = lib.risvec_marl_critic_pack_workspace(*dims, n_nets)
            assert (need != 0) == ok, (dims, n_nets)
            assert need % 16 == 0 and need < 4096, (dims, n_nets, need)
    for n_nets in (0, 3, -1):
        assert lib.risvec_marl_critic_pack_workspace(*DIMS, n_nets) == 0
    assert lib.risvec_marl_critic_pack_workspace(*DIMS, 2) >= lib.risvec_marl_critic_pack_workspace(*DIMS, 1)


def test_pack_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf = (C.c_float * 256)()                                 # host memory: never dereferenced, only checked
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    nbytes = lib.risvec_marl_critic_stream_bytes(*DIMS)
    assert nbytes == MC.marl_critic_geom(*DIMS).rows * 1024
    fields = ("W1", "W2", "W3", "wstream", "scales")

    def call(dims=DIMS, n_nets=2, nets="make", wb=nbytes, bad_net=1, wk=p, kb=None, **kw):
        if nets == "make":
            arr = (N.RisVecMarlCriticPackNet * 2)()
            for c in range(2):                                # distinct streams and scales per net
                arr[c] = N.RisVecMarlCriticPackNet(p, p, p, p + 64 + 128 * c, nbytes, p + 32 + 128 * c)
            arr[bad_net].wstream_bytes = wb
            for k, v in kw.items():
                setattr(arr[bad_net], k, v)
            nets = C.cast(arr, C.c_void_p)
        if kb is None:
            kb = lib.risvec_marl_critic_pack_workspace(*DIMS, 2)
        return lib.risvec_marl_critic_pack(*dims, n_nets, nets, wk, kb, None)
    # every call below carries exactly one fault: a complete set of host pointers is never passed
    for dims in REFUSED:
        assert call(dims=dims) == N.ERR_UNSUPPORTED, dims
        assert b"risvec_marl_critic_pack" in lib.risvec_last_error()
    for k in (0, 3, -1):
        assert call(n_nets=k) == N.ERR_ARG and b"n_nets" in lib.risvec_last_error()
    assert call(nets=None) == N.ERR_ARG and b"nets is NULL" in lib.risvec_last_error()
    for net in (0, 1):
        for f in fields:
            assert call(bad_net=net, **{f: None}) == N.ERR_ARG, f
            msg = lib.risvec_last_error()
            assert b"NULL" in msg and ("nets[%d].%s" % (net, f)).encode() in msg, msg
        assert call(wb=nbytes - 1024, bad_net=net) == N.ERR_ARG           # a stream of another shape
        assert b"wstream_bytes" in lib.risvec_last_error()
        assert call(wb=nbytes + 1024, bad_net=net) == N.ERR_ARG
        assert call(bad_net=net, wstream=p + 64 + 128 * net + 4) == N.ERR_ARG
        assert b"wstream is not 16-byte aligned" in lib.risvec_last_error()
        for f in ("W1", "W2", "W3", "scales"):                # float alignment is all the weights and the scales need
            assert call(bad_net=net, **{f: p + 2}) == N.ERR_ARG, f
            msg = lib.risvec_last_error()
            assert b"4-byte aligned" in msg and f.encode() in msg, msg
            assert call(bad_net=net, **{f: p + 1}) == N.ERR_ARG, f
    need = lib.risvec_marl_critic_pack_workspace(*DIMS, 2)
    assert call(wk=None) == N.ERR_ARG and b"workspace is NULL" in lib.risvec_last_error()
    assert call(wk=p + 8) == N.ERR_ARG and b"workspace is not 16-byte aligned" in lib.risvec_last_error()
    assert call(kb=need - 1) == N.ERR_ARG and b"workspace_bytes" in lib.risvec_last_error()
    assert call(kb=0) == N.ERR_ARG
    # one net needs less: what is enough for one net is refused for two
    need1 = lib.risvec_marl_critic_pack_workspace(*DIMS, 1)
    if need1 < need:
        assert call(kb=need1) == N.ERR_ARG and b"workspace_bytes" in lib.risvec_last_error()
    # two nets that would write the same buffer
    assert call(wstream=p + 64) == N.ERR_ARG and b"wstream" in lib.risvec_last_error() and b"same" in lib.risvec_last_error()
    assert call(scales=p + 32) == N.ERR_ARG and b"scales" in lib.risvec_last_error() and b"same" in lib.risvec_last_error()


def test_python_surface():
    import ris_vec_marl_amd as rv
    assert rv.pack_marl_critic_weights_device is MC.pack_marl_critic_weights_device
    assert "pack_marl_critic_weights_device" in rv.__all__
    assert list(inspect.signature(MC.pack_marl_critic_weights_device).parameters) == ["weights", "out", "workspace"]
    assert MC.BatchedTwinCritic.PACK_MODES == ("host", "device")
    assert isinstance(MC.BatchedTwinCritic.pack, property) and MC.BatchedTwinCritic.pack.fset is not None
    # the mode is a property, not a constructor argument: the parameter list is unchanged
    assert list(inspect.signature(MC.BatchedTwinCritic.__init__).parameters) == [
        "self", "state_dims", "action_dims", "fc1_dims", "fc2_dims", "fc3_dims", "n_nets", "device", "seed", "gemm"]


def test_device_pack_refuses_what_it_cannot_read_in_place_without_a_device():
    """The refusals that need no device: they are answered before anything is launched."""
    w = (torch.zeros(64, 48), torch.zeros(128, 64), torch.zeros(128, 128))
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights_device([w, w, w])                     # three nets
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights_device([])
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights_device([(w[0].double(), w[1], w[2])])
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights_device([(torch.zeros(48, 64).T, w[1], w[2])])
    with pytest.raises(ValueError):                                       # CPU tensors: nothing is moved to a device
        MC.pack_marl_critic_weights_device([w])
