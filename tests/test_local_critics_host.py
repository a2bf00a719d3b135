"""CPU-side tests of the local twin critics (`BatchedLocalCritics`, `risvec_local_critics`): the exported symbols, the
shape rule against a Python restatement, and every argument check of the C entry point, which must answer with its error
code and the offending name before touching a device."""
import ctypes as C
import itertools
import os
import re

import ris_vec_marl_amd
from ris_vec_marl_amd import _native as N
from ris_vec_marl_amd import marl_critic as MC


def supported(V, S, A, F1, F2, F3):
    """The rule of `risvec_local_critics_supported`, restated: 1 <= n_agents <= 16 and the twin critic's rule at (S, A)."""
    return (1 <= V <= 16 and S >= 1 and A >= 1 and S + A <= 128 and F1 >= 32 and F1 % 32 == 0 and F1 <= 1024
            and F2 in (128, 256, 512) and F3 in (128, 256))


def test_library_declares_and_exports_the_local_critics():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "risvec.h")).read()
    lib = N.load()
    for name in ("risvec_local_critics_supported", "risvec_local_critics"):
        assert name in N.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, header)
    m = re.search(r"#define RISVEC_ABI_VERSION (\d+)", header)
    assert int(m.group(1)) == N.ABI_VERSION == lib.risvec_abi_version() == 17     # new symbols only: the ABI version stays


def test_class_is_public():
    assert "BatchedLocalCritics" in ris_vec_marl_amd.__all__
    from ris_vec_marl_amd import BatchedLocalCritics
    from ris_vec_marl_amd.local_critics import BatchedLocalCritics as direct
    assert BatchedLocalCritics is direct and BatchedLocalCritics._SD == MC.BatchedTwinCritic._SD


def test_supported_rule_agrees_with_the_restatement_over_a_grid():
    lib = N.load()
    grid = list(itertools.product((0, 1, 4, 8, 16, 17), ((5, 10), (5, 123), (5, 124), (1, 127), (0, 10), (5, 0), (64, 64), (64, 65)),
                                  (0, 32, 48, 96, 1024, 1056), (64, 128, 256, 384, 512), (64, 128, 256, 512)))
    n_ok = 0
    for V, (S, A), F1, F2, F3 in grid:
        ok = bool(lib.risvec_local_critics_supported(V, S, A, F1, F2, F3))
        assert ok == supported(V, S, A, F1, F2, F3), (V, S, A, F1, F2, F3)
        assert ok == (1 <= V <= 16 and MC._supported(S, A, F1, F2, F3))
        n_ok += ok
    assert n_ok == 4 * 4 * 3 * 3 * 2                          # V in {1, 4, 8, 16}; S + A in {15, 128, 128, 128}
    for V, ok in ((0, 0), (1, 1), (16, 1), (17, 0)):
        assert lib.risvec_local_critics_supported(V, 5, V + 2, 1024, 512, 256) == ok
    assert lib.risvec_local_critics_supported(8, 5, 123, 1024, 512, 256) == 1         # S + A = 128
    assert lib.risvec_local_critics_supported(8, 5, 124, 1024, 512, 256) == 0         # S + A = 129
    assert lib.risvec_local_critics_supported(8, 5, 10, 1024, 384, 256) == 0


def test_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf = (C.c_float * 64)()                                  # host memory: never dereferenced, only checked
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    V, dims = 8, (5, 10, 1024, 512, 256)
    nbytes = lib.risvec_marl_critic_stream_bytes(*dims)
    fields = ("wstream", "scales", "b1", "b2", "b3", "qw", "qb")

    def call(n=4, V=V, dims=dims, n_nets=2, nets="make", wb=nbytes, bad_net=1, obs=p, ac=p, hd=None, pw=None, rw=p, dn=p,
             gamma=0.99, coef=p, lp=p, li=p, q1=p, q2=p, y=p, **kw):
        if nets == "make":
            count = max(V, 1) * 2
            arr = (N.RisVecMarlCriticNet * count)()
            for c in range(count):
                arr[c] = N.RisVecMarlCriticNet(p, nbytes, p, p, p, p, p, p)
            arr[bad_net].wstream_bytes = wb
            for k, v in kw.items():
                setattr(arr[bad_net], k, v)
            nets = C.cast(arr, C.c_void_p)
        return lib.risvec_local_critics(n, V, *dims, n_nets, nets, obs, ac, hd, pw, rw, dn, gamma, coef, lp, li, q1, q2, y, None)

    def refused(code, name, **kw):
        assert call(**kw) == code, kw
        err = lib.risvec_last_error()
        assert b"risvec_local_critics" in err and name in err, (kw, err)
    # every call below carries exactly one fault: a complete set of host pointers is never passed
    for n in (0, -3):
        refused(N.ERR_ARG, b"n_rows", n=n)
    for k in (0, 3, -1):
        refused(N.ERR_ARG, b"n_nets", n_nets=k)
    for bad_v in (0, 17, -1):
        refused(N.ERR_UNSUPPORTED, b"n_agents", V=bad_v)
    for bad in ((5, 124, 1024, 512, 256), (5, 10, 1000, 512, 256), (5, 10, 1024, 384, 256), (5, 10, 1024, 512, 512),
                (0, 10, 1024, 512, 256)):
        refused(N.ERR_UNSUPPORTED, b"fc2", dims=bad)
    refused(N.ERR_ARG, b"nets", nets=None)
    for net in (0, 1, 2 * V - 1):                             # the first agent's two and the last agent's second
        refused(N.ERR_ARG, b"wstream_bytes", wb=nbytes - 1024, bad_net=net)
        for f in fields:
            refused(N.ERR_ARG, f.encode(), bad_net=net, **{f: None})
    refused(N.ERR_ARG, b"b2", b2=p + 4)                       # not 16-byte aligned
    refused(N.ERR_ARG, b"obs", obs=None)
    refused(N.ERR_ARG, b"heads", hd=p, pw=p)                  # both forms
    refused(N.ERR_ARG, b"heads", ac=None)                     # neither
    refused(N.ERR_ARG, b"power", ac=None, hd=p)               # heads without power
    refused(N.ERR_ARG, b"power", pw=p)                        # power without heads
    refused(N.ERR_ARG, b"action_dims", ac=None, hd=p, pw=p, dims=(5, 11, 1024, 512, 256))     # heads with A != n_agents + 2
    assert call(ac=None, hd=p, pw=p, dims=(5, 10, 1024, 512, 256), n=0) == N.ERR_ARG          # (a valid from-policy set)
    refused(N.ERR_ARG, b"q1", q1=None, q2=None, y=None, lp=None, li=None)                     # at least one output
    refused(N.ERR_ARG, b"q2", n_nets=1)                       # q2 without a second net
    refused(N.ERR_ARG, b"reward", rw=None)
    refused(N.ERR_ARG, b"done", dn=None)                      # y needs reward and done
    refused(N.ERR_ARG, b"coef", coef=None)
    refused(N.ERR_ARG, b"coef", coef=None, lp=None)
    refused(N.ERR_ARG, b"coef", coef=None, li=None)
    refused(N.ERR_ARG, b"logp", y=None)                       # the entropy inputs without y
    for g in (float("nan"), float("inf"), -float("inf")):
        refused(N.ERR_ARG, b"gamma", gamma=g)
