"""CPU-side tests of the chunked twin critic (`BatchedTwinCritic(gemm="wide")`, `risvec_marl_critic_wide`,
k_marl_critic_wide in csrc/k_marl_critic.hip): the five exported symbols, the wide shape rule and that the fused rule did
not move, the weight stream at shapes only the wide rule covers, the argument checks of the two entry points (which answer
before touching a device), and the packed stream walked through the kernel's CHUNKED data flow in NumPy -- the input staged
8 k-steps at a time, one accumulator per fc1 group carried across the chunks -- against the float64 restatement."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

from ris_vec_marl_amd import _native as N
from ris_vec_marl_amd import marl_critic as MC
from tests import marl_critic_ref as R

SYMBOLS = ("risvec_marl_critic_wide_supported", "risvec_marl_critic_wide_stream_bytes", "risvec_marl_critic_wide",
           "risvec_marl_critic_wide_pack_workspace", "risvec_marl_critic_wide_pack")
DRIVER16 = (80, 288, 1024, 512, 256)                           # 16 vehicles: 23 k-steps, chunks 8 + 8 + 7
SMALL9 = (40, 90, 96, 256, 256)                               # 9 k-steps, the last with 2 live columns: chunks 8 + 1
CHUNK = 8                                                     # kWideChunk


def test_library_declares_and_exports_the_wide_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "risvec.h")).read()
    lib = N.load()
    for name in SYMBOLS:
        assert name in N.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, header)
    m = re.search(r"#define RISVEC_ABI_VERSION (\d+)", header)
    assert int(m.group(1)) == N.ABI_VERSION == 17             # new symbols only: the ABI version stays
    # the wide entries take the argument lists of the ones they stand beside
    for wide, narrow in (("risvec_marl_critic_wide", "risvec_marl_critic"), ("risvec_marl_critic_wide_pack", "risvec_marl_critic_pack"),
                         ("risvec_marl_critic_wide_pack_workspace", "risvec_marl_critic_pack_workspace"),
                         ("risvec_marl_critic_wide_stream_bytes", "risvec_marl_critic_stream_bytes"),
                         ("risvec_marl_critic_wide_supported", "risvec_marl_critic_supported")):
        assert N._PROTOS[wide] == N._PROTOS[narrow]


def test_wide_rule_agrees_with_the_library_over_a_grid():
    lib = N.load()
    sa = [(1, 1), (64, 64), (40, 89), (40, 90), (80, 288), (256, 256), (1, 511), (511, 1), (256, 257), (512, 1), (0, 80), (80, 0),
          (0, 0), (-3, 100)]
    assert {s + a for s, a in sa} >= {2, 128, 129, 130, 368, 512, 513}
    grid = list(itertools.product(sa, (0, 16, 32, 48, 96, 1000, 1024, 1056), (64, 128, 256, 384, 512, 1024), (64, 128, 192, 256, 512)))
    n_ok = 0
    for (s, a), f1, f2, f3 in grid:
        dims = (s, a, f1, f2, f3)
        ok = bool(lib.risvec_marl_critic_wide_supported(*dims))
        assert ok == MC._supported_wide(*dims), dims
        assert (lib.risvec_marl_critic_wide_stream_bytes(*dims) != 0) == ok, dims
        assert (lib.risvec_marl_critic_wide_pack_workspace(*dims, 2) != 0) == ok, dims
        want = s >= 1 and a >= 1 and s + a <= 512 and f1 % 32 == 0 and 32 <= f1 <= 1024 and f2 in (128, 256, 512) and f3 in (128, 256)
        assert ok == want, dims
        if lib.risvec_marl_critic_supported(*dims):            # the rules overlap: what the fused rule takes, the wide one takes
            assert ok and lib.risvec_marl_critic_wide_stream_bytes(*dims) == lib.risvec_marl_critic_stream_bytes(*dims)
        n_ok += ok
    assert n_ok == 8 * 3 * 3 * 2                              # 8 input pairs, fc1 in {32, 96, 1024}, 3 fc2, 2 fc3
    # each edge of the rule
    for dims, ok in (((80, 432, 1024, 512, 256), 1), ((80, 433, 1024, 512, 256), 0), ((80, 288, 1024 + 32, 512, 256), 0),
                     ((80, 288, 1000, 512, 256), 0), ((80, 288, 32, 512, 256), 1), ((80, 288, 0, 512, 256), 0),
                     ((80, 288, 1024, 64, 256), 0), ((80, 288, 1024, 384, 256), 0), ((80, 288, 1024, 128, 128), 1),
                     ((80, 288, 1024, 512, 512), 0), ((80, 288, 1024, 512, 64), 0), ((0, 288, 1024, 512, 256), 0),
                     ((80, 0, 1024, 512, 256), 0)):
        assert lib.risvec_marl_critic_wide_supported(*dims) == ok == int(MC._supported_wide(*dims)), dims
    for n_nets, ok in ((0, 0), (1, 1), (2, 1), (3, 0)):
        assert (lib.risvec_marl_critic_wide_pack_workspace(*DRIVER16, n_nets) != 0) == bool(ok)
    # the fused rule is where it was: 16 vehicles are not its shape
    assert lib.risvec_marl_critic_supported(*DRIVER16) == 0 and not MC._supported(*DRIVER16)
    assert lib.risvec_marl_critic_stream_bytes(*DRIVER16) == 0 and lib.risvec_marl_critic_pack_workspace(*DRIVER16, 2) == 0
    assert lib.risvec_marl_critic_wide_supported(*DRIVER16) == 1


def torch_weights(dims, seed):
    w = R.random_net(dims, seed)
    t = lambda k: torch.from_numpy(w[k])                      # noqa: E731
    return w, dict(W1=t("fc1.weight"), W2=t("fc2.weight"), W3=t("fc3.weight"))


@pytest.mark.parametrize("dims", [DRIVER16, SMALL9])
def test_wide_packing_round_trip_and_stream_size(dims):
    """The stream of a shape only the wide rule covers: the byte size the library states, hi + lo with the recorded scale
    within 2^-21 of each matrix's largest entry (the bar of the fused round-trip test), and the wide kernel's LDS -- one
    chunk of input fragments, the widest activation, the reduction slots -- within the 160 KiB of a CU."""
    lib = N.load()
    _, tw = torch_weights(dims, 3)
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights(tw["W1"], tw["W2"], tw["W3"])             # the three-argument call refuses as before
    stream, scales = MC.pack_marl_critic_weights(wide=True, **tw)
    g = MC.marl_critic_geom(*dims)
    S, A, F1, F2, F3 = dims
    assert (g.ks, g.ng, g.mt2, g.mt3) == (-(-(S + A) // 16), F1 // 32, F2 // 128, F3 // 128) and g.ks > CHUNK
    assert stream.dtype == torch.float16 and tuple(stream.shape) == (g.rows, 64, 8) and stream.is_contiguous()
    assert stream.numel() * 2 == g.rows * 1024 == lib.risvec_marl_critic_wide_stream_bytes(*dims)
    lds = (CHUNK + max(2 * g.ng, F2 // 16)) * 2048 + 1024
    assert lds <= 160 * 1024
    if dims == DRIVER16:
        assert lds == 145 * 1024                              # what (40, 80) runs with in the fused kernel
        assert (g.ks + max(2 * g.ng, F2 // 16)) * 2048 + 1024 > 160 * 1024        # why the fused kernel is not built here
    assert tuple(scales.shape) == (3,) and scales.dtype == torch.float32
    un = MC._unpack(stream, scales, *dims)
    want = {"fc1": tw["W1"].double().T, "fc2": tw["W2"].double().T, "fc3": tw["W3"].double().T}
    assert set(un) == set(want)
    for k in want:
        assert un[k].shape == want[k].shape, k
        assert float((un[k] - want[k]).abs().max()) <= 2.0 ** -21 * float(want[k].abs().max()), k


def test_wide_packing_is_the_fused_packing_where_both_rules_hold():
    _, tw = torch_weights((40, 80, 96, 256, 256), 5)
    a, b = MC.pack_marl_critic_weights(**tw), MC.pack_marl_critic_weights(wide=True, **tw)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights(torch.zeros(96, 513), tw["W2"], tw["W3"], wide=True)          # 513 inputs
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights(torch.zeros(96, 368), tw["W2"], torch.zeros(64, 256), wide=True)   # fc3 = 64


def test_wide_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf = (C.c_float * 64)()                                  # host memory: never dereferenced, only checked
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    dims = DRIVER16
    nbytes = lib.risvec_marl_critic_wide_stream_bytes(*dims)
    assert nbytes == MC.marl_critic_geom(*dims).rows * 1024
    fields = ("wstream", "scales", "b1", "b2", "b3", "qw", "qb")

    def call(n=4, dims=dims, n_nets=2, nets="make", wb=nbytes, bad_net=1, st=p, ac=p, rw=p, dn=p, gamma=0.99, coef=p, lp=p, li=p,
             q1=p, q2=p, y=p, **kw):
        if nets == "make":
            arr = (N.RisVecMarlCriticNet * 2)()
            for c in range(2):
                arr[c] = N.RisVecMarlCriticNet(p, nbytes, p, p, p, p, p, p)
            arr[bad_net].wstream_bytes = wb
            for k, v in kw.items():
                setattr(arr[bad_net], k, v)
            nets = C.cast(arr, C.c_void_p)
        return lib.risvec_marl_critic_wide(n, *dims, n_nets, nets, st, ac, rw, dn, gamma, coef, lp, li, q1, q2, y, None)
    # every call below carries exactly one fault: a complete set of host pointers is never passed
    for n in (0, -3):
        assert call(n=n) == N.ERR_ARG and b"risvec_marl_critic_wide" in lib.risvec_last_error()
    for k in (0, 3, -1):
        assert call(n_nets=k) == N.ERR_ARG and b"n_nets" in lib.risvec_last_error()
    for bad in ((80, 433, 1024, 512, 256), (80, 288, 1000, 512, 256), (80, 288, 1024, 384, 256), (80, 288, 1024, 512, 512),
                (0, 288, 1024, 512, 256)):
        assert call(dims=bad) == N.ERR_UNSUPPORTED
        assert b"risvec_marl_critic_wide" in lib.risvec_last_error()
    assert call(nets=None) == N.ERR_ARG
    other = lib.risvec_marl_critic_wide_stream_bytes(80, 272, 1024, 512, 256)        # one k-step fewer
    assert 0 < other < nbytes
    for net in (0, 1):
        for wb in (other, nbytes - 1024):
            assert call(wb=wb, bad_net=net) == N.ERR_ARG      # a stream packed for another shape
            assert b"wstream_bytes" in lib.risvec_last_error()
        for f in fields:
            assert call(bad_net=net, **{f: None}) == N.ERR_ARG, f
    assert call(b2=p + 4) == N.ERR_ARG                        # not 16-byte aligned
    assert call(st=None) == N.ERR_ARG and call(ac=None) == N.ERR_ARG
    assert call(q1=None, q2=None, y=None, lp=None, li=None) == N.ERR_ARG      # at least one output
    assert call(n_nets=1) == N.ERR_ARG and b"q2" in lib.risvec_last_error()   # q2 without a second net
    assert call(rw=None) == N.ERR_ARG and call(dn=None) == N.ERR_ARG          # y needs reward and done
    assert call(coef=None) == N.ERR_ARG and b"coef" in lib.risvec_last_error()
    assert call(y=None) == N.ERR_ARG                          # the entropy inputs without y
    for g in (float("nan"), float("inf")):
        assert call(gamma=g) == N.ERR_ARG and b"gamma" in lib.risvec_last_error()
    # the fused entry still refuses the shape
    arr = (N.RisVecMarlCriticNet * 2)()
    assert lib.risvec_marl_critic(4, *dims, 2, C.cast(arr, C.c_void_p), p, p, p, p, 0.99, p, p, p, p, p, p, None) == N.ERR_UNSUPPORTED


def test_wide_pack_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    dims = DRIVER16
    nbytes = lib.risvec_marl_critic_wide_stream_bytes(*dims)
    need = lib.risvec_marl_critic_wide_pack_workspace(*dims, 2)
    assert need == lib.risvec_marl_critic_pack_workspace(40, 80, 1024, 512, 256, 2) > 0

    def call(dims=dims, n_nets=2, nets="make", wb=nbytes, bad_net=1, ws=p, ws_bytes=need, same=None, **kw):
        if nets == "make":
            arr = (N.RisVecMarlCriticPackNet * 2)()
            for c in range(2):
                arr[c] = N.RisVecMarlCriticPackNet(p, p, p, p + 16 * c, nbytes, p + 32 + 16 * c)
            arr[bad_net].wstream_bytes = wb
            for k, v in kw.items():
                setattr(arr[bad_net], k, v)
            if same:
                setattr(arr[1], same, getattr(arr[0], same))
            nets = C.cast(arr, C.c_void_p)
        return lib.risvec_marl_critic_wide_pack(*dims, n_nets, nets, ws, ws_bytes, None)
    for k in (0, 3, -1):
        assert call(n_nets=k) == N.ERR_ARG and b"n_nets" in lib.risvec_last_error()
    for bad in ((80, 433, 1024, 512, 256), (80, 288, 1000, 512, 256), (80, 288, 1024, 384, 256)):
        assert call(dims=bad) == N.ERR_UNSUPPORTED and b"risvec_marl_critic_wide_pack" in lib.risvec_last_error()
    assert call(nets=None) == N.ERR_ARG
    for net in (0, 1):
        assert call(wb=nbytes - 1024, bad_net=net) == N.ERR_ARG and b"wstream_bytes" in lib.risvec_last_error()
        for f in ("W1", "W2", "W3", "wstream", "scales"):
            assert call(bad_net=net, **{f: None}) == N.ERR_ARG, f
    assert call(W2=p + 2) == N.ERR_ARG and call(wstream=p + 4) == N.ERR_ARG
    assert call(same="wstream") == N.ERR_ARG and call(same="scales") == N.ERR_ARG
    assert call(ws=None) == N.ERR_ARG
    assert call(ws_bytes=need - 1) == N.ERR_ARG and b"risvec_marl_critic_wide_pack_workspace" in lib.risvec_last_error()
    # the fused pack entry still refuses the shape
    arr = (N.RisVecMarlCriticPackNet * 2)()
    assert lib.risvec_marl_critic_pack(*dims, 2, C.cast(arr, C.c_void_p), p, 4096, None) == N.ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------
# k_marl_critic_wide's data flow on the packed stream, in NumPy.  fc1 is what differs from the walk in marl_critic_ref.py:
# s_in holds CHUNK k-steps, every group keeps ONE accumulator across the chunks and adds the k-steps in ascending order,
# and bias, ReLU and the split go to s_h after the last chunk.  From there on (fc2, fc3, q) it is that walk's.
def walk_stream_wide(stream, scales, w, state, action, dims, g):
    S_, A_, F1, F2, F3 = dims
    St = np.asarray(stream).astype(np.float64)
    u1, u2, u3 = (float(s) for s in np.asarray(scales))
    st = np.asarray(state, np.float32).reshape(len(state), -1)
    ac = np.asarray(action, np.float32).reshape(len(action), -1)
    n = len(st)
    lane = np.arange(64)
    out = np.zeros(n)
    chunks = []

    def gemm(base, wave, nks, mt, sb):
        acc = [np.zeros((32, 32)) for _ in range(mt)]
        for s in range(nks):
            for m in range(mt):
                row = base + ((wave * nks + s) * mt + m) * 2
                acc[m] += R._mfma3(St[row], St[row + 1], sb[s, 0], sb[s, 1])
        return [R._to_regs(d) for d in acc]

    def put(sh, tile, y):
        for u in range(2):
            hi, lo = R._split(y[:, 8 * u:8 * u + 8])
            sh[2 * tile + u, 0], sh[2 * tile + u, 1] = hi, lo

    def rowsum(v):
        s = v.sum(-1)
        return (s[:32] + s[32:])[lane & 31]

    for e0 in range(0, n, 32):
        rows = np.where(e0 + np.arange(32) < n, e0 + np.arange(32), 0)
        rr = rows[lane & 31][None, :, None]
        d = [np.zeros((32, 32)) for _ in range(g.ng)]         # per group, kept across the chunks
        chunks = []
        for c in range(-(-g.ks // CHUNK)):
            cs = min(CHUNK, g.ks - CHUNK * c)
            chunks.append(cs)
            # the chunk staged from two pointers: k < S from state, S <= k < S + A from action, zero beyond
            k = 16 * (CHUNK * c + np.arange(cs))[:, None, None] + 8 * (lane >> 5)[None, :, None] + np.arange(8)[None, None, :]
            v = np.where(k < S_, st[rr, np.minimum(k, S_ - 1)], np.where(k < S_ + A_, ac[rr, np.clip(k - S_, 0, A_ - 1)], 0.0))
            hi, lo = R._split(v)
            s_in = np.zeros((CHUNK, 2, 64, 8))
            s_in[:cs, 0], s_in[:cs, 1] = hi, lo
            for grp in range(g.ng):
                for s in range(cs):
                    row = g.fc1 + (grp * g.ks + CHUNK * c + s) * 2
                    d[grp] += R._mfma3(St[row], St[row + 1], s_in[s, 0], s_in[s, 1])
        s_h = np.zeros((max(2 * g.ng, 8 * g.mt2), 2, 64, 8))
        for grp in range(g.ng):
            put(s_h, grp, np.maximum(R._to_regs(d[grp]) * u1 + R._tab(w["fc1.bias"], 32 * grp), 0.0))
        acc = [gemm(g.fc2, wv, 2 * g.ng, g.mt2, s_h) for wv in range(4)]
        s_h = np.zeros_like(s_h)
        for wv in range(4):
            for m in range(g.mt2):
                t = wv * g.mt2 + m
                put(s_h, t, np.maximum(acc[wv][m] * u2 + R._tab(w["fc2.bias"], 32 * t), 0.0))
        a3 = [gemm(g.fc3, wv, 8 * g.mt2, g.mt3, s_h) for wv in range(4)]
        q = np.zeros(64)
        for wv in range(4):
            for m in range(g.mt3):
                f0 = 32 * (wv * g.mt3 + m)
                y = np.maximum(a3[wv][m] * u3 + R._tab(w["fc3.bias"], f0), 0.0)
                q += rowsum(y * R._tab(np.asarray(w["q.weight"]).reshape(-1), f0))
        q = q[:32] + float(np.asarray(w["q.bias"]).reshape(-1)[0])
        m_ = e0 + np.arange(32) < n
        out[e0 + np.arange(32)[m_]] = q[m_]
    return out, chunks


# 130, 250 and 360 inputs end on a partial k-step (2, 10 and 8 live columns); 368 fill their 23 k-steps; 120 are one chunk
@pytest.mark.parametrize("dims,chunks", [(SMALL9, [8, 1]), ((64, 186, 96, 256, 256), [8, 8]), ((80, 280, 64, 128, 128), [8, 8, 7]),
                                         ((80, 288, 96, 128, 256), [8, 8, 7]), ((40, 80, 96, 256, 256), [8])])
def test_numpy_walk_of_the_packed_stream_in_chunks(dims, chunks):
    """The bar is the one of the fused kernel's NumPy walk (test_marl_critic_host.py), which sits at 0.9e-7 ... 3.3e-7 of the
    batch scale: what is left is the split's rounding, 2^-22 per product."""
    w, tw = torch_weights(dims, 11)
    stream, scales = MC.pack_marl_critic_weights(wide=True, **tw)
    state, action = R.random_batch(dims, 37, 12)
    got, walked = walk_stream_wide(stream.numpy(), scales.numpy(), w, state, action, dims, MC.marl_critic_geom(*dims))
    assert walked == chunks
    e = R.err(got, R.critic_q64(w, state, action))
    print("chunked walk %s, chunks %s: err %.3g" % (dims, chunks, e))
    assert e < 1e-6
    if len(chunks) == 1:                                      # one chunk: the fused kernel's walk, to the last bit of the float64 sums
        same = R.walk_stream(stream.numpy(), scales.numpy(), w, state, action, dims, MC.marl_critic_geom(*dims))
        assert np.array_equal(got, same)


def test_python_surface_of_the_wide_mode():
    T = MC.BatchedTwinCritic
    assert T.GEMM_MODES == ("fused", "library", "wide")
    assert list(inspect.signature(T.__init__).parameters) == [
        "self", "state_dims", "action_dims", "fc1_dims", "fc2_dims", "fc3_dims", "n_nets", "device", "seed", "gemm"]
    assert inspect.signature(MC.pack_marl_critic_weights).parameters["wide"].default is False
    assert list(inspect.signature(MC.pack_marl_critic_weights_wide_device).parameters) == ["weights", "out", "workspace"]
    import ris_vec_marl_amd as rv
    assert rv.pack_marl_critic_weights_wide_device is MC.pack_marl_critic_weights_wide_device
    assert "pack_marl_critic_weights_wide_device" in rv.__all__
    w = (torch.zeros(64, 368), torch.zeros(128, 64), torch.zeros(128, 128))
    with pytest.raises(ValueError):                           # CPU tensors: nothing is moved to a device
        MC.pack_marl_critic_weights_wide_device([w])
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights_wide_device([w, w, w])
    from ris_vec_marl_amd import _weights as W
    # the mode is refused where the wide rule does not hold, accepted where it does, and never the default
    for fused_ok in (False, True):
        with pytest.raises(ValueError, match="gemm='wide' is not available"):
            W.choose_mode("gemm", "wide", "library", T.GEMM_MODES, fused_ok, "a shape", "a rule", False)
        assert W.choose_mode("gemm", "wide", "library", T.GEMM_MODES, fused_ok, "a shape", "a rule", True) == "wide"
        assert W.choose_mode("gemm", None, "fused" if fused_ok else "library", T.GEMM_MODES, fused_ok, "a shape", "a rule",
                             True) == ("fused" if fused_ok else "library")
    with pytest.raises(ValueError):
        W.choose_mode("gemm", "wide", "library", ("fused", "library"), True, "a shape", "a rule", True)   # a class without the mode
    # the constructor's own call of `_init_modes`, on an object that holds the dimensions only
    lib = N.load()

    def modes(dims, gemm):
        c = object.__new__(T)
        c._dims = dims
        c._init_modes(gemm, bool(lib.risvec_marl_critic_supported(*dims)), "a rule", bool(lib.risvec_marl_critic_wide_supported(*dims)))
        return c
    for dims in ((80, 433, 1024, 512, 256), (80, 288, 1000, 512, 256), (80, 288, 1024, 384, 256)):
        with pytest.raises(ValueError, match="gemm='wide' is not available for state_dims=80"):
            modes(dims, "wide")
    c = modes(DRIVER16, None)
    assert (c.gemm, c.pack, c._wide) == ("library", "host", False)
    with pytest.raises(ValueError):
        c.pack = "device"                                     # the library mode at 16 vehicles has no stream to pack
    with pytest.raises(ValueError):
        modes(DRIVER16, "fused")
    c = modes(DRIVER16, "wide")
    assert (c.gemm, c.pack, c._wide, c._fused(1)) == ("wide", "host", True, True)
    c = modes((40, 80, 1024, 512, 256), None)
    assert (c.gemm, c._wide) == ("fused", False)              # never chosen by default, where both rules hold either
    assert modes((40, 80, 1024, 512, 256), "wide").gemm == "wide"
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            T(80, 288, device="cpu", gemm="wide")
