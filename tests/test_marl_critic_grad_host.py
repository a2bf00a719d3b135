"""CPU-side tests of the critic loss and its gradients on the device (`BatchedTwinCritic.loss_backward`,
`risvec_marl_critic_grad`, csrc/k_marl_critic_grad.hip): the float64 oracle of marl_critic_grad_ref.py against
`torch.autograd` in float64, `nudge_biases`, the three exported symbols, the shape rule and the workspace size against their
Python restatements, and the argument checks of the entry point, which answer before touching a device."""
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
from tests import marl_critic_grad_ref as G

SYMBOLS = ("risvec_marl_critic_grad_supported", "risvec_marl_critic_grad_workspace", "risvec_marl_critic_grad")
DRIVER8 = (40, 80, 1024, 512, 256)


def autograd64(ws, state, action, target):
    F = torch.nn.functional
    x = torch.from_numpy(G._x64(state, action))
    y = torch.from_numpy(np.asarray(target, np.float64).reshape(-1))
    leaves, loss, qs = [], 0.0, []
    for w in ws:
        t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in w.items()}
        h = x
        for name in G.LAYERS:
            h = torch.relu(F.linear(h, t[name + ".weight"], t[name + ".bias"]))
        q = F.linear(h, t["q.weight"], t["q.bias"]).view(-1)
        loss = loss + F.mse_loss(q, y)
        leaves.append(t)
        qs.append(q.detach().numpy())
    loss.backward()
    return [{k: t[k].grad.numpy() for k in G.KEYS} for t in leaves], float(loss.detach()), qs


@pytest.mark.parametrize("dims,n,V", [((5, 10, 32, 128, 128), 33, 3), ((20, 24, 96, 512, 256), 97, 4), ((40, 88, 160, 256, 128), 31, None)])
def test_oracle_equals_autograd_in_float64(dims, n, V):
    ws = [G.random_net(dims, s) for s in (41, 42)]
    state, action = G.random_batch(dims, n, 7, V)
    target = np.random.default_rng(5).normal(0, 1, n)
    got, loss, qs = G.loss_grads64(ws, state, action, target)
    want, wloss, wq = autograd64(ws, state, action, target)
    assert abs(loss - wloss) <= 1e-12 * abs(wloss)
    for c in range(2):
        assert G.rel_err(qs[c], wq[c]) <= 1e-12
        for k in G.KEYS:
            assert got[c][k].shape == want[c][k].shape, k
            e = G.rel_err(got[c][k], want[c][k])
            assert e <= 1e-12, (c, k, e)


def test_nudge_biases_clears_the_guard():
    dims, n = (5, 10, 32, 128, 128), 33
    w = G.random_net(dims, 41)
    state, action = G.random_batch(dims, n, 7, 3)
    w2, nudged = G.nudge_biases(w, (state, action))
    assert 0 <= nudged <= 16
    zs, _, _ = G.forward64(w2, G._x64(state, action))
    for z in zs:
        assert not (np.abs(z) < 1e-4 * np.abs(z).max()).any()
    for k in G.KEYS:                                          # only biases move, and only upward
        if k.endswith("weight") or k == "q.bias":
            assert np.array_equal(w2[k], w[k])
        else:
            assert (w2[k] >= w[k]).all()
    # a unit planted on the kink is moved off it
    w3 = {k: v.copy() for k, v in w.items()}
    w3["fc1.weight"][0] = 0.0
    w3["fc1.bias"][0] = 0.0
    w4, nudged = G.nudge_biases(w3, (state, action))
    assert nudged >= 1 and w4["fc1.bias"][0] > 0


def test_library_declares_and_exports_the_grad_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "risvec.h")).read()
    lib = N.load()
    for name in SYMBOLS:
        assert name in N.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, header)
    m = re.search(r"#define RISVEC_ABI_VERSION (\d+)", header)
    assert int(m.group(1)) == N.ABI_VERSION == 17 == lib.risvec_abi_version()      # new symbols only
    for name in ("RisVecMarlCriticGradNet", "RisVecMarlCriticGrads"):
        assert re.search(r"\} %s;" % name, header)
    assert C.sizeof(N.RisVecMarlCriticGradNet) == C.sizeof(N.RisVecMarlCriticNet) + 16
    assert C.sizeof(N.RisVecMarlCriticGrads) == 64
    assert "k_marl_critic_grad.hip" in open(os.path.join(root, "ris_vec_marl_amd", "csrc", "Makefile")).read()


def test_grad_rule_and_workspace_agree_with_the_library():
    lib = N.load()
    sa = [(1, 1), (5, 10), (64, 64), (40, 88), (40, 89), (20, 24), (0, 80), (80, 0), (-3, 100)]
    n_ok = 0
    for (s, a), f1, f2, f3 in itertools.product(sa, (0, 32, 48, 96, 1024, 1056), (64, 128, 256, 384, 512), (64, 128, 256, 512)):
        dims = (s, a, f1, f2, f3)
        ok = bool(lib.risvec_marl_critic_grad_supported(*dims))
        assert ok == MC._supported(*dims) == bool(lib.risvec_marl_critic_supported(*dims)), dims
        for n, k in ((1, 1), (33, 2), (256, 2), (4096, 1)):
            b = lib.risvec_marl_critic_grad_workspace(n, *dims, k)
            assert b == MC.grad_workspace_bytes(n, *dims, k) and (b != 0) == ok, (dims, n, k)
        n_ok += ok
    assert n_ok == 5 * 3 * 3 * 2
    for n, k in ((0, 2), (-1, 2), (64, 0), (64, 3)):
        assert lib.risvec_marl_critic_grad_workspace(n, *DRIVER8, k) == 0 == MC.grad_workspace_bytes(n, *DRIVER8, k)
    # the formula, spelled out once: 256 rows of the driver's 8 vehicles, both nets
    assert MC.grad_workspace_bytes(256, *DRIVER8, 2) == 4 * (128 * 256 + 2 * (2 * 1792 * 256 + 2 * 256 + 24))
    # rows are padded to the tile: 33 rows cost what 64 do, and one more tile costs more
    assert MC.grad_workspace_bytes(33, *DRIVER8, 2) == MC.grad_workspace_bytes(64, *DRIVER8, 2) < MC.grad_workspace_bytes(65, *DRIVER8, 2)


def test_grad_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf = (C.c_float * 256)()                                 # host memory: never dereferenced, only checked
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    dims = DRIVER8
    nbytes = lib.risvec_marl_critic_stream_bytes(*dims)
    n0 = 64
    need = lib.risvec_marl_critic_grad_workspace(n0, *dims, 2)
    gfields = [f for f, _ in N.RisVecMarlCriticGrads._fields_]

    def call(n=n0, dims=dims, n_nets=2, nets="make", grads="make", wb=nbytes, bad_net=1, st=p, ac=p, tg=p, q1=p, q2=p + 16, loss=p + 32,
             ws=p, ws_bytes=need, gkw=None, W2=p, W3=p, **kw):
        if nets == "make":
            arr = (N.RisVecMarlCriticGradNet * 2)()
            for c in range(2):
                arr[c] = N.RisVecMarlCriticGradNet(N.RisVecMarlCriticNet(p, nbytes, p, p, p, p, p, p), p, p)
            arr[bad_net].fwd.wstream_bytes = wb
            arr[bad_net].W2, arr[bad_net].W3 = W2, W3
            for k, v in kw.items():
                setattr(arr[bad_net].fwd, k, v)
            nets = C.cast(arr, C.c_void_p)
        if grads == "make":
            ga = (N.RisVecMarlCriticGrads * 2)()
            for c in range(2):
                ga[c] = N.RisVecMarlCriticGrads(*(p + 64 + 4 * (8 * c + i) for i in range(8)))
            for k, v in (gkw or {}).items():
                setattr(ga[bad_net], k, v)
            grads = C.cast(ga, C.c_void_p)
        if n_nets == 1 and q2 == p + 16:
            q2 = None
        return lib.risvec_marl_critic_grad(n, *dims, n_nets, nets, grads, st, ac, tg, q1, q2, loss, ws, ws_bytes, None)
    # every call below carries exactly one fault: a complete set of host pointers is never passed
    for n in (0, -3):
        assert call(n=n) == N.ERR_ARG and b"risvec_marl_critic_grad: n_rows" in lib.risvec_last_error()
    for k in (0, 3, -1):
        assert call(n_nets=k) == N.ERR_ARG and b"n_nets" in lib.risvec_last_error()
    for bad in ((40, 89, 1024, 512, 256), (40, 80, 1000, 512, 256), (40, 80, 1024, 384, 256), (40, 80, 1024, 512, 512),
                (0, 80, 1024, 512, 256), (80, 288, 1024, 512, 256)):
        assert call(dims=bad) == N.ERR_UNSUPPORTED and b"risvec_marl_critic_grad" in lib.risvec_last_error()
    assert call(nets=None) == N.ERR_ARG and b"nets is NULL" in lib.risvec_last_error()
    assert call(grads=None) == N.ERR_ARG and b"grads is NULL" in lib.risvec_last_error()
    for net in (0, 1):
        assert call(wb=nbytes - 1024, bad_net=net) == N.ERR_ARG and b"wstream_bytes" in lib.risvec_last_error()
        for f in ("wstream", "scales", "b1", "b2", "b3", "qw", "qb"):
            assert call(bad_net=net, **{f: None}) == N.ERR_ARG, f
            assert b"nets[%d].%s is NULL" % (net, f.encode()) in lib.risvec_last_error()
        assert call(bad_net=net, W2=None) == N.ERR_ARG and b"W2 is NULL" in lib.risvec_last_error()
        assert call(bad_net=net, W3=None) == N.ERR_ARG and b"W3 is NULL" in lib.risvec_last_error()
        for f in gfields:
            assert call(bad_net=net, gkw={f: None}) == N.ERR_ARG, f
            assert b"grads[%d].%s is NULL" % (net, f.encode()) in lib.risvec_last_error()
    assert call(b2=p + 4) == N.ERR_ARG and b"16-byte aligned" in lib.risvec_last_error()
    assert call(W2=p + 2) == N.ERR_ARG and call(gkw={"dW2": p + 2}) == N.ERR_ARG
    assert call(gkw={"db1": p + 64}) == N.ERR_ARG and b"same buffer" in lib.risvec_last_error()    # net 2's db1 = net 1's dW1
    assert call(st=None) == N.ERR_ARG and call(ac=None) == N.ERR_ARG
    for k in ("tg", "q1", "q2", "loss", "ws"):
        assert call(**{k: None}) == N.ERR_ARG and b"is NULL" in lib.risvec_last_error(), k
    assert call(q2=p) == N.ERR_ARG and b"same buffer" in lib.risvec_last_error()
    assert call(n_nets=1, q2=p + 48) == N.ERR_ARG and b"q2" in lib.risvec_last_error()     # q2 without a second net
    assert call(ws=p + 4) == N.ERR_ARG
    assert call(ws_bytes=need - 1) == N.ERR_ARG and b"risvec_marl_critic_grad_workspace" in lib.risvec_last_error()
    assert call(n=n0 + 1) == N.ERR_ARG and b"workspace_bytes" in lib.risvec_last_error()    # one more tile needs more
    assert call(ws_bytes=0) == N.ERR_ARG


def test_python_surface_of_loss_backward():
    T = MC.BatchedTwinCritic
    assert list(inspect.signature(T.loss_backward).parameters) == ["self", "state", "action", "target", "grads", "q", "loss", "workspace"]
    assert list(inspect.signature(T.loss_backward_torch).parameters) == ["self", "state", "action", "target", "grads", "q", "loss"]
    assert list(inspect.signature(T.alloc_grads).parameters) == ["self"]
    lo, hi = T.GRAD_AUTO_ROWS
    assert isinstance(lo, int) and isinstance(hi, int)
    lib = N.load()

    def modes(dims, gemm):
        c = object.__new__(T)
        c._dims = dims
        c._init_modes(gemm, bool(lib.risvec_marl_critic_supported(*dims)), "a rule", bool(lib.risvec_marl_critic_wide_supported(*dims)))
        return c
    # an explicit gemm="fused" runs the device path at every row count; the library modes and other shapes never do
    c = modes(DRIVER8, "fused")
    assert c._grad_device(1) and c._grad_device(256) and c._grad_device(1 << 20)
    assert not modes(DRIVER8, "library")._grad_device(256) and not modes(DRIVER8, "wide")._grad_device(256)
    assert not modes((80, 288, 1024, 512, 256), None)._grad_device(256)
    c = modes(DRIVER8, None)
    for n in (1, 64, 256, 4096):
        assert c._grad_device(n) == (lo <= n <= hi)
    # the checks of the gradient tensors run on CPU tensors too
    from ris_vec_marl_amd import _critic_nets as CN
    cpu = torch.device("cpu")
    g = torch.Generator().manual_seed(0)
    nets = [CN.draw_net(g, 15, 32, 128, 128, cpu) for _ in range(2)]
    good = [[torch.zeros_like(getattr(net, a)) for a in CN._Net._WEIGHTS] for net in nets]
    assert [[t.shape for t in gs] for gs in CN.check_grads(good, nets, "t", cpu)] == [[getattr(n_, a).shape for a in CN._Net._WEIGHTS] for n_ in nets]
    with pytest.raises(ValueError):
        CN.check_grads(good[:1], nets, "t", cpu)
    with pytest.raises(ValueError):
        CN.check_grads([good[0], good[1][:7]], nets, "t", cpu)
    with pytest.raises(ValueError):
        CN.check_grads([good[0], [t.double() for t in good[1]]], nets, "t", cpu)
    with pytest.raises(ValueError):
        CN.check_grads([good[0], [t.t() for t in good[1]]], nets, "t", cpu)           # transposed: wrong shape / not contiguous
    with pytest.raises(ValueError):
        CN.check_grads([good[0], good[0]], nets, "t", cpu)                            # the same tensors twice
    with pytest.raises(ValueError):
        CN.check_grads(3, nets, "t", cpu)
