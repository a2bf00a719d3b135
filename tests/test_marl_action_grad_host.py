"""CPU-side tests of d min(q1, q2) / d action on the device (`BatchedTwinCritic.action_grad`, `risvec_marl_critic_action_grad`,
csrc/k_marl_critic_action_grad.hip): the float64 oracle of marl_action_grad_ref.py against `torch.autograd` in float64 -- the tie
rule of `torch.min`'s backward included -- and against central differences, the three exported symbols, the workspace size,
the argument checks of the entry point, which answer before touching a device, and the Python surface."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ris_vec_marl_amd import _native as N
from ris_vec_marl_amd import marl_critic as MC
from tests import marl_action_grad_ref as R
from tests import marl_critic_grad_ref as G

SYMBOLS = ("risvec_marl_critic_action_grad_supported", "risvec_marl_critic_action_grad_workspace", "risvec_marl_critic_action_grad")
DRIVER8 = (40, 80, 1024, 512, 256)
SMALL = (5, 10, 32, 128, 128)
ODD = (20, 24, 96, 512, 256)


def autograd64(ws, state, action, scale):
    """The statements of `action_grad_torch`, in float64 on the CPU -> (out, q_min, [q_c])"""
    F = torch.nn.functional
    n = len(state)
    a = torch.tensor(np.asarray(action, np.float64).reshape(n, -1), requires_grad=True)
    x = torch.cat([torch.from_numpy(np.asarray(state, np.float64).reshape(n, -1)), a], 1)
    qs = []
    for w in ws:
        h = x
        for name in G.LAYERS:
            h = torch.relu(F.linear(h, torch.from_numpy(np.asarray(w[name + ".weight"], np.float64)),
                                    torch.from_numpy(np.asarray(w[name + ".bias"], np.float64))))
        qs.append(F.linear(h, torch.from_numpy(np.asarray(w["q.weight"], np.float64)),
                           torch.from_numpy(np.asarray(w["q.bias"], np.float64))))
    m = torch.min(qs[0], qs[1]) if len(ws) == 2 else qs[0]
    g, = torch.autograd.grad(m.sum(), a)
    return (g * scale).numpy(), m.detach().numpy()[:, 0], [q.detach().numpy()[:, 0] for q in qs]


@pytest.mark.parametrize("dims,n,n_nets", [(SMALL, 33, 2), (ODD, 41, 2), (SMALL, 33, 1)])
def test_oracle_equals_autograd_in_float64(dims, n, n_nets):
    inp = R.inputs(dims, n, n_nets, 41, 7)
    scale = -1.0 / n
    out, q_min, qs, gs = R.action_grad64(inp.ws, inp.state, inp.action, scale)
    wout, wmin, wq = autograd64(inp.ws, inp.state, inp.action, scale)
    assert out.shape == wout.shape == (n, dims[1])
    assert R.rel_err(out, wout) <= 1e-12 and R.rel_err(q_min, wmin) <= 1e-12
    for c in range(n_nets):
        assert R.rel_err(qs[c], wq[c]) <= 1e-12
    if n_nets == 2:                                           # both nets are selected somewhere, so a swapped select would show
        assert (qs[0] < qs[1]).any() and (qs[0] > qs[1]).any()
        assert R.rel_err(scale * gs[0], wout) > 1e-3 and R.rel_err(scale * gs[1], wout) > 1e-3


@pytest.mark.parametrize("dims,n", [(SMALL, 34), (ODD, 40)])
def test_oracle_tie_rule_is_autograds(dims, n):
    """On the planted rows q_1 == q_2 bit for bit while g_1 != g_2, and `torch.min`'s backward gives each net half."""
    inp, tie = R.tie_inputs(dims, n, 61, 17)
    out, q_min, qs, gs = R.action_grad64(inp.ws, inp.state, inp.action, 1.0)
    assert tie.sum() == n // 2
    assert np.array_equal(qs[0][tie], qs[1][tie]) and not (qs[0][~tie] == qs[1][~tie]).any()
    assert R.rel_err(gs[0][tie], gs[1][tie]) > 1e-2
    assert np.array_equal(out[tie], 0.5 * (gs[0][tie] + gs[1][tie]))
    wout, wmin, wq = autograd64(inp.ws, inp.state, inp.action, 1.0)
    assert np.array_equal(wq[0][tie], wq[1][tie])             # a tie for autograd too
    assert R.rel_err(out[tie], wout[tie]) <= 1e-12 and R.rel_err(out, wout) <= 1e-12
    for one in gs:                                            # neither "the first net" nor "the second" is autograd's rule
        assert R.rel_err(one[tie], wout[tie]) > 1e-2


def test_oracle_meets_central_differences():
    """min(q_1, q_2) is piecewise linear in the action and `nudge_biases` keeps every unit 1e-4 of its layer's scale away from
    its kink, so a central difference with a step of 1e-6 is the derivative up to its own rounding."""
    dims, n = ODD, 41
    inp = R.inputs(dims, n, 2, 41, 7)
    out, *_ = R.action_grad64(inp.ws, inp.state, inp.action, 1.0)
    rng = np.random.default_rng(3)
    step = 1e-6
    for b, a in zip(rng.integers(0, n, 24), rng.integers(0, dims[1], 24)):
        act = np.asarray(inp.action, np.float64).copy()
        act[b, a] += step
        up = R.action_grad64(inp.ws, inp.state, act)[1].sum()
        act[b, a] -= 2 * step
        dn = R.action_grad64(inp.ws, inp.state, act)[1].sum()
        fd = (up - dn) / (2 * step)
        assert abs(fd - out[b, a]) <= 1e-7 * np.abs(out).max(), (b, a, fd, out[b, a])


def test_library_declares_and_exports_the_action_grad_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "risvec.h")).read()
    lib = N.load()
    for name in SYMBOLS:
        assert name in N.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, header)
    m = re.search(r"#define RISVEC_ABI_VERSION (\d+)", header)
    assert int(m.group(1)) == N.ABI_VERSION == 17 == lib.risvec_abi_version()      # new symbols only
    assert re.search(r"\} RisVecMarlCriticActionGradNet;", header)
    assert C.sizeof(N.RisVecMarlCriticActionGradNet) == C.sizeof(N.RisVecMarlCriticNet) + 24
    assert "k_marl_critic_action_grad.hip" in open(os.path.join(root, "ris_vec_marl_amd", "csrc", "Makefile")).read()


def test_action_grad_rule_and_workspace():
    lib = N.load()
    for dims in (DRIVER8, SMALL, (1, 127, 1024, 128, 256), (127, 1, 160, 256, 128), (40, 89, 1024, 512, 256), (40, 80, 1000, 512, 256),
                 (0, 80, 1024, 512, 256), (80, 288, 1024, 512, 256), (40, 80, 1024, 384, 256), (40, 80, 1024, 512, 512)):
        ok = bool(lib.risvec_marl_critic_action_grad_supported(*dims))
        assert ok == bool(lib.risvec_marl_critic_supported(*dims)) == MC._supported(*dims), dims
        for n, k in ((1, 1), (33, 2), (256, 2), (4096, 1)):
            b = lib.risvec_marl_critic_action_grad_workspace(n, *dims, k)
            npad = (n + 31) // 32 * 32
            assert b == (4 * k * npad * (dims[1] + 1) if ok else 0), (dims, n, k)
    for n, k in ((0, 2), (-1, 2), (64, 0), (64, 3), (64, -1)):
        assert lib.risvec_marl_critic_action_grad_workspace(n, *DRIVER8, k) == 0
    # no activation is kept: far below the workspace of loss_backward at the same rows
    assert lib.risvec_marl_critic_action_grad_workspace(256, *DRIVER8, 2) * 20 < lib.risvec_marl_critic_grad_workspace(256, *DRIVER8, 2)


def test_action_grad_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf = (C.c_float * 256)()                                 # host memory: never dereferenced, only checked
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    dims = DRIVER8
    nbytes = lib.risvec_marl_critic_stream_bytes(*dims)
    n0 = 64
    need = lib.risvec_marl_critic_action_grad_workspace(n0, *dims, 2)
    fn = b"risvec_marl_critic_action_grad"

    def call(n=n0, dims=dims, n_nets=2, nets="make", wb=nbytes, bad_net=1, st=p, ac=p, scale=1.0, q1=p, q2=p + 16, q_min=p + 32,
             out=p + 64, ws=p, ws_bytes=need, W1=p, W2=p, W3=p, **kw):
        if nets == "make":
            arr = (N.RisVecMarlCriticActionGradNet * 2)()
            for c in range(2):
                arr[c] = N.RisVecMarlCriticActionGradNet(N.RisVecMarlCriticNet(p, nbytes, p, p, p, p, p, p), p, p, p)
            arr[bad_net].fwd.wstream_bytes = wb
            arr[bad_net].W1, arr[bad_net].W2, arr[bad_net].W3 = W1, W2, W3
            for k, v in kw.items():
                setattr(arr[bad_net].fwd, k, v)
            nets = C.cast(arr, C.c_void_p)
        if n_nets == 1 and q2 == p + 16:
            q2 = None
        return lib.risvec_marl_critic_action_grad(n, *dims, n_nets, nets, st, ac, scale, q1, q2, q_min, out, ws, ws_bytes, None)
    # every call below carries exactly one fault: a complete set of host pointers is never passed
    for n in (0, -3):
        assert call(n=n) == N.ERR_ARG and fn + b": n_rows" in lib.risvec_last_error()
    for k in (0, 3, -1):
        assert call(n_nets=k) == N.ERR_ARG and b"n_nets" in lib.risvec_last_error()
    for bad in ((40, 89, 1024, 512, 256), (40, 80, 1000, 512, 256), (40, 80, 1024, 384, 256), (40, 80, 1024, 512, 512),
                (0, 80, 1024, 512, 256), (80, 288, 1024, 512, 256)):
        assert call(dims=bad) == N.ERR_UNSUPPORTED and fn in lib.risvec_last_error()
    assert call(nets=None) == N.ERR_ARG and b"nets is NULL" in lib.risvec_last_error()
    for net in (0, 1):
        assert call(wb=nbytes - 1024, bad_net=net) == N.ERR_ARG and b"wstream_bytes" in lib.risvec_last_error()
        for f in ("wstream", "scales", "b1", "b2", "b3", "qw", "qb"):
            assert call(bad_net=net, **{f: None}) == N.ERR_ARG, f
            assert b"nets[%d].%s is NULL" % (net, f.encode()) in lib.risvec_last_error()
        for f in ("W1", "W2", "W3"):
            assert call(bad_net=net, **{f: None}) == N.ERR_ARG and b"nets[%d].%s is NULL" % (net, f.encode()) in lib.risvec_last_error()
    assert call(b2=p + 4) == N.ERR_ARG and b"16-byte aligned" in lib.risvec_last_error()
    assert call(W1=p + 2) == N.ERR_ARG and b"4-byte aligned" in lib.risvec_last_error()
    assert call(st=None) == N.ERR_ARG and call(ac=None) == N.ERR_ARG
    assert call(out=None) == N.ERR_ARG and b"out is NULL" in lib.risvec_last_error()
    assert call(ws=None) == N.ERR_ARG and b"workspace is NULL" in lib.risvec_last_error()
    assert call(out=p + 2) == N.ERR_ARG and call(q_min=p + 2) == N.ERR_ARG and call(q1=p + 2) == N.ERR_ARG
    assert call(scale=float("nan")) == N.ERR_ARG and call(scale=float("inf")) == N.ERR_ARG and b"scale" in lib.risvec_last_error()
    assert call(q2=p) == N.ERR_ARG and b"same buffer" in lib.risvec_last_error()
    assert call(n_nets=1, q2=p + 48) == N.ERR_ARG and b"q2" in lib.risvec_last_error()     # q2 without a second net
    assert call(ws=p + 4) == N.ERR_ARG
    assert call(ws_bytes=need - 1) == N.ERR_ARG and b"risvec_marl_critic_action_grad_workspace" in lib.risvec_last_error()
    assert call(n=n0 + 1) == N.ERR_ARG and b"workspace_bytes" in lib.risvec_last_error()    # one more tile needs more
    assert call(ws_bytes=0) == N.ERR_ARG


def test_python_surface_of_action_grad():
    T = MC.BatchedTwinCritic
    assert list(inspect.signature(T.action_grad).parameters) == ["self", "state", "action", "out", "q_min", "q", "scale", "workspace"]
    assert list(inspect.signature(T.action_grad_torch).parameters) == ["self", "state", "action", "out", "q_min", "q", "scale"]
    assert inspect.signature(T.action_grad).parameters["scale"].default == 1.0
    rng = T.ACTION_GRAD_AUTO_ROWS
    assert rng == () or (len(rng) == 2 and all(isinstance(v, int) for v in rng) and 1 <= rng[0] <= rng[1] <= 4096)
    import ris_vec_marl_amd
    assert not any("action_grad" in name for name in ris_vec_marl_amd.__all__)      # nothing new beyond what the class brings
    lib = N.load()

    def modes(dims, gemm):
        c = object.__new__(T)
        c._dims = dims
        c._init_modes(gemm, bool(lib.risvec_marl_critic_supported(*dims)), "a rule", bool(lib.risvec_marl_critic_wide_supported(*dims)))
        return c
    # an explicit gemm="fused" runs the device path at every row count; the library modes and other shapes never do
    c = modes(DRIVER8, "fused")
    assert c._action_grad_device(1) and c._action_grad_device(256) and c._action_grad_device(1 << 20)
    assert not modes(DRIVER8, "library")._action_grad_device(256) and not modes(DRIVER8, "wide")._action_grad_device(256)
    assert not modes((80, 288, 1024, 512, 256), None)._action_grad_device(256)
    c = modes(DRIVER8, None)
    for n in (1, 64, 256, 4096, 4097):
        assert c._action_grad_device(n) == (rng != () and rng[0] <= n <= rng[1])
