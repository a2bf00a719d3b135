"""CPU-side tests of the SAC twin critic (`BatchedTwinCritic`, `risvec_marl_critic`): the exported symbols, the shape rule,
the argument checks of the C entry point (which must answer before touching a device), the weight packing -- a pure
function that runs on CPU tensors -- the packed stream walked through the kernel's index maps in NumPy, and the float64
restatement the GPU tests measure against, checked here against the vectors captured from the reference's own network
and its own target statements."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

from ris_vec_marl_amd import _native as N
from ris_vec_marl_amd import marl_critic as MC
from tests import marl_critic_ref as R
from tests import mlp_sweep_shapes as SW

# (S, A, fc1, fc2, fc3): the driver's two, the fixtures' two, the corners of the rule, then the shapes of the GPU sweep
# (every instantiation and edge of the kernel; test_mlp_sweep_hip.py)
SHAPES = [(20, 24, 1024, 512, 256), (40, 80, 1024, 512, 256), (40, 80, 64, 128, 128), (20, 24, 64, 128, 128),
          (127, 1, 1024, 512, 256), (1, 127, 32, 128, 128), (1, 1, 32, 128, 256), (33, 46, 160, 256, 128)]
SHAPES += [d for d in SW.dims_of(SW.MARL_CRITIC) if d not in SHAPES]
SMALL = [s for s in SHAPES if s[2] <= 160]


def test_library_declares_and_exports_the_twin_critic():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "risvec.h")).read()
    lib = N.load()
    for name in ("risvec_marl_critic_supported", "risvec_marl_critic_stream_bytes", "risvec_marl_critic"):
        assert name in N.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, header)
    assert "RisVecMarlCriticNet" in header
    m = re.search(r"#define RISVEC_ABI_VERSION (\d+)", header)
    assert int(m.group(1)) == N.ABI_VERSION == 17             # new symbols only: the ABI version stays
    # the POD struct as the header lays it out: 8 fields of 8 bytes
    assert C.sizeof(N.RisVecMarlCriticNet) == 64
    assert [f for f, _ in N.RisVecMarlCriticNet._fields_] == ["wstream", "wstream_bytes", "scales", "b1", "b2", "b3", "qw", "qb"]


def test_supported_rule_agrees_with_the_library_over_a_grid():
    lib = N.load()
    grid = list(itertools.product((0, 1, 20, 40, 48, 80, 127, 128), (0, 1, 24, 80, 88, 127, 128, 288),
                                  (0, 32, 48, 96, 1024, 1056), (64, 128, 256, 384, 512, 1024), (64, 128, 192, 256, 512)))
    n_ok = 0
    for dims in grid:
        ok = bool(lib.risvec_marl_critic_supported(*dims))
        assert ok == MC._supported(*dims), dims
        assert (lib.risvec_marl_critic_stream_bytes(*dims) != 0) == ok, dims
        n_ok += ok
    pairs = sum(1 for s, a in itertools.product((1, 20, 40, 48, 80, 127, 128), (1, 24, 80, 88, 127, 128, 288)) if s + a <= 128)
    assert n_ok == pairs * 3 * 3 * 2
    for dims in SHAPES:
        assert lib.risvec_marl_critic_supported(*dims) == 1 and MC._supported(*dims)
    # the driver's sizes at 1024-512-256: 4 and 8 vehicles are built, 16 vehicles (80, 288) take the library path
    assert lib.risvec_marl_critic_supported(20, 24, 1024, 512, 256) == 1
    assert lib.risvec_marl_critic_supported(40, 80, 1024, 512, 256) == 1
    assert lib.risvec_marl_critic_supported(80, 288, 1024, 512, 256) == 0 and not MC._supported(80, 288, 1024, 512, 256)
    # each edge of the rule
    for dims, ok in (((48, 80, 1024, 512, 256), 1), ((49, 80, 1024, 512, 256), 0), ((40, 80, 1024 + 32, 512, 256), 0),
                     ((40, 80, 1000, 512, 256), 0), ((40, 80, 32, 512, 256), 1), ((40, 80, 1024, 64, 256), 0),
                     ((40, 80, 1024, 128, 128), 1), ((40, 80, 1024, 512, 512), 0), ((0, 80, 1024, 512, 256), 0),
                     ((40, 0, 1024, 512, 256), 0)):
        assert lib.risvec_marl_critic_supported(*dims) == ok == int(MC._supported(*dims)), dims


def torch_weights(dims, seed, scale=1.0):
    w = R.random_net(dims, seed)
    t = lambda k: torch.from_numpy(w[k])                      # noqa: E731
    return w, dict(W1=t("fc1.weight") * scale, W2=t("fc2.weight"), W3=t("fc3.weight"))


@pytest.mark.parametrize("dims", SHAPES)
@pytest.mark.parametrize("scale", [1.0, 1e-3])
def test_packing_round_trip_and_stream_size(dims, scale):
    """hi + lo with the recorded scale reproduce every float32 weight to 2^-21 of the matrix's largest entry (the split
    keeps 22 bits below the largest entry's exponent); the stream has the byte size the library states."""
    _, tw = torch_weights(dims, 3, scale)
    stream, scales = MC.pack_marl_critic_weights(**tw)
    g = MC.marl_critic_geom(*dims)
    S, A, F1, F2, F3 = dims
    assert g.rows == g.ng * g.ks * 2 + 4 * 2 * g.ng * g.mt2 * 2 + 4 * (F2 // 16) * g.mt3 * 2
    assert (g.ks, g.ng, g.mt2, g.mt3) == (-(-(S + A) // 16), F1 // 32, F2 // 128, F3 // 128)
    assert stream.dtype == torch.float16 and tuple(stream.shape) == (g.rows, 64, 8) and stream.is_contiguous()
    assert stream.numel() * 2 == N.load().risvec_marl_critic_stream_bytes(*dims) == g.rows * 1024
    # the kernel's LDS: input fragments + the widest activation + the reduction slots, within the 160 KiB of a CU
    assert (g.ks + max(2 * g.ng, F2 // 16)) * 2048 + 2 * 4 * 32 * 4 <= 160 * 1024
    assert tuple(scales.shape) == (3,) and scales.dtype == torch.float32
    assert all(float(torch.log2(s)) == round(float(torch.log2(s))) for s in scales)       # powers of two
    un = MC._unpack(stream, scales, *dims)
    want = {"fc1": tw["W1"].double().T, "fc2": tw["W2"].double().T, "fc3": tw["W3"].double().T}
    assert set(un) == set(want)
    for k in want:
        assert un[k].shape == want[k].shape, k
        assert float((un[k] - want[k]).abs().max()) <= 2.0 ** -21 * float(want[k].abs().max()), k


def test_packing_refuses_unsupported_shapes():
    _, tw = torch_weights((40, 80, 64, 128, 128), 1)
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights(**dict(tw, W2=torch.zeros(64, 64), W3=torch.zeros(128, 64)))      # fc2 = 64
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights(**dict(tw, W3=torch.zeros(128, 256)))                             # does not chain
    with pytest.raises(ValueError):
        MC.pack_marl_critic_weights(torch.zeros(1024, 80 + 288), torch.zeros(512, 1024), torch.zeros(256, 512))


def test_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf = (C.c_float * 64)()                                  # host memory: never dereferenced, only checked
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    dims = (40, 80, 1024, 512, 256)
    nbytes = lib.risvec_marl_critic_stream_bytes(*dims)
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
        return lib.risvec_marl_critic(n, *dims, n_nets, nets, st, ac, rw, dn, gamma, coef, lp, li, q1, q2, y, None)
    # every call below carries exactly one fault: a complete set of host pointers is never passed
    for n in (0, -3):
        assert call(n=n) == N.ERR_ARG and b"risvec_marl_critic" in lib.risvec_last_error()
    for k in (0, 3, -1):
        assert call(n_nets=k) == N.ERR_ARG and b"n_nets" in lib.risvec_last_error()
    for bad in ((80, 288, 1024, 512, 256), (49, 80, 1024, 512, 256), (40, 80, 1000, 512, 256), (40, 80, 1024, 384, 256),
                (40, 80, 1024, 512, 512), (0, 80, 1024, 512, 256)):
        assert call(dims=bad) == N.ERR_UNSUPPORTED
        assert b"risvec_marl_critic" in lib.risvec_last_error()
    assert call(nets=None) == N.ERR_ARG
    for net in (0, 1):
        assert call(wb=nbytes - 1024, bad_net=net) == N.ERR_ARG           # a stream packed for another shape
        assert b"wstream_bytes" in lib.risvec_last_error()
        for f in fields:
            assert call(bad_net=net, **{f: None}) == N.ERR_ARG, f
    assert call(b2=p + 4) == N.ERR_ARG                        # not 16-byte aligned
    assert call(st=None) == N.ERR_ARG and call(ac=None) == N.ERR_ARG
    assert call(q1=None, q2=None, y=None, lp=None, li=None) == N.ERR_ARG      # at least one output
    assert call(n_nets=1) == N.ERR_ARG and b"q2" in lib.risvec_last_error()   # q2 without a second net
    assert call(rw=None) == N.ERR_ARG and call(dn=None) == N.ERR_ARG          # y needs reward and done
    assert call(coef=None) == N.ERR_ARG and b"coef" in lib.risvec_last_error()
    assert call(coef=None, lp=None) == N.ERR_ARG and call(coef=None, li=None) == N.ERR_ARG
    assert call(y=None) == N.ERR_ARG                          # the entropy inputs without y
    for g in (float("nan"), float("inf"), -float("inf")):
        assert call(gamma=g) == N.ERR_ARG and b"gamma" in lib.risvec_last_error()


@pytest.mark.parametrize("name", R.FIXTURES)
def test_float64_restatement_is_the_references_network(name):
    """q1, q2 and both targets of the fixtures (the reference's own float32 forward and its own target statements) against
    the float64 restatement: err < 2e-5, done rows equal the reward bit for bit."""
    fx = R.fixture(name)
    done = fx["done"]
    q64 = [R.critic_q64(R.weights_of(fx, c), fx["state_"], fx["action_"]) for c in (1, 2)]
    for c in (1, 2):
        assert set(R.weights_of(fx, c)) == set(R.KEYS) == set(MC.BatchedTwinCritic._SD)
    e = {"q1": R.err(fx["q1"], q64[0]), "q2": R.err(fx["q2"], q64[1])}
    for branch in ("single", "separate"):
        y64 = R.td_target64(fx["reward"], q64[0], q64[1], done, float(fx["gamma"]), fx["coef_" + branch], fx["logp_power"],
                            fx["logp_intent"])
        e["target_" + branch] = R.err(fx["target_" + branch], y64)
        assert np.array_equal(fx["target_" + branch].reshape(-1)[done], fx["reward"][done])
    print("%s: the reference's float32 against float64: %s" % (name, ", ".join("%s %.3g" % kv for kv in e.items())))
    assert all(v < R.BAR for v in e.values())
    assert fx["coef_single"][0] == fx["coef_single"][1] and fx["coef_separate"][0] != fx["coef_separate"][1]
    assert not np.array_equal(fx["target_single"], fx["target_separate"])


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixture_is_shaped_as_the_learners_batch(name):
    fx = R.fixture(name)
    V, S, A, B = (int(fx[k]) for k in ("V", "S", "A", "B"))
    assert (S, A) == (5 * V, V * (V + 2)) and fx["state_"].shape == (B, S) and fx["action_"].shape == (B, A)
    assert (int(fx["fc1"]), int(fx["fc2"]), int(fx["fc3"])) == (64, 128, 128)
    assert (name, V, B) in (("marl_critic_8", 8, 70), ("marl_critic_4", 4, 33))
    first = float((fx["q1"] < fx["q2"]).mean())
    second = float((fx["q2"] < fx["q1"]).mean())
    assert 0.4 <= first <= 0.6 and 0.4 <= second <= 0.6, (first, second)     # min() has both outcomes
    assert fx["done"].dtype == np.bool_ and abs(int(fx["done"].sum()) - B / 4) < 1
    act = fx["action_"].reshape(B, V, V + 2)
    assert np.array_equal(np.sort(act[:, :, :V], -1)[:, :, -2:], np.broadcast_to([0.0, 1.0], (B, V, 2)))   # one-hot
    assert act[:, :, V:].min() > 0 and act[:, :, V:].max() < 1
    assert float(np.abs(fx["q1"]).max()) > 0.3 and float(np.abs(fx["q2"]).max()) > 0.3
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert sum(os.path.getsize(os.path.join(root, n + ".npz")) for n in R.FIXTURES) < 482471    # the largest committed fixture


@pytest.mark.parametrize("dims", SMALL)
def test_numpy_walk_of_the_packed_stream(dims):
    """The packed stream walked through the kernel's data flow in NumPy (the input staged from two pointers, fragment
    addressing, the C/D -> B hand-over through LDS, the four-way feature split, split activations, three partial
    products) against float64.  What is left is the split's rounding: 2^-22 per product, far inside the bar."""
    w, tw = torch_weights(dims, 11)
    stream, scales = MC.pack_marl_critic_weights(**tw)
    state, action = R.random_batch(dims, 37, 12)
    got = R.walk_stream(stream.numpy(), scales.numpy(), w, state, action, dims, MC.marl_critic_geom(*dims))
    e = R.err(got, R.critic_q64(w, state, action))
    print("walk %s: err %.3g" % (dims, e))
    assert e < 1e-6


@pytest.mark.parametrize("name", R.FIXTURES)
def test_numpy_walk_reproduces_the_fixtures(name):
    fx = R.fixture(name)
    dims = tuple(int(fx[k]) for k in ("S", "A", "fc1", "fc2", "fc3"))
    for c in (1, 2):
        w = R.weights_of(fx, c)
        stream, scales = MC.pack_marl_critic_weights(*(torch.from_numpy(w[k + ".weight"]) for k in ("fc1", "fc2", "fc3")))
        got = R.walk_stream(stream.numpy(), scales.numpy(), w, fx["state_"], fx["action_"], dims, MC.marl_critic_geom(*dims))
        e = R.err(got, R.critic_q64(w, fx["state_"], fx["action_"]))
        print("walk %s net %d: err %.3g" % (name, c, e))
        assert e < 1e-6


def test_twin_critic_is_exported_and_needs_a_device():
    import inspect

    import ris_vec_marl_amd as rv
    for name in ("BatchedTwinCritic", "pack_marl_critic_weights"):
        assert getattr(rv, name) is getattr(MC, name) and name in rv.__all__
    assert set(MC.BatchedTwinCritic._SD) == {p + s for p in ("fc1.", "fc2.", "fc3.", "q.") for s in ("weight", "bias")}
    assert list(inspect.signature(MC.BatchedTwinCritic.__init__).parameters) == [
        "self", "state_dims", "action_dims", "fc1_dims", "fc2_dims", "fc3_dims", "n_nets", "device", "seed", "gemm"]
    assert list(inspect.signature(MC.BatchedTwinCritic.td_target).parameters) == [
        "self", "reward", "state_", "action_", "done", "gamma", "logp_power", "logp_intent", "coef", "out", "q"]
    assert MC.BatchedTwinCritic.AUTO_MIN_ROWS >= 1
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            rv.BatchedTwinCritic(40, 80, device="cpu")
    with pytest.raises(RuntimeError):
        rv.BatchedTwinCritic(40, 80, device=torch.device("cpu"))
