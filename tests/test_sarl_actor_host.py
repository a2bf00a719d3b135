"""CPU-side tests of the DDPG actor forward (`BatchedActor`, `risvec_sarl_actor`): the shape rule, the argument
checks of the C entry point (which must answer before touching a device), and the weight packing -- a pure function
that runs on CPU tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

from ris_vec_marl_amd import _native as N
from ris_vec_marl_amd import actor as ACT
from tests import mlp_sweep_shapes as SW

# then the shapes of the GPU sweep (every instantiation and edge of the kernel; test_mlp_sweep_hip.py)
SHAPES = [(80, 512, 256, 56), (104, 512, 256, 80), (36, 64, 128, 24), (128, 1024, 256, 96), (5, 32, 128, 1), (79, 96, 128, 33)]
SHAPES += [d for d in SW.dims_of(SW.SARL_ACTOR) if d not in SHAPES]


@pytest.mark.parametrize("dims,ok", [((80, 512, 256, 56), 1), ((104, 512, 256, 80), 1), ((36, 64, 128, 24), 1),
                                     ((128, 1024, 256, 96), 1), ((144, 512, 256, 56), 0), ((80, 500, 256, 56), 0),
                                     ((80, 512, 64, 56), 0), ((80, 512, 256, 288), 0), ((0, 512, 256, 56), 0),
                                     ((80, 1056, 256, 56), 0), ((80, 512, 256, 97), 0), ((129, 512, 256, 56), 0)])
def test_supported_truth_table(dims, ok):
    assert N.load().risvec_sarl_actor_supported(*dims) == ok
    assert ACT._supported(*dims) == bool(ok)


def test_abi_version_is_unchanged():
    assert N.load().risvec_abi_version() == 17 == N.ABI_VERSION


def test_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf = (C.c_float * 64)()                                  # host memory: never dereferenced, only checked
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    g = ACT.actor_geom(80, 512, 256, 56)
    nbytes = g.items * g.rows * 1024

    def call(n=4, dims=(80, 512, 256, 56), x=p, ws=p, wb=nbytes, sc=p, b2=p, lw=p, lb=p, bm=p, lg=None, mu=p):
        return lib.risvec_sarl_actor(n, *dims, x, ws, wb, sc, b2, lw, lb, bm, lg, mu, None)
    assert call(n=0) == N.ERR_SHAPE
    for dims in ((144, 512, 256, 56), (80, 500, 256, 56), (80, 512, 64, 56), (80, 512, 256, 288)):
        assert call(dims=dims) == N.ERR_SHAPE
        assert b"risvec_sarl_actor" in lib.risvec_last_error()
    assert call(wb=nbytes - 1024) == N.ERR_ARG                # a stream packed for another shape
    for name in ("x", "ws", "sc", "b2", "lw", "lb", "bm", "mu"):
        assert call(**{name: None}) == N.ERR_ARG, name
    assert call(mu=p + 4) == N.ERR_ARG and call(lg=p + 4) == N.ERR_ARG      # not 16-byte aligned


def random_weights(dims, seed, scale=1.0):
    IN, F1, F2, A = dims
    g = torch.Generator().manual_seed(seed)
    u = lambda *s, r: (torch.rand(*s, generator=g) * 2 - 1) * r     # noqa: E731
    return dict(W1=u(F1, IN, r=scale / F1 ** 0.5), b1=u(F1, r=scale / F1 ** 0.5), ln1_w=0.5 + torch.rand(F1, generator=g),
                ln1_b=u(F1, r=0.2), W2=u(F2, F1, r=1 / F2 ** 0.5), Wmu=u(A, F2, r=0.18))


@pytest.mark.parametrize("dims", SHAPES)
@pytest.mark.parametrize("scale", [1.0, 1e-3])
def test_packing_round_trip(dims, scale):
    """hi + lo with the recorded scale reproduce every float32 weight to 2^-21 of the matrix's largest entry (the split
    keeps 22 bits below the largest entry's exponent), in both copies of the fc1 weight; the LayerNorm-1 rows are exact."""
    IN, F1, F2, A = dims
    w = random_weights(dims, 3, scale)
    stream, scales = ACT.pack_actor_weights(**w)
    g = ACT.actor_geom(*dims)
    assert stream.dtype == torch.float16 and tuple(stream.shape) == (g.items, g.rows, 64, 8) and stream.is_contiguous()
    assert g.rows % 4 == 0 and 3 * g.rows * 1024 <= 160 * 1024          # three ring slots fit the LDS
    assert tuple(scales.shape) == (3,) and scales.dtype == torch.float32
    assert all(float(torch.log2(s)) == round(float(torch.log2(s))) for s in scales)       # powers of two
    un = ACT.unpack_actor_weights(stream, scales, *dims)
    c = ACT.centre_fc1(w["W1"], w["b1"])
    for got, want in ((un["fc1"], c), (un["fc1_pass1"], c), (un["fc2"], w["W2"].double().T), (un["mu"], w["Wmu"].double().T)):
        assert got.shape == want.shape
        assert float((got - want).abs().max()) <= 2.0 ** -21 * float(want.abs().max())
    assert torch.equal(un["fc1"], un["fc1_pass1"])
    assert torch.equal(un["ln1_w"].float(), w["ln1_w"]) and torch.equal(un["ln1_b"].float(), w["ln1_b"])


@pytest.mark.parametrize("dims", SHAPES)
def test_centred_fc1_rows_sum_to_zero(dims):
    w = random_weights(dims, 5)
    c = ACT.centre_fc1(w["W1"], w["b1"])
    assert c.dtype == torch.float64 and tuple(c.shape) == (dims[0] + 1, dims[1])
    # float64 rounding of F1 terms of size <= max|c|
    assert float(c.sum(-1).abs().max()) <= dims[1] * 2.0 ** -52 * float(c.abs().max())
    # what the kernel multiplies by: the split's rounding, at most 2^-22 of the largest entry per term
    stream, scales = ACT.pack_actor_weights(**w)
    un = ACT.unpack_actor_weights(stream, scales, *dims)
    assert float(un["fc1"].sum(-1).abs().max()) <= dims[1] * 2.0 ** -22 * float(c.abs().max())


def test_packing_refuses_unsupported_shapes():
    w = random_weights((80, 512, 256, 56), 1)
    w["W2"] = torch.zeros(64, 512)
    w["Wmu"] = torch.zeros(56, 64)
    with pytest.raises(ValueError):
        ACT.pack_actor_weights(**w)


def test_batched_actor_is_exported_and_needs_a_device():
    import ris_vec_marl_amd as rv
    assert rv.BatchedActor is ACT.BatchedActor and "BatchedActor" in rv.__all__
    assert set(ACT.BatchedActor._SD) == {p + s for p in ("fc1.", "fc2.", "bn1.", "bn2.", "mu.") for s in ("weight", "bias")}
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            rv.BatchedActor(80, 56, device="cpu")


def test_load_state_dict_rejects_a_wrong_shape():
    """Built without a device: the checks of load_state_dict come before any copy."""
    a = ACT.BatchedActor.__new__(ACT.BatchedActor)
    a.device = torch.device("cpu")
    dims = dict(W1=(96, 80), b1=(96,), ln1_w=(96,), ln1_b=(96,), W2=(128, 96), b2=(128,), ln2_w=(128,), ln2_b=(128,),
                Wmu=(56, 128), bmu=(56,))
    for k, s in dims.items():
        setattr(a, k, torch.zeros(*s))
    sd = {k: np.ones(dims[v], np.float32) for k, v in ACT.BatchedActor._SD.items()}
    a.load_state_dict(sd)
    assert float(a.W2.sum()) == 128 * 96 and float(a.bmu.sum()) == 56
    bad = dict(sd)
    bad["fc2.weight"] = np.ones((96, 128), np.float32)        # [in, out] instead of the reference's [out, in]
    with pytest.raises(ValueError):
        a.load_state_dict(bad)
    del bad["fc2.weight"]
    with pytest.raises(KeyError):
        a.load_state_dict(bad)
    assert set(a.state_dict()) == set(sd)
