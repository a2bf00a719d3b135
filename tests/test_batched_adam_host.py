"""CPU-side tests of `BatchedAdam` (ris_vec_marl_amd/optim.py) and `risvec_adam_step`: the symbols, every argument error of
the C entry point (answered before a device is touched), the Python refusals (each changes nothing), and the error bars
of tests/optim_ref.py -- PyTorch's own float32 `clip_grad_norm_` + `Adam` must stay inside them (so they are not tighter
than float32 permits), `step_torch` on CPU tensors must, and `from_torch` -> steps -> `to_torch` must continue a PyTorch
optimiser's trajectory inside them.

Observed |error| / bar, largest over all cases and steps (this file prints them): PyTorch CPU m 0.23, v 0.47, param 0.99;
its norm within 2.3 u (float32 accumulation; our kernel's float64 accumulation is held to 4 u in test_batched_adam_hip.py)."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import ris_vec_marl_amd as rv
from ris_vec_marl_amd import _native as N
from ris_vec_marl_amd import optim as OPT
from tests import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = N.ADAM_CHUNK


# ---------------------------------------------------------------------- symbols and the C argument checks
def test_symbols_are_exported_and_declared_and_the_abi_stays_17():
    lib = N.load()
    header = open(os.path.join(ROOT, "include", "risvec.h")).read()
    for name in ("risvec_adam_step", "risvec_adam_workspace"):
        assert name in N.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert lib.risvec_abi_version() == 17 == N.ABI_VERSION
    assert "#define RISVEC_ABI_VERSION 17" in header
    assert "#define RISVEC_ADAM_CHUNK %d" % CH in header
    assert C.sizeof(N.RisVecAdamTensor) == 64 and C.sizeof(N.RisVecAdamGroup) == 32
    assert rv.BatchedAdam is OPT.BatchedAdam and "BatchedAdam" in rv.__all__
    assert lib.risvec_adam_workspace(5) == 40 and lib.risvec_adam_workspace(0) == 0 and lib.risvec_adam_workspace(-3) == 0
    assert "no gradient" in OPT.BatchedAdam.step.__doc__ or "without a gradient" in OPT.BatchedAdam.step.__doc__


def _call(lib, p, numels=(3, CH + 1, 7), groups=(0, 0, 1), **kw):
    """risvec_adam_step over host memory that is only checked, never dereferenced on a device: a valid call unless `kw`
    breaks it.  kw: any scalar argument by name, `tens` / `grp`: a function that edits the host tables, `null`: the
    pointer arguments to pass as NULL, `off`: {pointer argument: byte offset}."""
    n, ng = len(numels), max(groups) + 1
    tens, grp = (N.RisVecAdamTensor * n)(), (N.RisVecAdamGroup * ng)()
    first = 0
    for i, (ne, g) in enumerate(zip(numels, groups)):
        base = p + 4096 * i
        tens[i] = N.RisVecAdamTensor(base, base + 512, base + 1024, base + 1536, base + 2048, ne, g, first, 0)
        first += (ne + CH - 1) // CH
    for g in range(ng):
        mine = [i for i in range(n) if groups[i] == g]
        grp[g] = N.RisVecAdamGroup(1e-3, 0.0, 1.0, tens[mine[0]].first_block,
                                   sum((numels[i] + CH - 1) // CH for i in mine), 0)
    kw.get("tens", lambda t: None)(tens)
    kw.get("grp", lambda t: None)(grp)
    a = dict(n_tensors=n, n_groups=ng, n_blocks=first, tensors=p + 65536, groups=p + 65536 + 1024, block_tensor=p + 65536 + 2048,
             tensors_host=C.cast(tens, C.c_void_p), groups_host=C.cast(grp, C.c_void_p), beta1=0.9, beta2=0.999, eps=1e-8, t=1,
             tau=0.005, omt=0.995, flags=N.ADAM_CLIP | N.ADAM_BLEND, partials=p + 65536 + 4096, partials_bytes=8 * first,
             norms=p + 65536 + 8192)
    a.update({k: v for k, v in kw.items() if k in a})
    for k in kw.get("null", ()):
        a[k] = None
    for k, o in kw.get("off", {}).items():
        a[k] += o
    return lib.risvec_adam_step(*a.values(), None)


def test_entry_point_rejects_bad_arguments_without_a_device():
    lib = N.load()
    buf = (C.c_char * (1 << 17))()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16

    def bad(code, word, **kw):
        assert _call(lib, p, **kw) == code, kw
        msg = lib.risvec_last_error()
        assert b"risvec_adam_step" in msg and word in msg, (kw, msg)
    bad(N.ERR_SHAPE, b"n_tensors", n_tensors=0)
    bad(N.ERR_SHAPE, b"n_tensors", n_tensors=(1 << 20) + 1)
    bad(N.ERR_SHAPE, b"n_groups", n_groups=0)
    bad(N.ERR_SHAPE, b"n_groups", n_groups=4)
    bad(N.ERR_SHAPE, b"n_blocks", n_blocks=2)
    bad(N.ERR_SHAPE, b"n_blocks", n_blocks=5)
    for name in ("tensors", "groups", "block_tensor", "tensors_host", "groups_host", "partials", "norms"):
        bad(N.ERR_ARG, name.encode() + b" is NULL", null=(name,))
    for name in ("tensors", "groups", "block_tensor", "partials"):
        bad(N.ERR_ARG, name.encode() + b" is not 16-byte aligned", off={name: 8})
    bad(N.ERR_ARG, b"norms is not 4-byte aligned", off={"norms": 2})
    bad(N.ERR_ARG, b"flags", flags=8)
    for b in (-0.1, 1.0, 1.5, float("nan")):
        bad(N.ERR_ARG, b"beta1", beta1=b)
        bad(N.ERR_ARG, b"beta2", beta2=b)
    for e in (float("nan"), float("inf"), -1e-8):
        bad(N.ERR_ARG, b"eps", eps=e)
    bad(N.ERR_ARG, b"t=0", t=0)
    bad(N.ERR_ARG, b"t=-3", t=-3)
    for x in (float("nan"), float("inf")):
        bad(N.ERR_ARG, b"tau", tau=x)
        bad(N.ERR_ARG, b"tau", omt=x)
        bad(N.ERR_ARG, b"lr", grp=lambda g, x=x: setattr(g[1], "lr", x))
        bad(N.ERR_ARG, b"weight_decay", grp=lambda g, x=x: setattr(g[0], "weight_decay", x))
    bad(N.ERR_ARG, b"lr", grp=lambda g: setattr(g[0], "lr", -1e-3))
    bad(N.ERR_ARG, b"weight_decay", grp=lambda g: setattr(g[0], "weight_decay", -0.01))
    bad(N.ERR_ARG, b"max_norm", grp=lambda g: setattr(g[0], "max_norm", float("nan")))
    bad(N.ERR_ARG, b"groups[1].first_block", grp=lambda g: setattr(g[1], "first_block", 2))
    bad(N.ERR_ARG, b"groups[0].n_blocks", grp=lambda g: setattr(g[0], "n_blocks", 2))
    bad(N.ERR_SHAPE, b"numel", tens=lambda t: setattr(t[0], "numel", 0))
    bad(N.ERR_ARG, b"tensors[1].first_block", tens=lambda t: setattr(t[1], "first_block", 0))
    bad(N.ERR_ARG, b"tensors[1].group", tens=lambda t: setattr(t[1], "group", 2))
    bad(N.ERR_ARG, b"tensors[0].group", tens=lambda t: setattr(t[0], "group", 1))
    bad(N.ERR_ARG, b"1 groups have tensors", tens=lambda t: setattr(t[2], "group", 0))   # group 1 is left empty
    for name in ("param", "grad", "exp_avg", "exp_avg_sq"):
        bad(N.ERR_ARG, b"tensors[1].%s is NULL" % name.encode(), tens=lambda t, name=name: setattr(t[1], name, None))
        bad(N.ERR_ARG, b"tensors[2].%s is not 4-byte aligned" % name.encode(),
            tens=lambda t, name=name: setattr(t[2], name, getattr(t[2], name) + 2))
    bad(N.ERR_ARG, b"same tensor", tens=lambda t: setattr(t[0], "target", t[0].param))
    bad(N.ERR_ARG, b"same tensor", tens=lambda t: setattr(t[0], "exp_avg_sq", t[0].exp_avg))
    bad(N.ERR_ARG, b"partials_bytes", partials_bytes=8)
    # a NULL target is allowed: the call gets as far as the last check
    bad(N.ERR_ARG, b"partials_bytes", partials_bytes=8, tens=lambda t: setattr(t[0], "target", None))


# ---------------------------------------------------------------------- the Python refusals
def _nets(n_groups=2, seed=0, sizes=((5, 3), (5,), (7,))):
    g = torch.Generator().manual_seed(seed)
    groups = [[torch.randn(*s, generator=g).requires_grad_() for s in sizes] for _ in range(n_groups)]
    for grp in groups:
        for p in grp:
            p.grad = torch.randn(p.shape, generator=g)
    return groups


def _snapshot(opt, extra=()):
    return [t.detach().clone() for t in opt._params + opt.exp_avg + opt.exp_avg_sq + list(extra)], opt.t


def _unchanged(opt, snap, extra=()):
    ts, t = snap
    return opt.t == t and all(torch.equal(a.detach(), b) for a, b in zip(opt._params + opt.exp_avg + opt.exp_avg_sq + list(extra), ts))


def test_constructor_refusals():
    groups = _nets()
    for bad in ([[groups[0][0].detach().double()]], [[torch.ones(4, 4).t()]], [[torch.zeros(0)]], [[1.0]], [], [[]], 3,
                [groups[0], [groups[0][1]]], [[groups[0][0], groups[0][0]]]):
        with pytest.raises(ValueError):
            OPT.BatchedAdam(bad)
    view = torch.zeros(8)
    with pytest.raises(ValueError, match="twice"):
        OPT.BatchedAdam([[view[:4]], [view[:4]]])
    for kw in (dict(lr=float("nan")), dict(lr=-1.0), dict(lr=[1e-3]), dict(lr=torch.tensor(1e-3)), dict(betas=(1.0, 0.999)),
               dict(betas=(0.9, -0.1)), dict(betas=(0.9,)), dict(eps=float("inf")), dict(eps=-1.0), dict(weight_decay=-0.1),
               dict(weight_decay=float("nan")), dict(max_norm=-1.0), dict(max_norm=float("inf")), dict(max_norm=[1.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            OPT.BatchedAdam(groups, **kw)
    opt = OPT.BatchedAdam(groups, lr=[1e-3, 3e-4], max_norm=[1.0, None], weight_decay=0.01)
    assert opt.lr == [1e-3, 3e-4] and opt.max_norm == [1.0, None] and opt.weight_decay == [0.01, 0.01]
    assert all(m.data_ptr() % 16 == p.data_ptr() % 16 for m, p in zip(opt.exp_avg + opt.exp_avg_sq, opt._params * 2))
    assert all(float(m.abs().max()) == 0 for m in opt.exp_avg + opt.exp_avg_sq)


@pytest.mark.parametrize("method", ["step", "step_torch"])
def test_step_refusals_change_nothing(method):
    groups = _nets()
    opt = OPT.BatchedAdam(groups)
    targets = [[torch.zeros_like(p) for p in g] for g in groups]
    flat_t = [t for g in targets for t in g]
    snap = _snapshot(opt, flat_t)
    run = getattr(opt, method)

    def refused(**kw):
        with pytest.raises(ValueError):
            run(**kw)
        assert _unchanged(opt, snap, flat_t)
    keep = groups[1][2].grad
    groups[1][2].grad = None
    refused()                                                 # a missing gradient
    groups[1][2].grad = keep

    def with_last(x):
        return [[p.grad for p in groups[0]], [groups[1][0].grad, groups[1][1].grad, x]]
    refused(grads=with_last(None))
    refused(grads=with_last(keep.double()))                   # dtype
    refused(grads=with_last(torch.zeros(7, 2)[:, 0]))         # not contiguous
    refused(grads=with_last(torch.zeros(8)))                  # shape
    refused(grads=[[p.grad for p in groups[0]]])              # grads of one group only
    refused(grads=[[p.grad for p in g][:2] for g in groups])
    refused(targets=targets)                                  # no tau
    refused(tau=0.005)                                        # no targets
    refused(targets=targets, tau=1.5)
    refused(targets=targets, tau=float("nan"))
    refused(targets=targets[:1], tau=0.005)                   # mismatched
    refused(targets=[targets[0], targets[1][:2]], tau=0.005)
    refused(targets=[targets[0], [targets[1][0], targets[1][1], torch.zeros(8)]], tau=0.005)
    refused(targets=[targets[0], [targets[1][0], targets[1][1], targets[1][2].double()]], tau=0.005)
    refused(targets=[targets[0], [targets[1][0], targets[1][1], groups[1][2]]], tau=0.005)      # its own target
    refused(targets=[targets[0], [targets[1][0], targets[1][1], groups[0][2]]], tau=0.005)      # another parameter
    if method == "step" and not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):  # valid arguments: only the device is missing
            opt.step(targets=targets, tau=0.005)
        assert _unchanged(opt, snap, flat_t)


def test_from_torch_refusals():
    def params():
        return [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(4))]
    A = torch.optim.Adam
    for make in (lambda: [A(params(), amsgrad=True)], lambda: [A(params(), maximize=True)],
                 lambda: [torch.optim.AdamW(params())], lambda: [A(params(), decoupled_weight_decay=True)],
                 lambda: [A(params(), lr=torch.tensor(1e-3))], lambda: [torch.optim.SGD(params(), lr=0.1)],
                 lambda: [A(params(), differentiable=True)], lambda: [],
                 lambda: [A([{"params": params()[:1], "lr": 1e-3}, {"params": params()[1:], "lr": 1e-4}])],
                 lambda: [A(params()), A(params(), betas=(0.8, 0.999))], lambda: [A(params()), A(params(), eps=1e-6)]):
        with pytest.raises(ValueError):
            OPT.BatchedAdam.from_torch(make())
    ps, qs = params(), params()
    a, b = A(ps), A(qs)
    for p in ps:
        p.grad = torch.ones_like(p)
    a.step()                                                  # a has stepped once, b never
    with pytest.raises(ValueError, match="step counts differ"):
        OPT.BatchedAdam.from_torch([a, b])
    opt = OPT.BatchedAdam.from_torch([a], max_norm=None)
    assert opt.t == 1 and opt.max_norm == [None] and torch.equal(opt.exp_avg[0], a.state[ps[0]]["exp_avg"])
    with pytest.raises(ValueError):
        opt.to_torch([b])                                     # other parameters
    with pytest.raises(ValueError):
        opt.to_torch([a, b])


# ---------------------------------------------------------------------- the bars
def _case(seed, t0, weight_decay, mag):
    """Two groups of three tensors, gradients of magnitude `mag` (a float, or "mixed": 1e-12 .. 1e3 element by element),
    moments as after t0 steps."""
    g = torch.Generator().manual_seed(seed)
    sizes = ((33, 7), (129,), (1,))
    groups = [[torch.randn(*s, generator=g).requires_grad_() for s in sizes] for _ in range(2)]

    def draw(shape):
        x = torch.randn(shape, generator=g)
        if mag == "mixed":
            return x * 10.0 ** (torch.rand(shape, generator=g) * 15 - 12)
        return x * mag
    grads = [[[draw(p.shape) for p in grp] for grp in groups] for _ in range(3)]
    m0 = [[draw(p.shape) * 0.5 if t0 else torch.zeros_like(p) for p in grp] for grp in groups]
    v0 = [[draw(p.shape) ** 2 * 0.5 if t0 else torch.zeros_like(p) for p in grp] for grp in groups]
    return groups, grads, m0, v0, dict(lr=[1e-3, 3e-4], weight_decay=weight_decay, max_norm=1.0), t0


CASES = [(0, 0, 0.0, 1.0), (1, 0, 0.01, 1e-3), (2, 1, 0.0, "mixed"), (3, 999, 0.01, "mixed"), (4, 999, 0.0, 1e3), (5, 0, 0.0, 1e-12)]
RATIOS = {}


def _judge(tag, before, after, grads, coefs, hyper, t, betas=(0.9, 0.999), eps=1e-8):
    """after vs the float64 restatement from `before` (lists per group of (p, m, v)), one coefficient per group."""
    worst = RATIOS.setdefault(tag, {"m": 0.0, "v": 0.0, "p": 0.0})
    for gi, (b, a, gs) in enumerate(zip(before, after, grads)):
        for (p, m, v), (p1, m1, v1), g in zip(b, a, gs):
            ref = R.adam_ref(p, g, m, v, coefs[gi], hyper["lr"][gi], betas, eps, hyper["weight_decay"], t)
            for k, got in (("m", m1), ("v", v1), ("p", p1)):
                worst[k] = max(worst[k], R.worst_ratio(got, ref[k], ref[k + "_bar"]))
    return worst


def _state(opt_like):
    return [[tuple(x.detach().clone() for x in pmv) for pmv in grp] for grp in opt_like]


@pytest.mark.parametrize("case", CASES)
def test_pytorch_cpu_float32_stays_inside_the_bars(case):
    """`torch.optim.Adam` + `clip_grad_norm_` on the CPU, fed the test's inputs step by step, rebased on its own float32
    state before every step, the coefficient from its own float32 norm."""
    groups, grads, m0, v0, hyper, t0 = _case(*case)
    opts = [torch.optim.Adam(grp, lr=hyper["lr"][gi], weight_decay=hyper["weight_decay"], foreach=False)
            for gi, grp in enumerate(groups)]
    for gi, (opt, grp) in enumerate(zip(opts, groups)):
        for k, p in enumerate(grp):
            opt.state[p] = {"step": torch.tensor(float(t0)), "exp_avg": m0[gi][k].clone(), "exp_avg_sq": v0[gi][k].clone()}
    for s in range(3):
        before = [[(p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in grp] for opt, grp in zip(opts, groups)]
        before = _state(before)
        coefs, norm_err = [], 0.0
        for gi, (opt, grp) in enumerate(zip(opts, groups)):
            for p, g in zip(grp, grads[s][gi]):
                p.grad = g.clone()
            total = torch.nn.utils.clip_grad_norm_(grp, hyper["max_norm"])
            want = R.norm_ref(grads[s][gi])
            norm_err = max(norm_err, abs(float(total.double()) - want) / (R.U32 * want))
            coefs.append(R.coef_f32(total, hyper["max_norm"]))
            opt.step()
        after = [[(p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in grp] for opt, grp in zip(opts, groups)]
        worst = _judge("torch_cpu", before, after, grads[s], coefs, hyper, t0 + s + 1)
        RATIOS["torch_cpu_norm_u"] = max(RATIOS.get("torch_cpu_norm_u", 0.0), norm_err)
    print("torch cpu: |err| / bar", worst, " norm error in u", RATIOS["torch_cpu_norm_u"])
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("case", CASES)
def test_step_torch_on_cpu_tensors_meets_the_bars(case):
    groups, grads, m0, v0, hyper, t0 = _case(*case)
    opt = OPT.BatchedAdam(groups, **hyper)
    opt.load_state_dict({"step": t0, "exp_avg": m0, "exp_avg_sq": v0})
    assert opt.t == t0
    targets = [[torch.randn(p.shape) for p in grp] for grp in groups]
    for s in range(3):
        before = _state([[(p, opt.exp_avg[i * 3 + k], opt.exp_avg_sq[i * 3 + k]) for k, p in enumerate(grp)]
                         for i, grp in enumerate(groups)])
        t_before = [[t.clone() for t in grp] for grp in targets]
        g_before = [[g.clone() for g in grp] for grp in grads[s]]
        norms = opt.step_torch(targets=targets, tau=0.005, grads=grads[s])
        assert norms.shape == (2,) and norms.dtype == torch.float32
        coefs = []
        for gi in range(2):
            want = R.norm_ref(grads[s][gi])
            assert abs(float(norms[gi].double()) - want) <= 8 * R.U32 * want      # the library's float32 accumulation
            coefs.append(R.coef_f32(norms[gi], hyper["max_norm"]))
        after = [[(p, opt.exp_avg[i * 3 + k], opt.exp_avg_sq[i * 3 + k]) for k, p in enumerate(grp)] for i, grp in enumerate(groups)]
        worst = _judge("step_torch", before, after, grads[s], coefs, hyper, t0 + s + 1)
        for gi, grp in enumerate(groups):
            for p, t, tb, g, gb in zip(grp, targets[gi], t_before[gi], grads[s][gi], g_before[gi]):
                assert torch.equal(t, 0.005 * p.detach() + (1 - 0.005) * tb)       # the reference's blend statement
                assert torch.equal(g, gb)                                          # gradients are left alone
    print("step_torch cpu: |err| / bar", worst)
    assert opt.t == t0 + 3 and max(worst.values()) <= 1.0


def test_from_torch_steps_to_torch_continues_a_pytorch_trajectory():
    groups, grads, _, _, hyper, _ = _case(7, 0, 0.01, 1.0)
    opts = [torch.optim.Adam(grp, lr=hyper["lr"][gi], weight_decay=0.01) for gi, grp in enumerate(groups)]

    def torch_step(s):
        coefs = []
        for gi, (o, grp) in enumerate(zip(opts, groups)):
            for p, g in zip(grp, grads[s][gi]):
                p.grad = g.clone()
            coefs.append(R.coef_f32(torch.nn.utils.clip_grad_norm_(grp, 1.0), 1.0))
            o.step()
        return coefs
    torch_step(0)
    opt = OPT.BatchedAdam.from_torch(opts, max_norm=1.0)
    assert opt.t == 1 and opt.lr == hyper["lr"] and opt.weight_decay == [0.01, 0.01] and opt.betas == (0.9, 0.999)
    before = _state([[(p, opt.exp_avg[i * 3 + k], opt.exp_avg_sq[i * 3 + k]) for k, p in enumerate(grp)] for i, grp in enumerate(groups)])
    norms = opt.step_torch(grads=grads[1])
    after = [[(p, opt.exp_avg[i * 3 + k], opt.exp_avg_sq[i * 3 + k]) for k, p in enumerate(grp)] for i, grp in enumerate(groups)]
    worst = _judge("continued", before, after, grads[1], [R.coef_f32(n, 1.0) for n in norms], hyper, 2)
    opt.to_torch(opts)
    assert all(int(o.state[p]["step"]) == 2 for o, grp in zip(opts, groups) for p in grp)
    before = _state([[(p, o.state[p]["exp_avg"], o.state[p]["exp_avg_sq"]) for p in grp] for o, grp in zip(opts, groups)])
    assert all(torch.equal(b[1], a[1]) and torch.equal(b[2], a[2]) for gb, ga in zip(before, after) for b, a in zip(gb, ga))
    coefs = torch_step(2)
    after = [[(p, o.state[p]["exp_avg"], o.state[p]["exp_avg_sq"]) for p in grp] for o, grp in zip(opts, groups)]
    worst = _judge("continued", before, after, grads[2], coefs, hyper, 3)
    assert all(int(o.state[p]["step"]) == 3 for o, grp in zip(opts, groups) for p in grp)
    assert max(worst.values()) <= 1.0
    sd = opt.state_dict()
    assert sd["step"] == 2 and sd["lr"] == hyper["lr"] and len(sd["exp_avg"]) == 2 and len(sd["exp_avg"][0]) == 3
    other = OPT.BatchedAdam([[p.detach().clone() for p in grp] for grp in groups])
    other.load_state_dict(sd)
    assert other.t == 2 and other.lr == hyper["lr"] and other.weight_decay == [0.01, 0.01]
    assert all(torch.equal(a, b) for a, b in zip(other.exp_avg + other.exp_avg_sq, opt.exp_avg + opt.exp_avg_sq))
    with pytest.raises(ValueError):
        other.load_state_dict({**sd, "exp_avg": sd["exp_avg"][:1]})
    assert other.t == 2


def test_nonfinite_gradient_goes_nan_in_its_group_only():
    groups, grads, _, _, hyper, _ = _case(8, 0, 0.0, 1.0)
    grads[0][1][0][3, 2] = float("nan")
    opt = OPT.BatchedAdam(groups, **hyper)
    keep = [p.detach().clone() for p in groups[0]]
    norms = opt.step_torch(grads=grads[0])
    assert math.isnan(float(norms[1])) and math.isfinite(float(norms[0]))
    assert all(torch.isnan(p).all() for p in groups[1]) and all(torch.isfinite(p).all() for p in groups[0])
    assert all(not torch.equal(p.detach(), k) for p, k in zip(groups[0], keep))
