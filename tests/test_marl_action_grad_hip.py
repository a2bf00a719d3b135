"""`BatchedTwinCritic.action_grad` (`risvec_marl_critic_action_grad`, csrc/k_marl_critic_action_grad.hip) on the GPU against the
float64 oracle of marl_action_grad_ref.py.

The bar is `loss_backward`'s: per tensor (`out`, each q_c, q_min) err = max|t - t64| / max|t64| must be <= max(8 x the err of
`action_grad_torch` on the same inputs in the same test, 2^-22) -- 8 = 4 (2^-22 against 2^-24 per product) x 2 (the extra split
roundings on the delta chain); 2^-22 is one split product's rounding, below which the ratio means nothing.  Every figure is
printed before it is asserted; those of a green run of the kernels as committed are in profiles/marl_action_grad_margins.txt.

The sweep: every (index, n_nets) of `MARL_CRITIC_RUNS` (tests/mlp_sweep_shapes.py) at 77 rows -- three tiles, 13 live rows in
the last --, the driver's shapes (40, 80) and (20, 24) at 1024-512-256 (<4,2>, the instantiation the table lacks) at 77 and 256
rows, case 0 at 1, 32 and 33 rows.  What the table's shapes bring to the last product, W1^T d1 on the action columns:

    (1, 1, ..)      A = 1: one live column of one output tile
    (127, 1, ..)    the action column is the LAST of W1's row: an unclamped read of the tile's other 31 columns leaves the tensor
    (1, 127, ..)    four output tiles, 31 live columns in the last; NG = 32: both mask words of h1 full
    (33, 46, ..)    output tiles that start off a 32-column boundary of W1; NG = 31
    (1, 15, ..) / (16, 1, ..) / (24, 40, ..)   MT2 = 4 with NG = 1, MT3 = 2 with NG = 2, <2,2> with two output tiles

The input recipe asserts its two conditions on the oracle alone (no ReLU unit inside the guard of `nudge_biases`; q_1 and q_2
apart by 1e-4 max|q| on every row that is not a planted tie) and has each net selected on half of the rows."""
import functools

import numpy as np
import pytest
import torch

from ris_vec_marl_amd import BatchedTwinCritic
from ris_vec_marl_amd import _native as N
from tests import marl_action_grad_ref as R
from tests import mlp_sweep_shapes as SW

pytestmark = pytest.mark.gpu
FLOOR = R.FLOOR
PAD = SW.PAD
SENTINEL = -7.25
DRIVER8 = (40, 80, 1024, 512, 256)
DRIVER4 = (20, 24, 1024, 512, 256)
MID = (40, 88, 160, 256, 128)

SWEEP = [("sweep-%s-x%d-n77" % (SW.case_id(SW.MARL_CRITIC[i]), k), SW.MARL_CRITIC[i].dims, 77, k, SW.seeds("marl", i))
         for i, k in SW.MARL_CRITIC_RUNS]
SWEEP += [("driver-%s-n%d" % (SW.case_id(SW.Case(d, "", "")), n), d, n, 2, (1190 + j, 1195 + j))
          for j, d in enumerate((DRIVER8, DRIVER4)) for n in (77, 256)]
SWEEP += [("rows-%s-n%d" % (SW.case_id(SW.MARL_CRITIC[0]), n), SW.MARL_CRITIC[0].dims, n, 2, SW.seeds("marl", 0)) for n in (1, 32, 33)]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def critic_of(dims, ws, **kw):
    c = BatchedTwinCritic(*dims, n_nets=len(ws), device=dev(), **kw)
    c.load_state_dict(*ws)
    return c


def on_dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in arrays)


class Run:
    """One call of `fn` into buffers that are PAD rows longer than n, NaN in the first n rows and SENTINEL beyond"""

    def __init__(self, fn, critic, s, a, scale=1.0, **kw):
        n, A, k = len(s), critic.action_dims, critic.n_nets

        def buf(*shape):
            t = torch.full((n + PAD,) + shape, SENTINEL, device=dev())
            t[:n] = float("nan")
            return t
        self.big = [buf(A), buf()] + [buf(1) for _ in range(k)]
        self.out, self.q_min = self.big[0][:n], self.big[1][:n]
        self.q = tuple(t[:n] for t in self.big[2:])
        got = fn(s, a, out=self.out, q_min=self.q_min, q=self.q if k == 2 else self.q[0], scale=scale, **kw)
        assert got is self.out
        self.n = n

    def tensors(self):
        return [self.out, self.q_min] + list(self.q)

    def check_written(self):
        for t in self.tensors():
            assert bool(torch.isfinite(t).all())              # every element was NaN before
        for t in self.big:
            assert bool((t[self.n:] == SENTINEL).all())       # nothing beyond n was written

    def errors(self, inp, scale=1.0, out64=None):
        e = {"out": R.rel_err(self.out.cpu().numpy(), scale * inp.out64 if out64 is None else out64),
             "q_min": R.rel_err(self.q_min.cpu().numpy(), inp.q_min64)}
        for c, q in enumerate(self.q):
            e["q%d" % (c + 1)] = R.rel_err(q.cpu().numpy(), inp.q64[c])
        return e


def same_bits(t, u):
    return torch.equal(t.contiguous().view(torch.int32), u.contiguous().view(torch.int32))


def check_bars(label, dev_err, lib_err):
    bad = []
    for k in dev_err:
        bar = max(8 * lib_err[k], FLOOR)
        print("%s %-6s device %.3g  library %.3g  bar %.3g" % (label, k, dev_err[k], lib_err[k], bar))
        if not dev_err[k] <= bar:
            bad.append((k, dev_err[k], bar))
    assert not bad, bad


@pytest.mark.parametrize("label,dims,n,n_nets,seeds", SWEEP, ids=[c[0] for c in SWEEP])
def test_action_grad_meets_the_oracle(label, dims, n, n_nets, seeds):
    inp = R.inputs(dims, n, n_nets, *seeds)
    critic = critic_of(dims, inp.ws, gemm="fused")
    s, a = on_dev(inp.state, inp.action)
    first = Run(critic.action_grad, critic, s, a)
    assert N.last_kernel() == ("k_marl_critic_action_grad_rows<%d,%d>x%d -> k_marl_critic_action_grad_select"
                               % (dims[3] // 128, dims[4] // 128, n_nets))
    first.check_written()
    again = Run(critic.action_grad, critic, s, a)
    for t, u in zip(first.tensors(), again.tensors()):
        assert same_bits(t, u)                                # determinism: identical bits
    fwd = critic.forward(s, a)
    for q, f in zip(first.q, fwd if n_nets == 2 else (fwd,)):
        assert same_bits(q, f)                                # the forward walk of k_marl_critic
    want_min = torch.minimum(first.q[0], first.q[1]) if n_nets == 2 else first.q[0]
    assert same_bits(first.q_min.view(n, 1), want_min)
    lib = Run(critic.action_grad_torch, critic, s, a)
    lib.check_written()
    check_bars(label, first.errors(inp), lib.errors(inp))


@functools.lru_cache(maxsize=None)
def tie_case():
    return R.tie_inputs(MID, 77, 61, 17)


def test_tie_gives_each_net_half():
    """On the rows whose action is exactly 0 the two nets -- equal but for fc1.weight's action columns -- give the same q bit
    for bit, and `out` there is 0.5 (g_1 + g_2), `torch.min`'s backward, not either net's gradient."""
    inp, tie = tie_case()
    critic = critic_of(MID, inp.ws, gemm="fused")
    s, a = on_dev(inp.state, inp.action)
    run, lib = Run(critic.action_grad, critic, s, a), Run(critic.action_grad_torch, critic, s, a)
    run.check_written()
    rows = torch.from_numpy(tie).to(dev())
    assert same_bits(run.q[0][rows], run.q[1][rows])
    assert not bool((run.q[0][~rows] == run.q[1][~rows]).any())
    half = 0.5 * (inp.g64[0] + inp.g64[1])
    assert np.array_equal(inp.out64[tie], half[tie])
    dev_err, lib_err = run.errors(inp), lib.errors(inp)
    dev_err["tie"] = R.rel_err(run.out[rows].cpu().numpy(), half[tie])
    lib_err["tie"] = R.rel_err(lib.out[rows].cpu().numpy(), half[tie])
    bar = max(8 * lib_err["tie"], FLOOR)
    for c in range(2):                                        # the test can tell the rules apart: one net alone is far off
        miss = R.rel_err(inp.g64[c][tie], half[tie])
        print("tie: net %d alone misses by %.3g, bar %.3g" % (c + 1, miss, bar))
        assert miss > 1000 * bar
    check_bars("tie %s x 77" % (MID,), dev_err, lib_err)


def test_one_net_is_its_own_gradient():
    """n_nets == 1: out = scale dq / da and q_min = q"""
    inp = R.inputs(MID, 77, 1, 1141, 1146)
    critic = critic_of(MID, inp.ws, gemm="fused")
    s, a = on_dev(inp.state, inp.action)
    scale = 0.375
    run, lib = Run(critic.action_grad, critic, s, a, scale), Run(critic.action_grad_torch, critic, s, a, scale)
    run.check_written()
    assert same_bits(run.q_min.view(-1, 1), run.q[0])
    assert np.array_equal(inp.out64, inp.g64[0])
    check_bars("one net %s x 77" % (MID,), run.errors(inp, scale), lib.errors(inp, scale))


def test_scale():
    """scale = 2^-8 gives exactly 2^-8 x the bits of scale = 1; scale = -1 / 77 (the actor loss's mean, negated) stays within the
    bar; q and q_min do not depend on it"""
    inp = R.inputs(MID, 77, 2, 1151, 1156)
    critic = critic_of(MID, inp.ws, gemm="fused")
    s, a = on_dev(inp.state, inp.action)
    one, small = Run(critic.action_grad, critic, s, a, 1.0), Run(critic.action_grad, critic, s, a, 2.0 ** -8)
    assert same_bits(small.out, one.out * 2.0 ** -8)
    for t, u in zip(one.tensors()[1:], small.tensors()[1:]):
        assert same_bits(t, u)
    sc = -1.0 / 77
    run, lib = Run(critic.action_grad, critic, s, a, sc), Run(critic.action_grad_torch, critic, s, a, sc)
    check_bars("scale -1/77", run.errors(inp, sc), lib.errors(inp, sc))


def test_small_deltas_are_scaled_before_the_split():
    """The q layer x 2^-24: d3 = q.weight [h3 > 0] is of order 2^-26, below float16's normal range, and so is every delta after it.
    The case that fails if the deltas are split unscaled."""
    inp = R.inputs(MID, 77, 2, 1161, 1166, None, 2.0 ** -24)
    assert max(float(np.abs(w["q.weight"]).max()) for w in inp.ws) < 2.0 ** -24
    critic = critic_of(MID, inp.ws, gemm="fused")
    s, a = on_dev(inp.state, inp.action)
    run, lib = Run(critic.action_grad, critic, s, a), Run(critic.action_grad_torch, critic, s, a)
    run.check_written()
    assert float(np.abs(inp.out64).max()) > 0
    check_bars("q.weight x 2^-24", run.errors(inp), lib.errors(inp))


def test_views_with_rows_beyond_n_are_not_read():
    inp = R.inputs(MID, 33, 2, 1171, 1176)
    critic = critic_of(MID, inp.ws, gemm="fused")
    s, a = on_dev(inp.state, inp.action)
    big = [torch.full((64, t.shape[1]), float("nan"), device=dev()) for t in (s, a)]
    for b, t in zip(big, (s, a)):
        b[:33] = t
    clean, viewed = Run(critic.action_grad, critic, s, a), Run(critic.action_grad, critic, big[0][:33], big[1][:33])
    viewed.check_written()
    for t, u in zip(clean.tensors(), viewed.tensors()):
        assert same_bits(t, u)


def test_shared_weights_are_read_in_place_after_an_update():
    """After an in-place update of shared weights the next call sees them: the stale stream is rebuilt (fc1's for the forward)
    and W1, W2, W3 are read where they are."""
    inp = R.inputs(MID, 77, 2, 1181, 1186)
    other = R.inputs(MID, 77, 2, 1281, 1286)
    params = [{k: torch.from_numpy(w[k].copy()).to(dev()) for k in w} for w in other.ws]
    critic = BatchedTwinCritic(*MID, device=dev(), gemm="fused")
    critic.pack = "device"
    critic.share_state_dict(*params)
    s, a = on_dev(inp.state, inp.action)
    Run(critic.action_grad, critic, s, a)
    packs = critic.packs
    for p, w in zip(params, inp.ws):
        for k in p:
            p[k].copy_(torch.from_numpy(w[k]))
    run, lib = Run(critic.action_grad, critic, s, a), Run(critic.action_grad_torch, critic, s, a)
    assert critic.packs == packs + 2
    check_bars("shared %s x 77" % (MID,), run.errors(inp), lib.errors(inp))


def test_fallbacks_launch_nothing_of_this_library():
    inp = R.inputs(MID, 33, 2, 1171, 1176)
    s, a = on_dev(inp.state, inp.action)
    fused = critic_of(MID, inp.ws, gemm="fused")
    lo_hi = BatchedTwinCritic.ACTION_GRAD_AUTO_ROWS
    for kw, state, action in (({"gemm": "library"}, s, a), ({}, s, a)):
        critic = critic_of(MID, inp.ws, **kw)
        if not kw and lo_hi != ():                            # gemm=None: a row count beyond the measured range
            reps = -(-(lo_hi[1] + 1) // 33)
            state, action = s.repeat(reps, 1)[:lo_hi[1] + 1].contiguous(), a.repeat(reps, 1)[:lo_hi[1] + 1].contiguous()
        fused.forward(s, a)
        before = N.last_kernel()
        assert before.startswith("k_marl_critic<")
        run = Run(critic.action_grad, critic, state, action, -0.5)
        assert N.last_kernel() == before
        run.check_written()
        want = Run(critic.action_grad_torch, critic, state, action, -0.5)
        for t, u in zip(run.tensors(), want.tensors()):       # the same statements into the same buffers
            assert same_bits(t, u)
    if lo_hi != ():                                           # and inside it gemm=None takes the device path
        critic = critic_of(MID, inp.ws)
        reps = -(-lo_hi[0] // 33)
        Run(critic.action_grad, critic, s.repeat(reps, 1)[:max(lo_hi[0], 33)].contiguous(), a.repeat(reps, 1)[:max(lo_hi[0], 33)].contiguous())
        assert N.last_kernel().startswith("k_marl_critic_action_grad_rows<2,1>x2")


def test_refusals():
    inp = R.inputs(MID, 33, 2, 1171, 1176)
    critic = critic_of(MID, inp.ws, gemm="fused")
    s, a = on_dev(inp.state, inp.action)
    with pytest.raises(ValueError, match="detach it"):
        critic.action_grad(s, a.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        critic.action_grad(s, a.double())                     # would have to be converted
    with pytest.raises(ValueError):
        critic.action_grad(s, a[:, :-1])                      # not this critic's width, and not contiguous
    with pytest.raises(ValueError):
        critic.action_grad(s, a, out=torch.empty(33, MID[1] + 1, device=dev()))
    with pytest.raises(ValueError):
        critic.action_grad(s, a, q_min=torch.empty(34, device=dev()))
    with pytest.raises(ValueError):
        critic.action_grad(s, a, q=torch.empty(33, 1, device=dev()))          # two nets: a pair
    with pytest.raises(ValueError):
        critic.action_grad(s, a, scale=float("nan"))
    with pytest.raises(ValueError):
        critic.action_grad(s, a, workspace=torch.empty(64, device=dev()))     # not uint8
    with pytest.raises(ValueError, match="workspace_bytes"):
        critic.action_grad(s, a, workspace=torch.empty(64, dtype=torch.uint8, device=dev()))      # too small
