"""GPU sweep of `BatchedTwinCritic.loss_backward` (`k_marl_critic_grad_rows<MT2,MT3>` -> `k_marl_critic_grad_weights`,
csrc/k_marl_critic_grad.hip) against the float64 oracle of marl_critic_grad_ref.py: every shape of `MARL_CRITIC`
(tests/mlp_sweep_shapes.py) -- five of the six instantiations; <4,2> is the driver's shape in test_marl_critic_grad_hip.py --
and the value edges of the power-of-two delta scaling.  The inputs are those of tests/marl_critic_grad_inputs.py; `BACKWARD_EDGE`
below names what each shape brings to the backward; test_marl_critic_grad_walk_host.py holds the NumPy walk of the
kernels' arithmetic to the same bar at the same inputs, so a failure here is a finding about the kernel.

The bar, the error measure and the helpers are those of test_marl_critic_grad_hip.py, imported: per tensor, for q and for the
loss, device err <= max(8 x the err of `loss_backward_torch` on the same inputs, 2^-22).  On top of it, per case:
  * `last_kernel()` names the instantiation; every output was NaN before the call and is finite after;
  * STRUCTURAL ZEROS: wherever the float64 gradient entry is exactly 0 -- a unit dead on every row: its row of dW, its db
    entry, its column of the next layer's dW -- the device entry is exactly +-0.  `nudge_biases` makes the float32 mask the
    float64 one, so this is derived, not measured; the relative measure above cannot see such an entry unless it is large;
  * the sweep: q has the bits of `forward` on the same object (the backward restates the forward walk), q buffers PAD rows
    longer keep their sentinel, and a second call gives the same bits in every output.
Every figure is printed before it is asserted (pytest -s shows them; a green run is in profiles/marl_critic_grad_margins.txt)."""
import numpy as np
import pytest
import torch

from ris_vec_marl_amd import BatchedTwinCritic
from ris_vec_marl_amd import _native as N
from tests import marl_critic_grad_inputs as I
from tests import marl_critic_grad_ref as G
from tests import mlp_sweep_shapes as SW
from tests import test_marl_critic_grad_hip as TG

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENTINEL = -7.0
AUTO_END = BatchedTwinCritic.GRAD_AUTO_ROWS[1]

#: what each shape of `MARL_CRITIC` brings to the backward that the forward does not have (the forward's edges are in the
#: table itself)
BACKWARD_EDGE = {
    (1, 1, 32, 128, 128): "2 live columns of d fc1.weight; NG = 1: three wavefronts own no group in the d1 loop",
    (1, 15, 32, 512, 128): "16 live columns; <4,1>",
    (16, 1, 64, 128, 256): "17 live columns; <1,2>",
    (127, 1, 160, 256, 128): "four full column tiles; NG = 5",
    (1, 127, 1024, 128, 256): "s_h sized by 2 NG; 148 480 bytes of LDS; eight d1 groups per wavefront",
    (33, 46, 992, 512, 128): "XF = 96 with 15 live columns in the last tile; NG = 31: an uneven d1 loop",
    (24, 40, 96, 256, 256): "<2,2>; NG = 3: wavefront 3 owns no group",
}


def grad_kernel(dims, n_nets):
    return "k_marl_critic_grad_rows<%d,%d>x%d" % (dims[3] // 128, dims[4] // 128, n_nets)


def launch(fn, critic, s, a, y, pad=0, **kw):
    """One call into NaN-filled outputs; q into buffers `pad` rows longer that hold a sentinel beyond n.
    -> (grads, q views [n, 1], loss, the q buffers)"""
    n = len(s)
    grads = [[torch.full_like(t, NAN) for t in gs] for gs in critic.alloc_grads()]
    bufs = tuple(torch.full((n + pad, 1), SENTINEL, device=TG.dev()) for _ in range(critic.n_nets))
    for b in bufs:
        b[:n] = NAN
    qs = tuple(b[:n] for b in bufs)
    loss = torch.full((1,), NAN, device=TG.dev())
    assert fn(s, a, y, grads=grads, q=qs if critic.n_nets == 2 else qs[0], loss=loss, **kw) is loss
    return grads, qs, loss, bufs


def flat(res):
    grads, qs, loss, _ = res
    return [t for gs in grads for t in gs] + list(qs) + [loss]


def same_bits(t, u):
    return torch.equal(t.contiguous().view(torch.int32), u.contiguous().view(torch.int32))


def check_zeros(label, grads, g64, nets=None):
    """-> how many gradient entries are exactly 0 in the oracle; each is exactly +-0 on the device (a NaN is not)"""
    total, bad = 0, []
    for c in (range(len(grads)) if nets is None else nets):
        for k, t in zip(G.KEYS, grads[c]):
            z = g64[c][k] == 0
            got = t.cpu().numpy().reshape(z.shape)
            wrong = int((got[z] != 0).sum())
            total += int(z.sum())
            if wrong:
                bad.append((c + 1, k, wrong, float(np.abs(got[z]).max())))
    print("%s: %d structural zeros, %d of them not 0 on the device" % (label, total, sum(b[2] for b in bad)))
    assert not bad, bad
    return total


def run_case(label, inp, critic, device_path=True, pad=0, **kw):
    """Both paths at `inp`: the kernel named (or none launched), all finite, the bar per tensor, the structural zeros.
    -> (what `launch` gave for the device path, the device tensors (s, a, y), the number of structural zeros)"""
    s, a, y = TG.on_dev(inp.state, inp.action, inp.target)
    before = N.last_kernel()
    res = launch(critic.loss_backward, critic, s, a, y, pad, **kw)
    if device_path:
        assert N.last_kernel().startswith(grad_kernel(inp.dims, critic.n_nets) + " "), N.last_kernel()
    lib = launch(critic.loss_backward_torch, critic, s, a, y)
    if not device_path:
        assert N.last_kernel() == before                      # no launch of this library's
    for t in flat(res):
        assert bool(torch.isfinite(t).all())
    for b in res[3]:
        assert bool((b[len(s):] == SENTINEL).all())
    TG.check_bars(label, TG.errors(*res[:3], inp.g64, inp.loss64, inp.q64), TG.errors(*lib[:3], inp.g64, inp.loss64, inp.q64))
    return res, (s, a, y), check_zeros(label, res[0], inp.g64)


# ------------------------------------------------------------------------------------------------------ the shape sweep
@pytest.mark.parametrize("index,n_nets", SW.MARL_CRITIC_RUNS,
                         ids=["%s-x%d" % (SW.case_id(SW.MARL_CRITIC[i]), k) for i, k in SW.MARL_CRITIC_RUNS])
def test_sweep(index, n_nets):
    case = SW.MARL_CRITIC[index]
    inp = I.sweep(index, n_nets)
    label = "sweep %s x%d" % (SW.case_id(case), n_nets)
    print("%s: %s" % (label, BACKWARD_EDGE[case.dims]))
    assert case.kernel.replace("k_marl_critic", "k_marl_critic_grad_rows") + "x%d" % n_nets == grad_kernel(inp.dims, n_nets)
    assert len(inp.state) == SW.CRITIC_ROWS and not inp.state[0].any() and not inp.action[0].any()
    critic = TG.critic_of(inp.dims, inp.ws, gemm="fused")
    res, (s, a, y), zeros = run_case(label, inp, critic, pad=SW.PAD)
    assert zeros >= 1                                         # a unit dead on all 70 rows, or more

    # q in step with the forward: the same bits
    qf = critic.forward(s, a)
    assert N.last_kernel().startswith(case.kernel + "x%d" % n_nets), N.last_kernel()
    for c, (qb, qv) in enumerate(zip(res[1], qf if n_nets == 2 else (qf,))):
        n_diff = int((qb.view(torch.int32) != qv.view(torch.int32)).sum())
        print("%s: q%d of loss_backward differs from forward in %d of %d rows" % (label, c + 1, n_diff, len(s)))
        assert n_diff == 0

    # a second call: the same bits in every output
    again = launch(critic.loss_backward, critic, s, a, y, SW.PAD)
    assert all(same_bits(t, u) for t, u in zip(flat(res), flat(again)))


# --------------------------------------------------------------------------------------------------------- value edges
@pytest.mark.parametrize("reverse", [False, True], ids=["small-first", "large-first"])
def test_mixed_tiles(reverse):
    """TD errors of 1e-6 in one tile and 1e3 in the other: fails if a tile's scale is taken from the wrong tile or wavefront
    slot, or if launch 2 takes a tile's scale for the layer's"""
    inp = I.mixed_tiles(reverse)
    td = np.abs(inp.q64[0] - inp.target)
    lo, hi = (td[32:], td[:32]) if reverse else (td[:32], td[32:])
    assert lo.max() < 1e-5 and hi.max() > 1e2
    run_case("mixed tiles, %s" % ("large first" if reverse else "small first"), inp, TG.critic_of(inp.dims, inp.ws, gemm="fused"))


def test_large_td():
    """TD errors of order 1e6: every scale exponent is negative"""
    inp = I.large_td()
    assert np.abs(inp.q64[0] - inp.target).max() > 1e6
    run_case("large TD", inp, TG.critic_of(inp.dims, inp.ws, gemm="fused"))


@pytest.mark.parametrize("head_large", [False, True], ids=["tail-large", "head-large"])
def test_more_than_64_tiles(head_large):
    """65 tiles, the last with 12 rows: the second trip of launch 2's loop over the tiles' maxima.  The TD error of tile 64 (or,
    mirrored, of tile 0) is 1e5 x the others': its deltas overflow float16 if the layer's scale leaves that tile out.  Into a
    caller's workspace of exactly the stated size."""
    inp = I.many_tiles(head_large)
    n = len(inp.state)
    assert n == 2060 and -(-n // 32) == 65
    need = N.load().risvec_marl_critic_grad_workspace(n, *inp.dims, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=TG.dev())
    run_case("65 tiles, %s" % ("head large" if head_large else "tail large"), inp, TG.critic_of(inp.dims, inp.ws, gemm="fused"), workspace=ws)


@pytest.mark.parametrize("extra,gemm,device_path", [(0, None, True), (1, None, False), (1, "fused", True)],
                         ids=["auto-end", "auto-end+1", "fused-end+1"])
def test_ends_of_the_auto_range(extra, gemm, device_path):
    """With gemm=None the last row count of `GRAD_AUTO_ROWS` runs the kernels and the next one the library path; gemm="fused"
    runs the kernels there too: 129 tiles, the last with one row"""
    inp = I.auto_range(AUTO_END + extra)
    assert AUTO_END % 32 == 0 and len(inp.state) == AUTO_END + extra
    # any other launch first, so that "unchanged" cannot be the same name written again
    other = TG.critic_of(inp.dims, inp.ws, gemm="fused")
    other.forward(*TG.on_dev(inp.state[:2], inp.action[:2]))
    assert N.last_kernel().startswith("k_marl_critic<1,1>x2")
    critic = TG.critic_of(inp.dims, inp.ws, **({} if gemm is None else {"gemm": gemm}))
    assert critic._grad_device(len(inp.state)) == device_path
    run_case("%s rows, gemm=%s" % (len(inp.state), gemm), inp, critic, device_path)


@pytest.mark.parametrize("n_nets", [1, 2])
def test_zero_td_error(n_nets):
    """target = the q of net 1 that a first call wrote: e = 0 on every row of net 1, so amax = 0 at every tile and layer -- the
    1e-30 floor and the +80 clamp.  Net 1's gradients are exactly 0, with no NaN; net 2's meet the oracle, and the loss is
    net 2's term."""
    first = I.plain_small(n_nets)
    critic = TG.critic_of(first.dims, first.ws, gemm="fused")
    label = "zero TD x%d" % n_nets
    s, a, y = TG.on_dev(first.state, first.action, first.target)
    q1 = launch(critic.loss_backward, critic, s, a, y)[1][0].clone()
    inp = I.with_target(first, q1.cpu().numpy().reshape(-1))
    y0 = q1.view(-1)
    res = launch(critic.loss_backward, critic, s, a, y0)
    lib = launch(critic.loss_backward_torch, critic, s, a, y0)
    assert N.last_kernel().startswith(grad_kernel(inp.dims, n_nets) + " ")
    assert same_bits(res[1][0], q1)
    for t in flat(res):
        assert bool(torch.isfinite(t).all())
    for k, t in zip(G.KEYS, res[0][0]):
        print("%s n1.%-12s largest |g| %.3g" % (label, k, float(t.abs().max())))
        assert not bool(t.any()), k                           # exactly +-0
    if n_nets == 1:
        print("%s loss %.3g" % (label, float(res[2])))
        assert float(res[2]) == 0.0
        return
    term2 = G.grads64(inp.ws[1], inp.state, inp.action, inp.target)[1]
    de, le = (TG.errors(*r[:3], inp.g64, term2, inp.q64) for r in (res, lib))
    keep = lambda d: {k: v for k, v in d.items() if k == "loss" or k.startswith("n2.")}     # noqa: E731
    TG.check_bars(label, keep(de), keep(le))
    check_zeros(label, res[0], inp.g64, nets=[1])


def test_dead_fc3():
    """fc3.bias = -1e3: every h3 is 0, q = q.bias, d q.bias meets the oracle, every other gradient is exactly 0"""
    inp = I.dead_layer("fc3")
    res, _, _ = run_case("dead fc3", inp, TG.critic_of(inp.dims, inp.ws, gemm="fused"))
    qb = torch.from_numpy(inp.ws[0]["q.bias"]).to(TG.dev())
    assert same_bits(res[1][0], qb.expand(len(inp.state)).reshape(-1, 1))
    for k, t in zip(G.KEYS, res[0][0]):
        assert bool(t.any()) == (k == "q.bias"), k


def test_dead_units_of_fc2():
    """fc2.bias[:64] = -1e3: rows 0 - 63 of d fc2.weight, d fc2.bias[:64] and columns 0 - 63 of d fc3.weight are exactly 0, the
    rest meets the bar"""
    inp = I.dead_layer("fc2")
    res, _, _ = run_case("dead fc2[:64]", inp, TG.critic_of(inp.dims, inp.ws, gemm="fused"))
    g, u = dict(zip(G.KEYS, res[0][0])), I.DEAD_UNITS
    assert not bool(g["fc2.weight"][:u].any()) and not bool(g["fc2.bias"][:u].any()) and not bool(g["fc3.weight"][:, :u].any())
    assert bool(g["fc2.weight"][u:].any()) and bool(g["fc3.weight"][:, u:].any())
