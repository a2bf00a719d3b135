"""CPU-side tests of `ris_vec_marl_amd._critic_nets`, what `BatchedTwinCritic` and `BatchedLocalCritics` share around a group
of `CriticNetwork` nets: the helpers take the device as an argument, so everything here runs on CPU tensors."""
import ctypes as C
import math

import pytest
import torch

from ris_vec_marl_amd import _critic_nets as CN
from ris_vec_marl_amd import _native as N
from ris_vec_marl_amd import _weights as W
from ris_vec_marl_amd import marl_critic as MC

CPU = torch.device("cpu")
IN, F1, F2, F3 = 5, 32, 128, 128
DIMS = (3, 2, F1, F2, F3)                                     # state + action = IN


def drawn_as_before(g, count):
    """The constructors' draw loop as it stood before the nets were drawn by one function, restated literally."""
    def uni(*shape, r):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * r).to(CPU)
    nets = []
    for _ in range(count):
        net = {}
        for w, b, fan_out, fan_in in (("W1", "b1", F1, IN), ("W2", "b2", F2, F1), ("W3", "b3", F3, F2), ("Wq", "bq", 1, F3)):
            r = 1.0 / math.sqrt(fan_in)
            net[w] = uni(fan_out, fan_in, r=r)
            net[b] = uni(fan_out, r=r)
        nets.append(net)
    return nets


def test_net_is_the_class_marl_critic_exports():
    assert MC._Net is CN._Net and issubclass(MC.BatchedTwinCritic, CN.CriticNets)
    assert MC.BatchedTwinCritic._SD is CN._Net._SD


def test_seeded_construction_draws_what_the_constructors_drew():
    g, g_ref = torch.Generator(device="cpu").manual_seed(7), torch.Generator(device="cpu").manual_seed(7)
    want = drawn_as_before(g_ref, 4)
    nets = [CN.draw_net(g, IN, F1, F2, F3, CPU) for _ in range(2)]
    nets += [CN.draw_net(g, IN, F1, F2, F3, CPU) for _ in range(2)]      # the second agent's: the same generator goes on
    for net, ref in zip(nets, want):
        assert isinstance(net, CN._Net) and net.device == CPU
        for a in CN._Net._WEIGHTS:
            t = getattr(net, a)
            assert t.dtype == torch.float32 and t.shape == ref[a].shape and torch.equal(t, ref[a]), a
    assert not torch.equal(nets[0].W1, nets[2].W1)


class Group(CN.CriticNets):
    """The least a subclass sets: one group of two nets on the CPU."""

    def __init__(self, seed=3):
        self.device, self._dims, self.n_nets = CPU, DIMS, 2
        self._init_modes(None, False, "no fused kernel on the CPU")
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.nets = [CN.draw_net(g, IN, F1, F2, F3, CPU) for _ in range(2)]

    def _shape(self):
        return "a CPU group"

    def _all_nets(self):
        return self.nets


def test_stale_rebuild_on_the_host_path():
    grp = Group()
    assert (grp.gemm, grp.pack, grp.packs, grp._pack_workspace) == ("library", "host", 0, None)
    packed = lambda: [net._packed[1] for net in grp.nets]     # noqa: E731
    grp._rebuild_stale(grp.nets)
    assert grp.packs == 2
    first = packed()
    for net, (ws, sc) in zip(grp.nets, first):
        want_ws, want_sc = MC.pack_marl_critic_weights(net.W1, net.W2, net.W3)
        assert torch.equal(ws, want_ws) and torch.equal(sc, want_sc)
    grp._rebuild_stale(grp.nets)                              # nothing is stale
    assert grp.packs == 2 and all(a[0] is b[0] and a[1] is b[1] for a, b in zip(first, packed()))
    grp.nets[1].W2.add_(0.25)                                 # in place: seen through the version counter
    grp._rebuild_stale(grp.nets)
    second = packed()
    assert grp.packs == 3 and second[0][0] is first[0][0] and second[1][0] is not first[1][0]
    assert torch.equal(second[1][0], MC.pack_marl_critic_weights(grp.nets[1].W1, grp.nets[1].W2, grp.nets[1].W3)[0])
    assert not torch.equal(second[1][0], first[1][0])
    grp.mark_stale()
    grp._rebuild_stale(grp.nets)
    assert grp.packs == 5 and all(a[0] is not b[0] for a, b in zip(second, packed()))
    grp._rebuild_stale(grp.nets[:1])                          # one group's nets only, none stale
    assert grp.packs == 5
    with pytest.raises(ValueError, match="pack='device' is not available for a CPU group"):
        grp.pack = "device"
    assert grp.pack == "host" and grp.packs == 5 and grp.nets[0]._stale() is None
    assert grp._fused(1) is False and grp.fused_min_rows == CN.CriticNets.AUTO_MIN_ROWS == 1


def test_q_outs_accepts_and_refuses():
    for shape in ((4, 1), (3, 4, 1)):
        a, b = torch.zeros(shape), torch.zeros(shape)
        assert CN.q_outs(None, 2, shape, "q", CPU) is None
        got = CN.q_outs([a, b], 2, shape, "q", CPU)
        assert isinstance(got, tuple) and got[0] is a and got[1] is b
        assert CN.q_outs(a, 1, shape, "q", CPU) == (a,)
        hold = r"td_target: q must hold 2 tensors of shape \(%s\)" % ", ".join(str(d) for d in shape)
        for bad in (a, (a,), (a, b, b), (a, None), (None, None)):
            with pytest.raises(ValueError, match=hold):
                CN.q_outs(bad, 2, shape, "td_target: q", CPU)
        with pytest.raises(ValueError, match=r"forward: out must hold 1 tensors of shape \(%s\)" % ", ".join(str(d) for d in shape)):
            CN.q_outs((a, b), 1, shape, "forward: out", CPU)
        for bad in (torch.zeros(shape[:-1]), torch.zeros((5,) + shape[1:]), torch.zeros(shape, dtype=torch.float64),
                    torch.zeros(shape + (2,))[..., 0]):
            with pytest.raises(ValueError, match="td_target: q"):
                CN.q_outs((a, bad), 2, shape, "td_target: q", CPU)
        with pytest.raises(ValueError, match="td_target: q: the two tensors are the same"):
            CN.q_outs((a, a), 2, shape, "td_target: q", CPU)


def test_entropy_args_and_the_three_expression_forms():
    n, V = 6, 3
    g = torch.Generator().manual_seed(1)
    coef = torch.rand(2, generator=g) + 0.1
    for shapes, text in ((((n,), (n, 1)), r"\(6,\) or \(6, 1\)"), (((n, V),), r"\(6, 3\)")):
        lp, li = torch.randn(shapes[-1], generator=g), torch.randn(shapes[0], generator=g)
        assert CN.entropy_args(None, None, None, shapes, CPU) is None
        assert CN.entropy_args(None, None, coef, shapes, CPU) is None         # no logp: the term is absent, coef unused
        for a, b in ((lp, li), (lp, None), (None, li)):
            assert CN.entropy_args(a, b, coef, shapes, CPU) is coef
            with pytest.raises(ValueError, match="td_target: logp_power / logp_intent need coef, a float32 tensor of 2 values on cpu"):
                CN.entropy_args(a, b, None, shapes, CPU)
        for bad in (torch.zeros(3), torch.zeros(2, dtype=torch.float64), torch.zeros(4)[::2], [0.1, 0.2]):
            with pytest.raises(ValueError, match="td_target: coef must be a contiguous float32 tensor of 2 values on cpu"):
                CN.entropy_args(lp, None, bad, shapes, CPU)
        for bad in (torch.zeros(n + 1), torch.zeros(V, n), lp.double(), torch.zeros(shapes[0] + (2,))[..., 0]):
            with pytest.raises(ValueError, match="td_target: logp_power must be a contiguous float32 tensor of shape %s on cpu" % text):
                CN.entropy_args(bad, li, coef, shapes, CPU)
            with pytest.raises(ValueError, match="td_target: logp_intent must be a contiguous float32 tensor of shape %s on cpu" % text):
                CN.entropy_args(None, bad, coef, shapes, CPU)
    m, lp, li = torch.randn(V, n, generator=g), torch.randn(n, V, generator=g).t(), torch.randn(n, V, generator=g).t()
    c0, c1 = coef[0], coef[1]
    assert torch.equal(CN.minus_entropy(m, coef, lp, li), m - (c0 * lp + c1 * li))
    assert torch.equal(CN.minus_entropy(m, coef, lp, None), m - c0 * lp)
    assert torch.equal(CN.minus_entropy(m, coef, None, li), m - c1 * li)
    assert CN.minus_entropy(m, None, None, None) is m
    # the grouping is the reference's: one subtraction of the summed terms, not two subtractions
    two = (m - c0 * lp) - c1 * li
    assert two.dtype == torch.float32 and not torch.equal(CN.minus_entropy(m, coef, lp, li), two)
    assert torch.equal(CN.minus_entropy(m, coef.view(1, 2), lp, li), m - (c0 * lp + c1 * li))


def test_q_net_is_the_relu_mlp():
    g = torch.Generator(device="cpu").manual_seed(5)
    net = CN.draw_net(g, IN, F1, F2, F3, CPU)
    x = torch.randn(7, IN, generator=g)
    F = torch.nn.functional
    h = torch.relu(F.linear(x, net.W1, net.b1))
    h = torch.relu(F.linear(h, net.W2, net.b2))
    h = torch.relu(F.linear(h, net.W3, net.b3))
    assert torch.equal(CN.q_net(net, x), F.linear(h, net.Wq, net.bq)) and CN.q_net(net, x).shape == (7, 1)


def test_net_table_holds_every_pointer():
    g = torch.Generator(device="cpu").manual_seed(2)
    nets = [CN.draw_net(g, IN, F1, F2, F3, CPU) for _ in range(4)]
    packed = [MC.pack_marl_critic_weights(net.W1, net.W2, net.W3) for net in nets]
    for give in (lambda x: x, iter):                          # lists or any iterables
        table = CN.net_table(4, give(nets), give(packed))
        assert len(table) == 4 and C.sizeof(table) == 4 * C.sizeof(N.RisVecMarlCriticNet)
        for row, net, (ws, sc) in zip(table, nets, packed):
            assert row.wstream == ws.data_ptr() and row.wstream_bytes == ws.numel() * 2 == MC.marl_critic_geom(*DIMS).rows * 1024
            assert row.scales == sc.data_ptr()
            assert (row.b1, row.b2, row.b3, row.qw, row.qb) == tuple(getattr(net, a).data_ptr() for a in ("b1", "b2", "b3", "Wq", "bq"))
    assert len({row.wstream for row in table}) == 4


def test_soft_update_splits_into_runs_of_the_launch_limit():
    assert W.SOFT_UPDATE_MAX == 32                            # kSoftUpdateMax: what `risvec_soft_update` takes at most
    assert W.soft_update_runs(33) == [slice(0, 32), slice(32, 33)]
    assert W.soft_update_runs(32) == [slice(0, 32)]
    assert W.soft_update_runs(1) == [slice(0, 1)] and W.soft_update_runs(16) == [slice(0, 16)]
    assert W.soft_update_runs(64) == [slice(0, 32), slice(32, 64)]
    assert W.soft_update_runs(65) == [slice(0, 32), slice(32, 64), slice(64, 65)]
    # no pairs: one empty run, so the entry point is still asked and refuses n_tensors = 0
    assert W.soft_update_runs(0) == [slice(0, 0)]
    pairs = list(range(70))
    assert [p for run in W.soft_update_runs(70) for p in pairs[run]] == pairs


def test_done_and_gamma_check_is_the_one_td_args_runs():
    done = torch.zeros(4, dtype=torch.bool)
    W.done_gamma_args(done, 0.99, 4, CPU)
    W.done_gamma_args(done.to(torch.uint8), 0.0, 4, CPU)
    W.td_args(torch.zeros(4), done, 0.99, 4, CPU)
    for bad in (None, torch.zeros(4), torch.zeros(5, dtype=torch.bool), torch.zeros(4, 1, dtype=torch.bool),
                torch.zeros(8, dtype=torch.bool)[::2]):
        for check in (lambda d: W.done_gamma_args(d, 0.99, 4, CPU), lambda d: W.td_args(torch.zeros(4), d, 0.99, 4, CPU)):
            with pytest.raises(ValueError, match=r"td_target: done must be a contiguous bool or uint8 tensor of shape \(4,\) on cpu"):
                check(bad)
    for gamma in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="td_target: gamma must be finite"):
            W.done_gamma_args(done, gamma, 4, CPU)
        with pytest.raises(ValueError, match="td_target: gamma must be finite"):
            W.td_args(torch.zeros(4), done, gamma, 4, CPU)
    with pytest.raises(ValueError, match="td_target: reward"):
        W.td_args(None, torch.zeros(5), float("nan"), 4, CPU)     # the reward is looked at first
