"""`BatchedTwinCritic.loss_backward` (`risvec_marl_critic_grad`, csrc/k_marl_critic_grad.hip) on the GPU against the float64
oracle of marl_critic_grad_ref.py, at the smallest shapes at which the walk can go wrong:

    (5, 10, 32, 128, 128) x 1, 33     one k-step, one fc1 group (three wavefronts idle in fc1), one tile per wavefront; a tile
                                      with one live row
    (40, 88, 160, 256, 128) x 31, 64  128 inputs = eight full k-steps, 5 fc1 groups over 4 wavefronts, MT2 = 2
    (20, 24, 96, 512, 256) x 97       44 inputs: the second column tile of d fc1.weight has 12 live columns; MT2 = 4, MT3 = 2;
                                      three full tiles + 1 row
    (40, 80, 1024, 512, 256) x 64, 256  the driver's 8 vehicles at the reference's batch; n_nets = 1 once

Per case and per tensor err = max|g - g64| / max|g64|, likewise for the loss and q.  The bar: device err <= max(8 x the err of
`loss_backward_torch` on the same inputs in the same test, 2^-22) -- 8 = 4 (2^-22 against 2^-24 per product) x 2 (the two
extra split roundings on the delta chain); 2^-22 is one split product's rounding, below which the ratio means nothing.  Every
weight set went through `nudge_biases`, whose closing assert (no ReLU unit within 1e-4 of its layer's scale of the kink) is a
condition of every comparison.  The errors of a green run of the kernels as committed are in
profiles/marl_critic_grad_margins.txt."""
import functools

import numpy as np
import pytest
import torch

from ris_vec_marl_amd import BatchedAdam, BatchedTwinCritic
from ris_vec_marl_amd import _native as N
from tests import marl_critic_grad_ref as G

pytestmark = pytest.mark.gpu
DRIVER8 = (40, 80, 1024, 512, 256)
FLOOR = 2.0 ** -22
CASES = [((5, 10, 32, 128, 128), 1, 2), ((5, 10, 32, 128, 128), 33, 2), ((40, 88, 160, 256, 128), 31, 2),
         ((40, 88, 160, 256, 128), 64, 2), ((20, 24, 96, 512, 256), 97, 2), (DRIVER8, 64, 2), (DRIVER8, 256, 2), (DRIVER8, 64, 1)]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def case(dims, n, n_nets, small_td=False):
    """The nudged weight sets, the batch, the target and the float64 oracle of one case: computed once, shared, not modified."""
    state, action = G.random_batch(dims, n, 7, dims[0] // 5)
    ws = [G.nudge_biases(G.random_net(dims, 41 + c), (state, action))[0] for c in range(n_nets)]
    rng = np.random.default_rng(9)
    if small_td:
        q64 = G.critic_q64(ws[0], state, action)
        target = (q64 + 1e-4 * rng.normal(0, 1, n)).astype(np.float32)
    else:
        target = rng.normal(0, 1, n).astype(np.float32)
    g64, loss64, q64 = G.loss_grads64(ws, state, action, target)
    return ws, state, action, target, g64, loss64, q64


def critic_of(dims, ws, **kw):
    c = BatchedTwinCritic(*dims, n_nets=len(ws), device=dev(), **kw)
    c.load_state_dict(*ws)
    return c


def on_dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in arrays)


def errors(grads, qs, loss, g64, loss64, q64):
    """{name: err} of every gradient tensor, q and the loss against the oracle"""
    out = {"loss": G.rel_err(loss.cpu().numpy(), [loss64])}
    for c, (gs, q) in enumerate(zip(grads, qs)):
        out["n%d.q" % (c + 1)] = G.rel_err(q.cpu().numpy(), q64[c])
        for k, t in zip(G.KEYS, gs):
            assert tuple(t.shape) == g64[c][k].shape, k
            out["n%d.%s" % (c + 1, k)] = G.rel_err(t.cpu().numpy(), g64[c][k])
    return out


def run_both(critic, state, action, target):
    """(device errors' inputs, library errors' inputs): grads, q, loss of each path, pre-filled with NaN"""
    res = []
    for fn in (critic.loss_backward, critic.loss_backward_torch):
        grads = [[torch.full_like(t, float("nan")) for t in gs] for gs in critic.alloc_grads()]
        qs = tuple(torch.full((len(state), 1), float("nan"), device=dev()) for _ in range(critic.n_nets))
        loss = torch.full((1,), float("nan"), device=dev())
        got = fn(state, action, target, grads=grads, q=qs if critic.n_nets == 2 else qs[0], loss=loss)
        assert got is loss
        res.append((grads, qs, loss))
    return res


def check_bars(label, dev_err, lib_err):
    bad = []
    for k in dev_err:
        bar = max(8 * lib_err[k], FLOOR)
        print("%s %-16s device %.3g  library %.3g  bar %.3g" % (label, k, dev_err[k], lib_err[k], bar))
        if not dev_err[k] <= bar:
            bad.append((k, dev_err[k], bar))
    assert not bad, bad


@pytest.mark.parametrize("dims,n,n_nets", CASES)
def test_loss_backward_meets_the_oracle(dims, n, n_nets):
    ws, state, action, target, g64, loss64, q64 = case(dims, n, n_nets)
    critic = critic_of(dims, ws, gemm="fused")
    s, a, y = on_dev(state, action, target)
    (dg, dq, dl), (lg, lq, ll) = run_both(critic, s, a, y)
    assert N.last_kernel().startswith("k_marl_critic_grad_rows<%d,%d>x%d" % (dims[3] // 128, dims[4] // 128, n_nets))
    # every byte is written: everything was NaN before
    for t in [x for gs in dg for x in gs] + list(dq) + [dl]:
        assert bool(torch.isfinite(t).all())
    check_bars("%s x %d" % (dims, n), errors(dg, dq, dl, g64, loss64, q64), errors(lg, lq, ll, g64, loss64, q64))


@pytest.mark.parametrize("dims,n", [((40, 88, 160, 256, 128), 64), (DRIVER8, 256)])
def test_small_td_error(dims, n):
    """target = q64 + 1e-4 noise: the deltas are of order 1e-7 and smaller, below float16's normal range.  The case that
    fails if the deltas are split unscaled."""
    ws, state, action, target, g64, loss64, q64 = case(dims, n, 1, True)
    critic = critic_of(dims, ws, gemm="fused")
    s, a, y = on_dev(state, action, target)
    (dg, dq, dl), (lg, lq, ll) = run_both(critic, s, a, y)
    assert float(np.abs(q64[0] - target).max()) < 1e-3       # so |e| < 2e-3 / n: every delta is below float16's normal range
    check_bars("small TD %s x %d" % (dims, n), errors(dg, dq, dl, g64, loss64, q64), errors(lg, lq, ll, g64, loss64, q64))


def test_rows_beyond_n_are_not_read_and_calls_repeat_bit_for_bit():
    dims, n = (40, 88, 160, 256, 128), 33
    ws, state, action, target, *_ = case(dims, n, 2)
    critic = critic_of(dims, ws, gemm="fused")
    s, a, y = on_dev(state, action, target)
    big = [torch.full((64,) + tuple(t.shape[1:]), float("nan"), device=dev()) for t in (s, a, y)]
    for b, t in zip(big, (s, a, y)):
        b[:n] = t
    views = [b[:n] for b in big]
    assert all(v.is_contiguous() for v in views)

    def run(s_, a_, y_):
        grads, qs, loss = critic.alloc_grads(), tuple(torch.empty(n, 1, device=dev()) for _ in range(2)), torch.empty(1, device=dev())
        critic.loss_backward(s_, a_, y_, grads=grads, q=qs, loss=loss)
        return [t for gs in grads for t in gs] + list(qs) + [loss]
    clean, again, viewed = run(s, a, y), run(s, a, y), run(*views)
    for t, u, v in zip(clean, again, viewed):
        assert bool(torch.isfinite(t).all())
        assert torch.equal(t.view(torch.int32), u.view(torch.int32))          # determinism: identical bits
        assert torch.equal(t.view(torch.int32), v.view(torch.int32))          # the NaN rows beyond n were never read


def test_shared_weights_after_an_optimiser_step():
    """After `BatchedAdam.step` on shared parameters the next `loss_backward` matches the oracle on the UPDATED weights: the
    stale stream was rebuilt, and the in-place read of W2 / W3 sees the new weights."""
    dims, n = (20, 24, 96, 512, 256), 97
    ws, state, action, target, *_ = case(dims, n, 2)
    params = [[torch.from_numpy(w[k]).to(dev()) for k in G.KEYS] for w in ws]
    critic = BatchedTwinCritic(*dims, device=dev(), gemm="fused")
    critic.pack = "device"
    critic.share_state_dict(*(dict(zip(G.KEYS, ps)) for ps in params))
    s, a, y = on_dev(state, action, target)
    grads = critic.alloc_grads()
    critic.loss_backward(s, a, y, grads=grads)
    packs = critic.packs
    BatchedAdam(params, lr=1e-3, max_norm=1.0).step(grads=grads)
    new = [{k: p.cpu().numpy() for k, p in zip(G.KEYS, ps)} for ps in params]
    assert not np.array_equal(new[0]["fc2.weight"], ws[0]["fc2.weight"])
    new = [G.nudge_biases(w, (state, action))[0] for w in new]
    for ps, w in zip(params, new):                            # the nudged biases go back into the shared tensors
        for k, p in zip(G.KEYS, ps):
            if k.endswith("bias"):
                p.copy_(torch.from_numpy(w[k]))
    g64, loss64, q64 = G.loss_grads64(new, state, action, target)
    (dg, dq, dl), (lg, lq, ll) = run_both(critic, s, a, y)
    assert critic.packs == packs + 2
    check_bars("shared %s x %d" % (dims, n), errors(dg, dq, dl, g64, loss64, q64), errors(lg, lq, ll, g64, loss64, q64))


@pytest.mark.parametrize("dims,kw", [((40, 88, 160, 256, 128), dict(gemm="library")), ((80, 288, 96, 128, 128), dict(gemm="wide"))])
def test_library_modes_run_the_library_path(dims, kw):
    n = 33
    ws, state, action, target, g64, loss64, q64 = case(dims, n, 2)
    critic = critic_of(dims, ws, **kw)
    s, a, y = on_dev(state, action, target)
    before = N.last_kernel()
    (dg, dq, dl), (lg, lq, ll) = run_both(critic, s, a, y)
    assert N.last_kernel() == before                          # no launch of this library's
    check_bars("%s %s" % (kw["gemm"], dims), errors(dg, dq, dl, g64, loss64, q64), errors(lg, lq, ll, g64, loss64, q64))


def test_loss_backward_refuses_what_it_would_have_to_copy():
    dims, n = (5, 10, 32, 128, 128), 33
    ws, state, action, target, *_ = case(dims, n, 2)
    critic = critic_of(dims, ws, gemm="fused")
    s, a, y = on_dev(state, action, target)
    with pytest.raises(ValueError):
        critic.loss_backward(s, a, y.double())
    with pytest.raises(ValueError):
        critic.loss_backward(s, a, y[:-1])
    with pytest.raises(ValueError):
        critic.loss_backward(s, a, torch.stack([y, y], 1)[:, 0])          # not contiguous
    with pytest.raises(ValueError):
        critic.loss_backward(s.cpu(), a, y)
    with pytest.raises(ValueError):
        critic.loss_backward(s, a, y, grads=critic.alloc_grads()[:1])
    with pytest.raises(ValueError):
        critic.loss_backward(s, a, y, workspace=torch.empty(64, dtype=torch.uint8, device=dev()))      # too small
    with pytest.raises(ValueError):
        critic.loss_backward(s, a, y, loss=torch.empty(2, device=dev()))
    # a caller's workspace of the stated size is used; the cached one grows on demand
    need = N.load().risvec_marl_critic_grad_workspace(n, *dims, 2)
    critic.loss_backward(s, a, y.view(n, 1), workspace=torch.empty(need, dtype=torch.uint8, device=dev()))
    critic.loss_backward(s[:1], a[:1], y[:1])
    small = critic._grad_workspace.numel()
    critic.loss_backward(s, a, y)
    assert critic._grad_workspace.numel() == need > small
