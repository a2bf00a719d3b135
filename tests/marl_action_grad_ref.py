"""Shared by test_marl_action_grad_host.py and test_marl_action_grad_hip.py: a float64 restatement in NumPy, on
`marl_critic_grad_ref.forward64`, of the critic side of `centralized_actor_update` (Simulation-MARL-BCD/global_sac_critic.py:
174-176 and the backward() at :246) for `CriticNetwork`s (networks.py:38-49):

    x = [state | action]   h1, h2, h3, q_c = the forward of net c
    d3 = q.weight * [h3 > 0]     d2 = (W3^T d3) * [h2 > 0]     d1 = (W2^T d2) * [h1 > 0]
    g_c = (W1^T d1)[S : S + A]                                               = d q_c / d action, row by row
    w_1, w_2 = (1, 0) where q_1 < q_2, (0, 1) where q_1 > q_2, (0.5, 0.5) where q_1 == q_2        torch.min's backward
    out = scale (w_1 g_1 + w_2 g_2)        q_min = min(q_1, q_2)                                  one net: out = scale g_1

and the input recipe.  Two CONDITIONS of every comparison that uses these inputs are asserted here, on the oracle alone:
`nudge_biases` leaves no ReLU unit inside its guard, and on every row that is not a planted tie |q_1 - q_2| >= SEPARATION x
max|q|, so that a float32 computation selects the net the float64 one selects.  With under 100 rows a violation of the second
is a roughly 1 % event: `inputs` then moves on to the next seed pair (+ SEED_STEP), it never loosens the guard.

A plain module: no fixtures, no test collection.  Every builder is computed once and its arrays are not modified."""
import functools
from typing import NamedTuple

import numpy as np

from tests import marl_critic_grad_ref as G

SEPARATION = 1e-4
SEED_STEP = 1000
SEED_TRIES = 8
FLOOR = 2.0 ** -22                   # one split product's rounding: below it the ratio to the library's error means nothing


def action_grad64(ws, state, action, scale=1.0):
    """-> (out [n, A], q_min [n], [q_c [n]], [g_c [n, A]]), float64"""
    x = G._x64(state, action)
    A = np.asarray(action).reshape(len(x), -1).shape[1]
    S = x.shape[1] - A
    qs, gs = [], []
    for w in ws:
        _, hs, q = G.forward64(w, x)
        d = np.asarray(w["q.weight"], np.float64).reshape(1, -1) * (hs[3] > 0)
        for k in (2, 1):
            d = (d @ np.asarray(w[G.LAYERS[k] + ".weight"], np.float64)) * (hs[k] > 0)
        gs.append((d @ np.asarray(w["fc1.weight"], np.float64))[:, S:])
        qs.append(q)
    if len(ws) == 1:
        return float(scale) * gs[0], qs[0].copy(), qs, gs
    w1 = np.where(qs[0] < qs[1], 1.0, np.where(qs[0] > qs[1], 0.0, 0.5))[:, None]
    return float(scale) * (w1 * gs[0] + (1.0 - w1) * gs[1]), np.minimum(qs[0], qs[1]), qs, gs


def separated(qs, rows=None):
    """|q_1 - q_2| >= SEPARATION max|q| on every row of `rows` (default: all)"""
    q1, q2 = (np.asarray(q)[slice(None) if rows is None else rows] for q in qs)
    return bool((np.abs(q1 - q2) >= SEPARATION * max(np.abs(qs[0]).max(), np.abs(qs[1]).max())).all())


class Inputs(NamedTuple):
    dims: tuple
    ws: list                 # nudged weight sets under the reference's key names, float32
    state: np.ndarray
    action: np.ndarray
    out64: np.ndarray        # the oracle at scale = 1
    q_min64: np.ndarray
    q64: list
    g64: list
    seeds: tuple             # the (weight, batch) seeds in use


def finish(dims, ws, state, action, seeds, tie_rows=None):
    """The oracle at these inputs, after the two conditions were asserted"""
    for w in ws:
        assert G.nudge_biases(w, (state, action))[1] == 0, "a ReLU unit is inside the guard"
    out, q_min, qs, gs = action_grad64(ws, state, action)
    if len(ws) == 2:
        rows = None if tie_rows is None else ~tie_rows
        assert separated(qs, rows), "q_1 and q_2 come within %g max|q| of each other: take other seeds" % SEPARATION
        if len(state) >= 8:                                   # each net is selected somewhere: a select stuck on one net shows
            assert (qs[0] < qs[1]).any() and (qs[0] > qs[1]).any()
    return Inputs(dims, ws, state, action, out, q_min, qs, gs, seeds)


@functools.lru_cache(maxsize=None)
def inputs(dims, n, n_nets, w_seed, b_seed, V=None, q_scale=1.0):
    """n rows at `dims`: `random_net` at seeds w_seed + c, `random_batch` at b_seed (row 0 all zero where n > 1), every weight
    set nudged; the q layer multiplied by q_scale (a power of two, so q and every delta scale exactly) before that.  The first of the seed pairs (w_seed, b_seed) +
    k SEED_STEP, k < SEED_TRIES, whose oracle keeps the two q apart is the one in use.  With two nets and n > 1, net 2's
    q.bias is shifted so that both nets are selected (see below)."""
    for k in range(SEED_TRIES):
        ws_, bs_ = w_seed + k * SEED_STEP, b_seed + k * SEED_STEP
        state, action = G.random_batch(dims, n, bs_, V, zero_row0=n > 1)
        ws = []
        for c in range(n_nets):
            w = G.random_net(dims, ws_ + c)
            for key in ("q.weight", "q.bias"):
                w[key] = (w[key] * np.float32(q_scale)).astype(np.float32)
            ws.append(G.nudge_biases(w, (state, action))[0])
        if n_nets == 1:
            break
        # q is dominated by q.bias, and with two independent biases one net would be the smaller on every row: net 2's q.bias
        # is moved to the middle between the two central values of q_1 - q_2, so that each net is selected on half of the rows
        qs = action_grad64(ws, state, action)[2]
        d = np.sort(qs[0] - qs[1]) if n > 1 else np.zeros(2)
        ws[1]["q.bias"] = (ws[1]["q.bias"] + np.float32(0.5 * (d[n // 2 - 1] + d[n // 2]))).astype(np.float32)
        if separated(action_grad64(ws, state, action)[2]):
            break
    return finish(dims, ws, state, action, (ws_, bs_))


def _nudge_together(w1, w2, batch, passes=12):
    """Both nets share every bias: nudge one, hand its biases to the other, until neither moves"""
    for _ in range(passes):
        w1, a = G.nudge_biases(w1, batch)
        for k in G.KEYS:
            if k.endswith("bias"):
                w2[k] = w1[k].copy()
        w2, b = G.nudge_biases(w2, batch)
        for k in G.KEYS:
            if k.endswith("bias"):
                w1[k] = w2[k].copy()
        if a == 0 and b == 0:
            break
    return w1, w2


@functools.lru_cache(maxsize=None)
def tie_inputs(dims, n, w_seed, b_seed):
    """Two nets that differ ONLY in the action columns of fc1.weight -- net 2's are net 1's moved down one output feature, so
    the matrix keeps its largest entry and with it the power of two its weight stream is scaled by -- on a batch whose EVEN
    rows have an action of exactly 0: there x is the same for both nets' fc1 up to terms that are exactly 0, so q_1 == q_2 bit
    for bit in any arithmetic, while g_1 != g_2.  -> (Inputs, tie_rows [n] bool)"""
    S = dims[0]
    tie = np.arange(n) % 2 == 0
    for k in range(SEED_TRIES):
        ws_, bs_ = w_seed + k * SEED_STEP, b_seed + k * SEED_STEP
        state, action = G.random_batch(dims, n, bs_, zero_row0=False)
        action[tie] = 0.0
        w1 = G.random_net(dims, ws_)
        w2 = {key: v.copy() for key, v in w1.items()}
        w2["fc1.weight"][:, S:] = np.roll(w1["fc1.weight"][:, S:], 1, axis=0)
        w1, w2 = _nudge_together(w1, w2, (state, action))
        if separated(action_grad64([w1, w2], state, action)[2], ~tie):
            break
    for key in G.KEYS:
        assert np.array_equal(w1[key], w2[key]) == (key != "fc1.weight"), key
    assert np.array_equal(w1["fc1.weight"][:, :S], w2["fc1.weight"][:, :S])
    return finish(dims, [w1, w2], state, action, (ws_, bs_), tie), tie


def rel_err(got, want):
    return G.rel_err(got, want)
