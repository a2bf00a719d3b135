"""The inputs of the `loss_backward` sweep, shared by test_marl_critic_grad_sweep_hip.py (the kernels against float64) and
test_marl_critic_grad_walk_host.py (the NumPy walk of the kernels' arithmetic against float64, at these very inputs, without a
GPU): every shape of `MARL_CRITIC` (tests/mlp_sweep_shapes.py) at `CRITIC_ROWS` rows -- the GPU file names the edge each
brings to the backward -- and the value edges.  Every weight set went through `nudge_biases`; every builder is computed once
and its arrays are not modified.

A plain module: no fixtures, no test collection."""
import functools
from typing import NamedTuple

import numpy as np

from tests import marl_critic_grad_ref as G
from tests import mlp_sweep_shapes as SW

SMALL = (5, 10, 32, 128, 128)        # the smallest shape the kernel supports with a real input
MID = (40, 88, 160, 256, 128)
DISTINCT = 64                        # distinct rows of a tiled batch


class Inputs(NamedTuple):
    dims: tuple
    ws: list                 # nudged weight sets under the reference's key names, float32
    state: np.ndarray
    action: np.ndarray
    target: np.ndarray       # [n] float32
    g64: list                # the float64 oracle of marl_critic_grad_ref.py at these inputs
    loss64: float
    q64: list


def finish(dims, ws, state, action, target):
    target = np.asarray(target, np.float32)
    g64, loss64, q64 = G.loss_grads64(ws, state, action, target)
    return Inputs(dims, ws, state, action, target, g64, loss64, q64)


def with_target(inp, target):
    """`inp` with another target and the oracle at it"""
    return finish(inp.dims, inp.ws, inp.state, inp.action, target)


def tile_rows(a, n):
    """The rows of `a` repeated to n rows"""
    return np.ascontiguousarray(np.tile(a, (-(-n // len(a)),) + (1,) * (a.ndim - 1))[:n])


def _nets(dims, n_nets, batch, edit=None, seed=41):
    ws = []
    for c in range(n_nets):
        w = G.random_net(dims, seed + c)
        if edit is not None:
            edit(w)
        ws.append(G.nudge_biases(w, batch)[0])
    return ws


@functools.lru_cache(maxsize=None)
def _base(dims, n, n_nets):
    """The recipe of `case` of test_marl_critic_grad_hip.py: (weight sets, state, action)"""
    state, action = G.random_batch(dims, n, 7, dims[0] // 5)
    return _nets(dims, n_nets, (state, action)), state, action


@functools.lru_cache(maxsize=None)
def _tiled(dims, n, n_nets):
    """DISTINCT distinct rows (nudged), tiled to n rows.  `nudge_biases` cannot clear thousands of independent rows of a 128-unit
    layer: with a tiled batch the ReLU masks repeat, the targets and so the gradients still differ row by row."""
    state, action = G.random_batch(dims, DISTINCT, 7, dims[0] // 5)
    ws = _nets(dims, n_nets, (state, action))
    return ws, tile_rows(state, n), tile_rows(action, n)


@functools.lru_cache(maxsize=None)
def sweep(index, n_nets):
    """Case `index` of MARL_CRITIC at CRITIC_ROWS rows, the sweep's seeds, target = normal(0, 1)"""
    dims, n = SW.MARL_CRITIC[index].dims, SW.CRITIC_ROWS
    w_seed, b_seed = SW.seeds("marl", index)
    state, action = G.random_batch(dims, n, b_seed)
    ws = _nets(dims, n_nets, (state, action), seed=w_seed)
    return finish(dims, ws, state, action, np.random.default_rng(b_seed + 2).normal(0, 1, n))


def _around_q(ws, state, action, scale, seed=9):
    """q64 of net 1 + scale [n] x normal noise"""
    n = len(state)
    return G.critic_q64(ws[0], state, action) + np.asarray(scale, np.float64) * np.random.default_rng(seed).normal(0, 1, n)


@functools.lru_cache(maxsize=None)
def mixed_tiles(reverse):
    """Two tiles whose TD errors lie nine decimal orders apart: launch 1 scales per tile, launch 2 once per layer"""
    ws, state, action = _base(MID, 64, 1)
    s = np.where(np.arange(64) < 32, 1e-6, 1e3)
    return finish(MID, ws, state, action, _around_q(ws, state, action, s[::-1] if reverse else s))


@functools.lru_cache(maxsize=None)
def large_td():
    """Every exponent negative"""
    ws, state, action = _base(MID, 64, 1)
    return finish(MID, ws, state, action, 1e6 * np.random.default_rng(9).normal(0, 1, 64))


MANY_ROWS = 2060                     # 65 tiles, the last with 12 rows: the second trip of launch 2's loop over the tiles' maxima


@functools.lru_cache(maxsize=None)
def many_tiles(head_large):
    """The TD error 1e5 x larger in tile 64 (rows 2048 ..) than elsewhere -- the layer's scale overflows float16 there if tile
    64 is left out of the maximum -- or in tile 0 (the mirror image).  Row 2048 is row 0 again, the all-zero row: a large TD
    error on that row ALONE is ill-conditioned for d fc1.weight in any float32 arithmetic, so the whole tail tile has it."""
    n = MANY_ROWS
    ws, state, action = _tiled(SMALL, n, 1)
    r = np.arange(n)
    s = np.where(r < 32, 1e2, 1e-3) if head_large else np.where(r < 2048, 1e-3, 1e2)
    return finish(SMALL, ws, state, action, _around_q(ws, state, action, s))


@functools.lru_cache(maxsize=None)
def auto_range(n):
    """A tiled batch of n rows with plain targets, both nets"""
    ws, state, action = _tiled(SMALL, n, 2)
    return finish(SMALL, ws, state, action, np.random.default_rng(9).normal(0, 1, n))


@functools.lru_cache(maxsize=None)
def plain_small(n_nets):
    """SMALL x 33 with a plain target: what the zero-TD tests start from"""
    ws, state, action = _base(SMALL, 33, n_nets)
    return finish(SMALL, ws, state, action, np.random.default_rng(9).normal(0, 1, 33))


DEAD_BIAS = np.float32(-1e3)
DEAD_UNITS = 64


@functools.lru_cache(maxsize=None)
def dead_layer(which):
    """"fc3": fc3.bias = -1e3, every h3 is 0; "fc2": fc2.bias[:64] = -1e3, those 64 units are dead on every row.  The bias is
    set BEFORE `nudge_biases`, whose guard is relative to the layer's largest |z|: with 1e3 in the layer it moves every live
    unit of that layer at least 0.1 above the kink."""
    state, action = G.random_batch(SMALL, 33, 7, 1)

    def edit(w):
        if which == "fc3":
            w["fc3.bias"][:] = DEAD_BIAS
        else:
            w["fc2.bias"][:DEAD_UNITS] = DEAD_BIAS
    ws = _nets(SMALL, 1, (state, action), edit)
    return finish(SMALL, ws, state, action, np.random.default_rng(9).normal(0, 1, 33))


#: name -> builder of every input whose target is fixed beforehand (the zero-TD targets come from a first call)
ALL = {"sweep-%s-x%d" % (SW.case_id(SW.MARL_CRITIC[i]), k): functools.partial(sweep, i, k) for i, k in SW.MARL_CRITIC_RUNS}
ALL.update({
    "mixed-small-first": functools.partial(mixed_tiles, False), "mixed-large-first": functools.partial(mixed_tiles, True),
    "large-td": large_td,
    "many-tiles-tail-large": functools.partial(many_tiles, False), "many-tiles-head-large": functools.partial(many_tiles, True),
    "auto-4096": functools.partial(auto_range, 4096), "auto-4097": functools.partial(auto_range, 4097),
    "plain-small-x1": functools.partial(plain_small, 1), "plain-small-x2": functools.partial(plain_small, 2),
    "dead-fc3": functools.partial(dead_layer, "fc3"), "dead-fc2-units": functools.partial(dead_layer, "fc2"),
})
