"""Shared by test_marl_critic_grad_host.py and test_marl_critic_grad_hip.py: a float64 restatement in NumPy, on top of
marl_critic_ref.py, of the critic loss of `global_learn` (Simulation-MARL-BCD/global_sac_critic.py:355-363) and of its
gradient with respect to every weight of a `CriticNetwork` (networks.py:38-49):

    x = [state | action]   z1 = fc1 x, h1 = relu z1   z2 = fc2 h1, h2 = relu z2   z3 = fc3 h2, h3 = relu z3   q = q(h3)
    e  = (2 / n) (q - y)
    loss = sum_c (1 / n) sum_b (q_c[b] - y[b])^2
    d3 = (e q.weight) * [h3 > 0]     d2 = (W3^T d3) * [h2 > 0]     d1 = (W2^T d2) * [h1 > 0]
    d q.weight = sum_b e h3     d q.bias = sum_b e     d fcl.weight = dl^T a(l-1)  (a0 = x)     d fcl.bias = sum_b dl

and `nudge_biases`, which moves every ReLU unit away from the kink so that the mask of a float32 computation is the
float64 one."""
import numpy as np

from tests.marl_critic_ref import KEYS, critic_q64, random_batch, random_net  # noqa: F401

LAYERS = ("fc1", "fc2", "fc3")


def _x64(state, action):
    n = len(state)
    return np.concatenate([np.asarray(state, np.float64).reshape(n, -1), np.asarray(action, np.float64).reshape(n, -1)], 1)


def forward64(w, x):
    """-> (pre-activations [z1, z2, z3], activations [x, h1, h2, h3], q [n])"""
    zs, hs = [], [x]
    for name in LAYERS:
        z = hs[-1] @ np.asarray(w[name + ".weight"], np.float64).T + np.asarray(w[name + ".bias"], np.float64)
        zs.append(z)
        hs.append(np.maximum(z, 0.0))
    q = hs[-1] @ np.asarray(w["q.weight"], np.float64).T + np.asarray(w["q.bias"], np.float64)
    return zs, hs, q[:, 0]


def grads64(w, state, action, target):
    """One net: ({key: gradient} under the reference's key names, its loss term, q [n])"""
    x = _x64(state, action)
    n = len(x)
    y = np.asarray(target, np.float64).reshape(n)
    zs, hs, q = forward64(w, x)
    e = (2.0 / n) * (q - y)
    g = {"q.weight": (e[:, None] * hs[3]).sum(0)[None, :], "q.bias": np.array([e.sum()])}
    d = (e[:, None] * np.asarray(w["q.weight"], np.float64).reshape(1, -1)) * (hs[3] > 0)
    for k in (2, 1, 0):
        name = LAYERS[k]
        g[name + ".weight"] = d.T @ hs[k]
        g[name + ".bias"] = d.sum(0)
        if k:
            d = (d @ np.asarray(w[name + ".weight"], np.float64)) * (hs[k] > 0)
    return {k: g[k] for k in KEYS}, float(((q - y) ** 2).mean()), q


def loss_grads64(ws, state, action, target):
    """Every net: (list of {key: gradient}, loss = the sum of the nets' terms, list of q [n])"""
    out = [grads64(w, state, action, target) for w in ws]
    return [o[0] for o in out], float(sum(o[1] for o in out)), [o[2] for o in out]


def nudge_biases(w, x, guard=1e-4, passes=20):
    """A ReLU unit whose float64 pre-activation is within rounding of 0 can take either mask in float32, and that changes
    a whole row of dW: no tolerance covers it.  Layer by layer: while any unit has |z| < guard max|z| of its layer on any
    row, add 4 guard max|z| to that unit's bias (at most `passes` passes); then ASSERT that no unit is left inside the
    guard -- a condition of every comparison that uses the result, not a measurement.  w: a weight set under the
    reference's key names (float32 arrays); x [n, S + A], or the pair (state, action).  -> (a new weight set, float32; the
    number of units nudged, counted once each).  The guard is 5 x the forward's own bar of 2e-5."""
    if isinstance(x, tuple):
        x = _x64(*x)
    x = np.asarray(x, np.float64)
    w = {k: np.array(v, np.float32) for k, v in w.items()}
    nudged = 0
    h = x
    for name in LAYERS:
        W = np.asarray(w[name + ".weight"], np.float64).T
        touched = np.zeros(W.shape[1], bool)
        for _ in range(passes):
            z = h @ W + np.asarray(w[name + ".bias"], np.float64)
            top = np.abs(z).max()
            close = (np.abs(z) < guard * top).any(0)
            if not close.any():
                break
            w[name + ".bias"][close] += np.float32(4 * guard * top)
            touched |= close
        z = h @ W + np.asarray(w[name + ".bias"], np.float64)
        assert not (np.abs(z) < guard * np.abs(z).max()).any(), "nudge_biases: %s still has a unit inside the guard" % name
        nudged += int(touched.sum())
        h = np.maximum(z, 0.0)
    return w, nudged


def rel_err(got, want):
    """max|g - g64| / max|g64| of one tensor (0 for an all-zero reference that is met exactly)"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    top = np.abs(want).max()
    d = np.abs(got - want).max()
    return 0.0 if d == 0.0 else d / top if top > 0 else np.inf
