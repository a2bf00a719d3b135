"""Shared by test_sarl_critic_host.py and test_sarl_critic_hip.py: a float64 restatement of the reference's
`CriticNetwork.forward` (Simulation-SARL/networks.py:66-79), of `ActorNetwork.forward` (:132-141) and of the TD target
(ddpg_torch.py:84-88) in NumPy, the error measure of both files, the fixtures (loaded once), random weight sets under
the reference's key names, and a NumPy walk of the packed weight stream through the kernel's data flow."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 2e-5                                    # err < BAR in every mode (the project's bar, test_sarl_actor_hip.py)


def fused_bar(lib_err):
    """fused <= max(8 x the library mode's err on the same inputs, 1e-7)"""
    return max(8.0 * lib_err, 1e-7)


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def weights_of(fx, prefix="w."):
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


def layer_norm64(x, w, b):
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + 1e-5) * np.asarray(w, np.float64) + np.asarray(b, np.float64)


def _lin(x, w, name):
    return x @ np.asarray(w[name + ".weight"], np.float64).T + np.asarray(w[name + ".bias"], np.float64)


def critic_q64(w, state, action):
    """networks.py:66-79 in float64 -> q [n]"""
    x = np.asarray(state, np.float64).reshape(len(state), -1)
    s = np.maximum(layer_norm64(_lin(x, w, "fc1"), w["bn1.weight"], w["bn1.bias"]), 0.0)
    s = layer_norm64(_lin(s, w, "fc2"), w["bn2.weight"], w["bn2.bias"])
    h = np.maximum(s + _lin(np.asarray(action, np.float64), w, "action_value"), 0.0)
    h = np.maximum(layer_norm64(_lin(h, w, "fc3"), w["bn3.weight"], w["bn3.bias"]), 0.0)
    return _lin(h, w, "q")[:, 0]


def actor_mu64(w, state):
    """networks.py:132-141 in float64 -> mu [n, n_actions]"""
    x = np.asarray(state, np.float64).reshape(len(state), -1)
    h = np.maximum(layer_norm64(_lin(x, w, "fc1"), w["bn1.weight"], w["bn1.bias"]), 0.0)
    h = np.maximum(layer_norm64(_lin(h, w, "fc2"), w["bn2.weight"], w["bn2.bias"]), 0.0)
    return 1.0 / (1.0 + np.exp(-_lin(h, w, "mu")))


def td_target64(reward, q, done, gamma):
    """ddpg_torch.py:84-87: critic_value_[done] = 0; target = rewards + gamma critic_value_"""
    q = np.where(np.asarray(done, bool), 0.0, np.asarray(q, np.float64))
    return np.asarray(reward, np.float64) + float(gamma) * q


def err(got, want):
    """max over rows |q - q64| / max(max over the batch |q64|, 1e-3): the scale is batch-wide because a single q can
    cancel to near zero"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape and np.isfinite(got).all()
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-3))


def random_critic(dims, seed, q_range=0.4):
    """A weight set under the reference's key names at its init ranges (networks.py:40-58), float32; q widened to
    +-q_range and the LayerNorm parameters drawn in [0.5, 1.5] / +-0.2 as the fixtures do.  dims = (in, fc1, fc2, fc3,
    n_actions)."""
    IN, F1, F2, F3, A = dims
    rng = np.random.default_rng(seed)
    u = lambda r, *s: rng.uniform(-r, r, s).astype(np.float32)     # noqa: E731
    w = {"fc1.weight": u(F1 ** -0.5, F1, IN), "fc1.bias": u(F1 ** -0.5, F1), "fc2.weight": u(F2 ** -0.5, F2, F1),
         "fc2.bias": u(F2 ** -0.5, F2), "fc3.weight": u(F3 ** -0.5, F3, F2), "fc3.bias": u(F3 ** -0.5, F3),
         "action_value.weight": u(F2 ** -0.5, F2, A), "action_value.bias": u(F2 ** -0.5, F2),
         "q.weight": u(q_range, 1, F3), "q.bias": u(q_range, 1)}
    for i, f in ((1, F1), (2, F2), (3, F3)):
        w["bn%d.weight" % i] = rng.uniform(0.5, 1.5, f).astype(np.float32)
        w["bn%d.bias" % i] = u(0.2, f)
    return w


def random_batch(dims, n, seed, zero_row0=True):
    """(state [n, in] like observations: phases in [0, 2 pi) and scalars in [0, 1.2]; action [n, A], half in +-0.999 and
    half in (0, 1)), float32"""
    IN, A = dims[0], dims[4]
    rng = np.random.default_rng(seed)
    state = np.where(rng.uniform(size=(n, IN)) < 0.5, rng.uniform(0, 2 * np.pi, (n, IN)), rng.uniform(0, 1.2, (n, IN))).astype(np.float32)
    action = np.where((np.arange(n) % 2 == 0)[:, None], rng.uniform(-0.999, 0.999, (n, A)), rng.uniform(0, 1, (n, A))).astype(np.float32)
    if zero_row0:
        state[0] = 0.0
        action[0] = 0.0
    return state, action


# ---------------------------------------------------------------------------------------------------------------------
# The kernel's data flow on the packed stream, in NumPy: fragments are addressed by the kernel's index rules
# (csrc/k_sarl_critic.hip), activations are split into float16 hi + lo exactly as split16 does, the three partial
# products are summed (in float64: the MFMA's float32 accumulation is what the GPU tests measure).
def _split(v):
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    return hi.astype(np.float64), (v - hi.astype(np.float32)).astype(np.float16).astype(np.float64)


def _mfma3(ah, al, bh, bl):
    """A / B fragments [64 lanes, 8] -> D [32 M, 32 N]: lane = 32 h + (M or N), k = 8 h + j"""
    m = lambda f: f.reshape(2, 32, 8).transpose(1, 0, 2).reshape(32, 16)      # noqa: E731
    return m(ah) @ m(bh).T + m(al) @ m(bh).T + m(ah) @ m(bl).T


_Q = np.arange(16)
_CD_ROW = (_Q & 3) + 8 * (_Q >> 2)                # + 4 h: the feature of register q in a C/D tile


def _to_regs(D):
    """D [32 M, 32 N] -> y [64 lanes, 16 regs]: lane = 32 h + N holds rows (q & 3) + 8 (q >> 2) + 4 h"""
    return np.stack([D[_CD_ROW + 4 * h].T for h in range(2)], 0).reshape(64, 16)


def _tab(tab, base):
    """per-feature parameters in C/D register order -> [64 lanes, 16]"""
    t = np.asarray(tab, np.float64)
    return np.stack([np.broadcast_to(t[base + _CD_ROW + 4 * h], (32, 16)) for h in range(2)], 0).reshape(64, 16)


def walk_stream(stream, scales, w, state, action, dims, geom):
    """q [n] as the kernel computes it from the packed `stream` [rows, 64, 8] float16 / `scales` [4] and the small
    parameters of `w` (reference key names)."""
    IN, F1, F2, F3, A = dims
    g = geom
    S = np.asarray(stream).astype(np.float64)
    u1, u2, uav, u3 = (float(s) for s in np.asarray(scales))
    x = np.asarray(state, np.float32).reshape(len(state), -1)
    a = np.asarray(action, np.float32)
    n = len(x)
    lane = np.arange(64)
    out = np.zeros(n)

    def stage(src, W, ks, one, rows):
        k = 16 * np.arange(ks)[:, None, None] + 8 * (lane >> 5)[None, :, None] + np.arange(8)[None, None, :]
        v = np.where(k < W, src[rows[lane & 31]][np.arange(64)[None, :, None], np.minimum(k, W - 1)], (one & (k == W)) * 1.0)
        hi, lo = _split(v)
        return np.stack([hi, lo], 1)                              # [ks, 2, 64, 8]

    def gemm(base, wave, nks, mt, sb):
        acc = [np.zeros((32, 32)) for _ in range(mt)]
        for s in range(nks):
            for m in range(mt):
                row = base + ((wave * nks + s) * mt + m) * 2
                acc[m] += _mfma3(S[row], S[row + 1], sb[s, 0], sb[s, 1])
        return [_to_regs(d) for d in acc]

    def put(sh, tile, y):
        for u in range(2):
            hi, lo = _split(y[:, 8 * u:8 * u + 8])
            sh[2 * tile + u, 0], sh[2 * tile + u, 1] = hi, lo

    def rowsum(v):                                                # per row: both half-waves, as shfl_xor 32 does
        s = v.sum(-1)
        return (s[:32] + s[32:])[lane & 31]

    for e0 in range(0, n, 32):
        rows = np.where(e0 + np.arange(32) < n, e0 + np.arange(32), 0)
        s_in = stage(x, IN, g.ks, True, rows)
        s_a = stage(a, A, g.ksa, False, rows)
        av = [gemm(g.av, wv, g.ksa, g.mt2, s_a) for wv in range(4)]
        s_h = np.zeros((max(2 * g.ng, 8 * g.mt2), 2, 64, 8))
        raw, ss = {}, np.zeros(64)
        for grp in range(g.ng):
            d = np.zeros((32, 32))
            for s in range(g.ks):
                row = g.fc1 + (grp * g.ks + s) * 2
                d += _mfma3(S[row], S[row + 1], s_in[s, 0], s_in[s, 1])
            raw[grp] = _to_regs(d)
            ss += rowsum(raw[grp] ** 2)
        k1 = 1.0 / np.sqrt(ss * u1 * u1 / F1 + 1e-5) * u1
        for grp in range(g.ng):
            y = np.maximum(raw[grp] * k1[:, None] * _tab(w["bn1.weight"], 32 * grp) + _tab(w["bn1.bias"], 32 * grp), 0.0)
            put(s_h, grp, y)
        acc = [gemm(g.fc2, wv, 2 * g.ng, g.mt2, s_h) for wv in range(4)]
        for wv in range(4):
            for m in range(g.mt2):
                acc[wv][m] = acc[wv][m] * u2 + _tab(w["fc2.bias"], 32 * (wv * g.mt2 + m))
        mean = sum(rowsum(t) for wv in range(4) for t in acc[wv]) / F2
        var = sum(rowsum((t - mean[:, None]) ** 2) for wv in range(4) for t in acc[wv]) / F2
        rs = 1.0 / np.sqrt(var + 1e-5)
        s_h = np.zeros_like(s_h)
        for wv in range(4):
            for m in range(g.mt2):
                f0 = 32 * (wv * g.mt2 + m)
                y = (acc[wv][m] - mean[:, None]) * rs[:, None] * _tab(w["bn2.weight"], f0) + _tab(w["bn2.bias"], f0)
                y = y + av[wv][m] * uav + _tab(w["action_value.bias"], f0)
                put(s_h, wv * g.mt2 + m, np.maximum(y, 0.0))
        a3 = [gemm(g.fc3, wv, 8 * g.mt2, g.mt3, s_h) for wv in range(4)]
        for wv in range(4):
            for m in range(g.mt3):
                a3[wv][m] = a3[wv][m] * u3 + _tab(w["fc3.bias"], 32 * (wv * g.mt3 + m))
        mean = sum(rowsum(t) for wv in range(4) for t in a3[wv]) / F3
        var = sum(rowsum((t - mean[:, None]) ** 2) for wv in range(4) for t in a3[wv]) / F3
        rs = 1.0 / np.sqrt(var + 1e-5)
        q = np.zeros(64)
        for wv in range(4):
            for m in range(g.mt3):
                f0 = 32 * (wv * g.mt3 + m)
                y = np.maximum((a3[wv][m] - mean[:, None]) * rs[:, None] * _tab(w["bn3.weight"], f0) + _tab(w["bn3.bias"], f0), 0.0)
                q += rowsum(y * _tab(np.asarray(w["q.weight"]).reshape(-1), f0))
        q = q[:32] + float(np.asarray(w["q.bias"]).reshape(-1)[0])
        m_ = e0 + np.arange(32) < n
        out[e0 + np.arange(32)[m_]] = q[m_]
    return out
