"""Shared by test_marl_critic_host.py and test_marl_critic_hip.py: a float64 restatement of the reference's
`CriticNetwork.forward` (Simulation-MARL-BCD/networks.py:38-49) and of the TD target of `global_learn`
(global_sac_critic.py:339-352) in NumPy, the fixtures (loaded once), random weight sets under the reference's key names,
and a NumPy walk of the packed weight stream through the kernel's data flow.  The error measure and its two bars are
those of sarl_critic_ref.py, imported and not restated."""
import numpy as np

from tests.sarl_critic_ref import BAR, _mfma3, _split, _tab, _to_regs, err, fixture, fused_bar  # noqa: F401

FIXTURES = ("marl_critic_8", "marl_critic_4")
KEYS = tuple(p + s for p in ("fc1.", "fc2.", "fc3.", "q.") for s in ("weight", "bias"))


def weights_of(fx, net):
    """The weights of net 1 or 2 of a fixture under the reference's key names."""
    prefix = "n%d." % net
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


def _lin(x, w, name):
    return x @ np.asarray(w[name + ".weight"], np.float64).T + np.asarray(w[name + ".bias"], np.float64)


def critic_q64(w, state, action):
    """networks.py:38-49 in float64 -> q [n]"""
    n = len(state)
    x = np.concatenate([np.asarray(state, np.float64).reshape(n, -1), np.asarray(action, np.float64).reshape(n, -1)], 1)
    for name in ("fc1", "fc2", "fc3"):
        x = np.maximum(_lin(x, w, name), 0.0)
    return _lin(x, w, "q")[:, 0]


def td_target64(reward, q1, q2, done, gamma, coef=None, logp_power=None, logp_intent=None):
    """global_sac_critic.py:341-352 in float64: target = r + gamma (min(q1, q2) - c0 lp - c1 li); target[done] = r[done].
    q2 None: one net.  An absent logp is an absent term."""
    m = np.asarray(q1, np.float64).reshape(-1)
    if q2 is not None:
        m = np.minimum(m, np.asarray(q2, np.float64).reshape(-1))
    ent = np.zeros_like(m)
    if logp_power is not None:
        ent = ent + float(coef[0]) * np.asarray(logp_power, np.float64).reshape(-1)
    if logp_intent is not None:
        ent = ent + float(coef[1]) * np.asarray(logp_intent, np.float64).reshape(-1)
    r = np.asarray(reward, np.float64)
    return np.where(np.asarray(done, bool), r, r + float(gamma) * (m - ent))


def y_bound(reward, q1, q2, gamma, coef=None, logp_power=None, logp_intent=None):
    """2^-22 (|r| + |gamma| (|m| + |c0 lp| + |c1 li|)) per row: at most four float32 roundings on terms no larger than
    that sum"""
    m = np.asarray(q1, np.float64).reshape(-1)
    if q2 is not None:
        m = np.minimum(m, np.asarray(q2, np.float64).reshape(-1))
    s = np.abs(m)
    if logp_power is not None:
        s = s + np.abs(float(coef[0]) * np.asarray(logp_power, np.float64).reshape(-1))
    if logp_intent is not None:
        s = s + np.abs(float(coef[1]) * np.asarray(logp_intent, np.float64).reshape(-1))
    return 2.0 ** -22 * (np.abs(np.asarray(reward, np.float64)) + abs(float(gamma)) * s)


def random_net(dims, seed, q_range=0.4):
    """A weight set under the reference's key names at nn.Linear's default ranges (1 / sqrt(fan_in), networks.py:29-32),
    float32; q widened to +-q_range.  dims = (S, A, fc1, fc2, fc3)."""
    S, A, F1, F2, F3 = dims
    rng = np.random.default_rng(seed)
    u = lambda r, *s: rng.uniform(-r, r, s).astype(np.float32)     # noqa: E731
    IN = S + A
    return {"fc1.weight": u(IN ** -0.5, F1, IN), "fc1.bias": u(IN ** -0.5, F1), "fc2.weight": u(F1 ** -0.5, F2, F1),
            "fc2.bias": u(F1 ** -0.5, F2), "fc3.weight": u(F2 ** -0.5, F3, F2), "fc3.bias": u(F2 ** -0.5, F3),
            "q.weight": u(q_range, 1, F3), "q.bias": u(q_range, 1)}


def random_batch(dims, n, seed, V=None, zero_row0=True):
    """(state [n, S] in [0, 1.2]; action [n, A]: with V per agent a one-hot of width V, then two powers in (0, 1), as the
    learner's next_actions; without V uniform in (0, 1)), float32"""
    S, A = dims[0], dims[1]
    rng = np.random.default_rng(seed)
    state = rng.uniform(0, 1.2, (n, S)).astype(np.float32)
    if V is not None and A == V * (V + 2):
        action = np.zeros((n, V, V + 2), np.float32)
        action[np.arange(n)[:, None], np.arange(V)[None, :], rng.integers(0, V, (n, V))] = 1.0
        action[:, :, V:] = rng.uniform(0.001, 0.999, (n, V, 2))
        action = action.reshape(n, A)
    else:
        action = rng.uniform(0, 1, (n, A)).astype(np.float32)
    if zero_row0:
        state[0] = 0.0
        action[0] = 0.0
    return state, action


# ---------------------------------------------------------------------------------------------------------------------
# The kernel's data flow on the packed stream, in NumPy: fragments are addressed by the kernel's index rules
# (csrc/k_marl_critic.hip), activations are split into float16 hi + lo exactly as split16 does, the three partial
# products are summed (in float64: the MFMA's float32 accumulation is what the GPU tests measure).
def walk_stream(stream, scales, w, state, action, dims, geom):
    """q [n] as the kernel computes it from one net's packed `stream` [rows, 64, 8] float16 / `scales` [3] and the
    biases and q layer of `w` (reference key names)."""
    S_, A_, F1, F2, F3 = dims
    g = geom
    St = np.asarray(stream).astype(np.float64)
    u1, u2, u3 = (float(s) for s in np.asarray(scales))
    st = np.asarray(state, np.float32).reshape(len(state), -1)
    ac = np.asarray(action, np.float32).reshape(len(action), -1)
    n = len(st)
    lane = np.arange(64)
    out = np.zeros(n)

    def gemm(base, wave, nks, mt, sb):
        acc = [np.zeros((32, 32)) for _ in range(mt)]
        for s in range(nks):
            for m in range(mt):
                row = base + ((wave * nks + s) * mt + m) * 2
                acc[m] += _mfma3(St[row], St[row + 1], sb[s, 0], sb[s, 1])
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
        # the input staged from two pointers: k < S from state, S <= k < S + A from action, zero beyond
        k = 16 * np.arange(g.ks)[:, None, None] + 8 * (lane >> 5)[None, :, None] + np.arange(8)[None, None, :]
        rr = rows[lane & 31][None, :, None]
        v = np.where(k < S_, st[rr, np.minimum(k, S_ - 1)],
                     np.where(k < S_ + A_, ac[rr, np.clip(k - S_, 0, A_ - 1)], 0.0))
        hi, lo = _split(v)
        s_in = np.stack([hi, lo], 1)                              # [ks, 2, 64, 8]
        s_h = np.zeros((max(2 * g.ng, 8 * g.mt2), 2, 64, 8))
        for grp in range(g.ng):
            d = np.zeros((32, 32))
            for s in range(g.ks):
                row = g.fc1 + (grp * g.ks + s) * 2
                d += _mfma3(St[row], St[row + 1], s_in[s, 0], s_in[s, 1])
            put(s_h, grp, np.maximum(_to_regs(d) * u1 + _tab(w["fc1.bias"], 32 * grp), 0.0))
        acc = [gemm(g.fc2, wv, 2 * g.ng, g.mt2, s_h) for wv in range(4)]
        s_h = np.zeros_like(s_h)
        for wv in range(4):
            for m in range(g.mt2):
                t = wv * g.mt2 + m
                put(s_h, t, np.maximum(acc[wv][m] * u2 + _tab(w["fc2.bias"], 32 * t), 0.0))
        a3 = [gemm(g.fc3, wv, 8 * g.mt2, g.mt3, s_h) for wv in range(4)]
        q = np.zeros(64)
        for wv in range(4):
            for m in range(g.mt3):
                f0 = 32 * (wv * g.mt3 + m)
                y = np.maximum(a3[wv][m] * u3 + _tab(w["fc3.bias"], f0), 0.0)
                q += rowsum(y * _tab(np.asarray(w["q.weight"]).reshape(-1), f0))
        q = q[:32] + float(np.asarray(w["q.bias"]).reshape(-1)[0])
        m_ = e0 + np.arange(32) < n
        out[e0 + np.arange(32)[m_]] = q[m_]
    return out
