"""For test_marl_critic_grad_walk_host.py, and for whoever reads a failure of test_marl_critic_grad_sweep_hip.py: a NumPy
walk of the ARITHMETIC of `risvec_marl_critic_grad` (csrc/k_marl_critic_grad.hip) -- every scale, split, product, un-scale, mask and rounding the two
launches make, in the order they make them, as whole matrices: not the lane layout, not the order of the MFMA's own sums.
The three partial products of a split product are summed in float64, as `walk_stream` of marl_critic_ref.py does: the MFMA's
float32 accumulation is what the GPU tests measure.  What the walk gives is therefore what the scaled-split scheme can
deliver at an input; if the walk meets a bar and the kernel does not, the kernel is wrong, and the stage can be found by
comparing the workspace with `info` below.

Beside it `loss_grads32`, the same backprop in plain float32 NumPy with no split: the stand-in for the library path
(`loss_backward_torch`) where no GPU is present.

A plain module: no fixtures, no test collection."""
import numpy as np

from tests.marl_critic_grad_ref import KEYS, LAYERS

GRAD_SCALE_CLAMP = 80            # kGradScaleClamp
F32 = np.float32


def grad_scale_exp(amax):
    """`grad_scale_exp`: s with amax 2^s in [64, 128), from frexpf of max(amax, 1e-30f), clamped to +-80"""
    _, ex = np.frexp(np.maximum(F32(amax), F32(1e-30)))
    return int(min(max(7 - int(ex), -GRAD_SCALE_CLAMP), GRAD_SCALE_CLAMP))


def _pow2(s):
    return np.ldexp(F32(1.0), int(s))                         # float32, exact for |s| <= 126


class _Operands:
    """Every float16 operand the walk forms goes through `split`: the largest |hi| per name, and whether all were finite"""

    def __init__(self):
        self.top, self.finite = {}, True

    def split(self, name, v):
        """`split16`: hi = fp16(v), lo = fp16(v - hi), both as float64"""
        v = np.asarray(v)
        assert v.dtype == np.float32, name
        with np.errstate(over="ignore", invalid="ignore"):
            hi = v.astype(np.float16)
            lo = (v - hi.astype(np.float32)).astype(np.float16)
        self.finite = self.finite and bool(np.isfinite(hi).all() and np.isfinite(lo).all())
        self.top[name] = max(self.top.get(name, 0.0), float(np.abs(hi.astype(np.float64)).max()))
        return hi.astype(np.float64), lo.astype(np.float64)


def _mfma3(ah, al, bh, bl):
    """hi.hi + lo.hi + hi.lo of A [M, K] and B [K, N], in float64"""
    return ah @ bh + al @ bh + ah @ bl


def scaled_weight(W):
    """(W 2^s in float32 with its largest entry in [64, 128), 2^-s in float32): the matrix the forward stream holds and the
    `scales` entry beside it; the transposed products of the row launch re-form the same matrix as W * (1 / scale)."""
    W = np.asarray(W, np.float32)
    amax = np.maximum(np.abs(W).max(), F32(1e-30))
    _, ex = np.frexp(amax)
    s = int(min(max(7 - int(ex), -40), 40))
    return W * _pow2(s), _pow2(-s)


def walk_net(w, state, action, target, ops=None):
    """One net through both launches.  -> ({key: gradient, float32, shaped as the weight}, sum_b diff^2 in float64,
    q [n] float32, info).  info: "e" [n], "d1" "d2" "d3" [F, npad] as the workspace holds them, "tmax" [3, tiles] (layer 1,
    2, 3), "s_tile" [2, tiles] (s3, s2 of every tile), "s_layer" [3], "operands": the `_Operands` record."""
    ops = ops or _Operands()
    n = len(state)
    x = np.concatenate([np.asarray(state, np.float32).reshape(n, -1), np.asarray(action, np.float32).reshape(n, -1)], 1)
    y = np.asarray(target, np.float32).reshape(n)
    npad = (n + 31) // 32 * 32
    ntiles = npad // 32
    b = {k: np.asarray(w[k + ".bias"], np.float32) for k in LAYERS}
    Ws, u = {}, {}
    for k in LAYERS:
        Ws[k], u[k] = scaled_weight(w[k + ".weight"])
    Wsplit = {k: ops.split(k + ".weight 2^s", Ws[k]) for k in LAYERS}           # [out, in]

    # ---- the forward: A = weights (rows = output features), B = activations (columns = rows of the batch)
    acts = [np.ascontiguousarray(x.T)]                        # feature-major, as the workspace: x, h1, h2, h3
    for k in LAYERS:
        ah, al = Wsplit[k]
        bh, bl = ops.split("input of " + k, acts[-1])
        z = _mfma3(ah, al, bh, bl) * float(u[k]) + b[k].astype(np.float64)[:, None]
        acts.append(np.maximum(z, 0.0).astype(np.float32))
    h3 = acts[3]
    qw = np.asarray(w["q.weight"], np.float32).reshape(-1)
    q = ((h3.astype(np.float64) * qw.astype(np.float64)[:, None]).sum(0) + float(np.asarray(w["q.bias"]).reshape(-1)[0])).astype(np.float32)

    # ---- the row launch: e, d3 in float32; per tile d2 and d1 through the scaled split product
    diff = (q - y).astype(np.float32)
    e = (diff * (F32(2.0) / F32(n))).astype(np.float32)

    def padded(v):                                            # rows >= n of the last tile carry e = 0, so every delta 0
        out = np.zeros(v.shape[:-1] + (npad,), np.float32)
        out[..., :n] = v
        return out
    hp = [padded(a) for a in acts]                            # their activations never meet a non-zero delta
    d3 = np.where(hp[3] > 0, qw[:, None] * padded(e)[None, :], F32(0.0)).astype(np.float32)
    d2 = np.zeros_like(hp[2])
    d1 = np.zeros_like(hp[1])
    tmax = np.zeros((3, ntiles), np.float32)
    s_tile = np.zeros((2, ntiles), int)
    W3h, W3l = (m.T for m in Wsplit["fc3"])                   # read transposed: [fc2, fc3]
    W2h, W2l = (m.T for m in Wsplit["fc2"])                   # [fc1, fc2]
    with np.errstate(over="ignore", under="ignore"):
        for t in range(ntiles):
            c = slice(32 * t, 32 * t + 32)
            m3 = np.abs(d3[:, c]).max()
            s3 = grad_scale_exp(m3)
            bh, bl = ops.split("d3 2^s (tile)", d3[:, c] * _pow2(s3))
            back = u["fc3"] * _pow2(-s3)
            v = (_mfma3(W3h, W3l, bh, bl) * float(back)).astype(np.float32)
            d2[:, c] = np.where(hp[2][:, c] > 0, v, F32(0.0))
            m2 = np.abs(d2[:, c]).max()
            s2 = grad_scale_exp(m2)
            bh, bl = ops.split("d2 2^s (tile)", d2[:, c] * _pow2(s2))
            back = u["fc2"] * _pow2(-s2)
            v = (_mfma3(W2h, W2l, bh, bl) * float(back)).astype(np.float32)
            d1[:, c] = np.where(hp[1][:, c] > 0, v, F32(0.0))
            tmax[:, t] = np.abs(d1[:, c]).max(), m2, m3
            s_tile[:, t] = s3, s2

        # ---- the weight launch: one exponent per layer from the tiles' maxima; d 2^s split, the activation split unscaled
        g = {}
        s_layer = []
        for l, (k, d) in enumerate(zip(LAYERS, (d1, d2, d3))):
            sx = grad_scale_exp(tmax[l].max())
            s_layer.append(sx)
            ah, al = ops.split("d%d 2^s (layer)" % (l + 1), d * _pow2(sx))
            bh, bl = ops.split("input of " + k, hp[l])
            g[k + ".weight"] = (_mfma3(ah, al, bh.T, bl.T) * float(_pow2(-sx))).astype(np.float32)
            g[k + ".bias"] = d.astype(np.float64).sum(1).astype(np.float32)
    e64 = padded(e).astype(np.float64)
    g["q.weight"] = (hp[3].astype(np.float64) * e64[None, :]).sum(1).astype(np.float32)[None, :]
    g["q.bias"] = np.array([e64.sum()]).astype(np.float32)
    info = {"e": e, "d1": d1, "d2": d2, "d3": d3, "tmax": tmax, "s_tile": s_tile, "s_layer": s_layer, "operands": ops}
    return {k: g[k] for k in KEYS}, float((diff.astype(np.float64) ** 2).sum()), q, info


def walk_loss_grads(ws, state, action, target):
    """Every net: (list of {key: gradient}, loss [float32: the nets' float64 sums added, divided by n, rounded once], list of
    q [n], list of info).  All nets share one `_Operands` record (info["operands"])."""
    ops = _Operands()
    out = [walk_net(w, state, action, target, ops) for w in ws]
    loss = F32(sum(o[1] for o in out) / float(len(state)))
    return [o[0] for o in out], loss, [o[2] for o in out], [o[3] for o in out]


def loss_grads32(ws, state, action, target):
    """The backprop of marl_critic_grad_ref.py in plain float32 NumPy, no split and no scaling: (list of {key: gradient},
    loss, list of q [n])"""
    n = len(state)
    x = np.concatenate([np.asarray(state, np.float32).reshape(n, -1), np.asarray(action, np.float32).reshape(n, -1)], 1)
    y = np.asarray(target, np.float32).reshape(n)
    grads, qs, loss = [], [], F32(0.0)
    for w in ws:
        w = {k: np.asarray(v, np.float32) for k, v in w.items()}
        hs = [x]
        for k in LAYERS:
            hs.append(np.maximum(hs[-1] @ w[k + ".weight"].T + w[k + ".bias"], F32(0.0)))
        q = (hs[3] @ w["q.weight"].T + w["q.bias"])[:, 0]
        diff = q - y
        e = diff * (F32(2.0) / F32(n))
        g = {"q.weight": (e[:, None] * hs[3]).sum(0)[None, :], "q.bias": np.array([e.sum()], np.float32)}
        d = (e[:, None] * w["q.weight"].reshape(1, -1)) * (hs[3] > 0)
        for l in (2, 1, 0):
            k = LAYERS[l]
            g[k + ".weight"] = d.T @ hs[l]
            g[k + ".bias"] = d.sum(0)
            if l:
                d = (d @ w[k + ".weight"]) * (hs[l] > 0)
        assert all(v.dtype == np.float32 for v in g.values())
        grads.append({k: g[k] for k in KEYS})
        qs.append(q)
        loss = loss + (diff * diff).mean(dtype=np.float32)
    return grads, F32(loss), qs
