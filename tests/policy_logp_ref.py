"""Shared by test_policy_sample_normal_host.py and test_policy_sample_normal_hip.py: a float64 restatement of the
reference's `PolicyNetwork.sample_normal` (Simulation-MARL-BCD/sac_agent.py:80-127, SAC below) in NumPy for one agent's
heads on a batch of rows, built on `oracle.policy_oracle.sample_heads` / `mask_logits`, and the bounds both test files
assert (the fixtures, loaded once, too).

    logp_power  = sum_i ( -eps_i^2 / 2 - log_std_i - log(2 pi) / 2 - log(1 - p_i^2 + 1e-6) )                (SAC:87-88)
    logp_intent = sum_k y_k lsm_k  (soft)   or   lsm[argmax y]  (hard),   lsm = log_softmax(masked logits)  (SAC:116-124)

The Normal term is written with the draw `eps`: (x_t - mu)^2 / (2 var) with x_t = mu + std eps IS eps^2 / 2 in exact
arithmetic.  The tanh correction is evaluated on p ROUNDED TO FLOAT32, because the tensor `power_action` the reference
squares is a float32 tensor: where the tanh saturates, 1 - p^2 is a difference of nearly equal numbers and the rounding
of p is the whole error.  What is left of that effect is one float32 rounding of 1 - p^2 + 1e-6 itself (2^-24 of a
value <= 1 + 1e-6, twice: the difference and the sum), i.e. a relative error of the logarithm's argument of up to
2^-23 / (1 - p^2 + 1e-6) and as much absolute error in the logarithm; `floor` is twice that, 2^-22 / (1 - p^2 + 1e-6)
per element, and the bound of logp_power carries the sum of its two floors."""
import functools
import os

import numpy as np

from oracle import policy_oracle as PO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("logp_policy_8", "logp_policy_4")
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
ABS = 2.0 ** -20            # absolute term of both log-prob bounds
REL = 1e-5                  # relative term on float32 heads taken as given
REL_DEVICE_HEADS = 2e-5     # ... where the heads come from the device forward (the policy tests allow 5e-6 on the heads)
FLOOR_CAP = 1e-4            # a fixture sample "saturates" above this floor
FLOOR_CAP_SHARE = 0.02      # at most this share of a fixture's samples may


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def agent_weights(fx, a):
    pre = "a%d." % a
    return {k[len(pre):]: v for k, v in fx.items() if k.startswith(pre)}


def sample_normal(mu, log_std, logits, mask, tau, eps, expo, hard=False):
    """SAC:80-127 on given head outputs [B, 2], [B, 2], [B, N] with the draws eps [B, 2] ~ N(0,1), expo [B, N] ~ Exp(1).
    -> dict(power [B,2], y [B,N], onehot [B,N], logp_power [B], logp_intent [B], floor [B,2])."""
    power, y, onehot = PO.sample_heads(mu, log_std, logits, mask, tau, eps, expo, hard)
    ls = np.clip(np.asarray(log_std, np.float64), -20.0, 2.0)
    e = np.asarray(eps, np.float64)
    p32 = power.astype(np.float32).astype(np.float64)
    arg = 1.0 - p32 * p32 + 1e-6
    logp_power = (-0.5 * e * e - ls - HALF_LOG_2PI - np.log(arg)).sum(-1)
    ml = PO.mask_logits(np.asarray(logits, np.float64), mask)
    sh = ml - ml.max(-1, keepdims=True)
    lsm = sh - np.log(np.exp(sh).sum(-1, keepdims=True))
    if hard:
        logp_intent = lsm[np.arange(len(lsm)), y.argmax(-1)]
    else:
        logp_intent = np.where(y == 0.0, 0.0, y * lsm).sum(-1)          # 0 * (finfo.min / 2 - ...) is 0
    return dict(power=power, y=y, onehot=onehot, logp_power=logp_power, logp_intent=logp_intent, floor=2.0 ** -22 / arg)


def bound_power(ref, floor, rel=REL):
    return rel * np.abs(ref) + ABS + np.asarray(floor).sum(-1)


def bound_intent(ref, rel=REL):
    return rel * np.abs(ref) + ABS


def batch(heads, mask, tau, hard, eps, expo):
    """`sample_normal` for every agent of host-made heads [V, B, 4+V] (mask [B,V,V] or None, tau / hard [V], eps
    [B,V,2], expo [B,V,V]) -> the same dict with every entry [B, V, ...], plus clear [B, V]: the arg-max is decided
    (top two soft probabilities further apart than 1e-4)."""
    V, B, _ = heads.shape
    h = np.asarray(heads, np.float64)
    outs = []
    clear = np.empty((B, V), bool)
    for a in range(V):
        m = None if mask is None else np.asarray(mask)[:, a].astype(np.float64)
        t = float(np.float32(tau[a]))
        args = (h[a][:, 0:2], h[a][:, 2:4], h[a][:, 4:], m, t, eps[:, a], expo[:, a])
        outs.append(sample_normal(*args, hard=bool(hard[a])))
        clear[:, a] = PO.top2_gap(PO.sample_heads(*args)[1]) > 1e-4
    r = {k: np.stack([o[k] for o in outs], axis=1) for k in outs[0]}
    r["clear"] = clear
    return r
