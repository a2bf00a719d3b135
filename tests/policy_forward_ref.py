"""Shared by test_policy_forward_host.py and test_policy_forward_hip.py: float64 restatements of the reference's
`PolicyNetwork.forward` (Simulation-MARL-BCD/sac_agent.py:62-78) cut where the library cuts it -- layer 1 alone, the heads
from a given fc2 product, and the whole forward -- on `oracle.policy_oracle.layer_norm`, the error measure of
test_policy_hip.py taken against float64, and the inputs of a sweep case built once.  The bars and the weight recipe are
imported from where they live (tests/sarl_critic_ref.py, tests/mlp_sweep_shapes.py through tests/policy_forward_shapes.py)."""
import functools

import numpy as np

from oracle.policy_oracle import layer_norm
from tests import policy_forward_shapes as PS
from tests.sarl_critic_ref import BAR, fused_bar  # noqa: F401  (re-exported: the bars of both test files)

HEAD_NAMES = ("mu", "log_std", "intent_logits")


def _w64(w):
    return {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}


def layer1_64(w, obs):
    """relu(LayerNorm(fc1 obs + b1)) -> [n, fc1]; obs [n, IN]"""
    W = _w64(w)
    x = np.asarray(obs, dtype=np.float64)
    return np.maximum(layer_norm(x @ W["fc1.weight"].T + W["fc1.bias"], W["bn1.weight"], W["bn1.bias"]), 0.0)


def heads_from_g64(w, g):
    """[n, 4 + V] = (mu, log_std unclamped, intent_logits) from g [n, fc2], the fc2 product WITHOUT its bias: the input
    contract of `risvec_policy_heads`, which adds fc2.bias itself"""
    W = _w64(w)
    x = np.maximum(layer_norm(np.asarray(g, dtype=np.float64) + W["fc2.bias"], W["bn2.weight"], W["bn2.bias"]), 0.0)
    return np.concatenate([x @ W[k + ".weight"].T + W[k + ".bias"] for k in HEAD_NAMES], axis=-1)


def forward64(w, obs):
    """(mu [n, 2], log_std [n, 2] unclamped, logits [n, V]) of one agent on obs [n, IN]"""
    W2 = np.asarray(w["fc2.weight"], dtype=np.float64)
    h = heads_from_g64(w, layer1_64(w, obs) @ W2.T)
    return h[:, 0:2], h[:, 2:4], h[:, 4:]


def heads64(w, obs):
    """`forward64` as the one [n, 4 + V] row `forward_heads` returns"""
    return np.concatenate(forward64(w, obs), axis=-1)


def err(got, ref64):
    """max over rows and outputs of |got - ref| / max(that row's max |ref|, 1e-3)"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    scale = np.maximum(np.abs(ref64).max(-1, keepdims=True), 1e-3)
    return float((np.abs(got - ref64) / scale).max())


class CaseData:
    """The inputs of one sweep case and their float64 references, per agent.  Built once and shared; never modified."""

    def __init__(self, kind, index):
        self.case = PS.case_of(kind, index)
        self.dims = self.case.dims
        IN, F1, F2, V = self.dims
        w_seed, b_seed = PS.seeds(kind, index)
        self.weights = PS.case_weights(kind, index)
        self.obs = PS.observations(self.dims, PS.ROWS, b_seed)                  # [n, V, IN]
        self.g = PS.random_g(self.dims, PS.ROWS, b_seed + 1)                    # [V, n, fc2]
        self.h1_64 = [layer1_64(self.weights[a], self.obs[:, a]) for a in range(V)]
        self.heads_64 = [heads_from_g64(self.weights[a], self.h1_64[a] @ np.asarray(self.weights[a]["fc2.weight"], np.float64).T)
                         for a in range(V)]
        self.heads_g_64 = [heads_from_g64(self.weights[a], self.g[a]) for a in range(V)]
        for t in (self.obs, self.g, *self.h1_64, *self.heads_64, *self.heads_g_64):
            t.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case_data(kind, index):
    return CaseData(kind, index)
