#!/usr/bin/env python3
"""Capture golden vectors for every agent's local twin target critics and local TD target (`BatchedLocalCritics`) from the
REFERENCE.

    python tools/capture_golden_local_critic.py <path to the reference checkout>      (or RISVEC_REFERENCE)

Imports the reference's own `Simulation-MARL-BCD/networks.CriticNetwork` (CPU torch) read-only and builds V x 2 of them
as `Agent.__init__` does (`sac_agent.py:169-182`: a local critic on obs (5) + action (V + 2)), at reduced hidden sizes.
The class creates its checkpoint directory at construction, so an absolute temporary `chkpt_dir` is passed: nothing is
written into the checkout.  The statements of `Agent.local_learn` that compute the target (`sac_agent.py`: from
`masked_logits_fw = ...` through `target = ...`, inside its `with T.no_grad():`) are taken from the script's syntax tree
and executed as they stand on recorded inputs, once per agent -- the module itself is not imported (it pulls in the
driver's buffer), and no sampling is replayed: what `policy.forward` and `policy.sample_normal` returned (`mu_fw`,
`logstd_fw`, `intent_logits_fw`, `next_power_actions`, the two log-probabilities) is recorded input.

As in capture_golden_marl_critic.py both q layers are widened to +-0.4 and net 2's q bias is set so that the median of
q1 - q2 over the recorded rows is 0; each net is asserted to be the minimum on 40-60 % of the rows, per agent.  On a third
of the rows the agent's own logit is the largest, so the replacement decides the one-hot.  A quarter of the rows have
`done` set.

V x 2 nets of random float32 weights do not fit a fixture of the size of marl_critic_8.npz, so the fc2 and fc3 weight
matrices are rounded to 4 levels across the range of the reference's initialisation (+-r (2 k + 1) / 4) before anything
is computed: still dense, and compressible.  fc1, the biases and the q layers stay as drawn.  Fixtures hold weights,
inputs and outputs only.
"""
from __future__ import annotations

import ast
import os
import sys
import tempfile
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("RISVEC_REFERENCE", "")
REF_DIR = os.path.join(REF, "Simulation-MARL-BCD")
OUT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
if not REF or not os.path.isfile(os.path.join(REF_DIR, "networks.py")):
    sys.exit("capture_golden_local_critic: give the reference checkout (argument or RISVEC_REFERENCE)")
sys.dont_write_bytecode = True
sys.path.insert(0, REF_DIR)
import torch  # noqa: E402
import networks as REFNET  # noqa: E402  (the reference itself)

AGENT = os.path.join(REF_DIR, "sac_agent.py")
LEVELS = 4


def _stores(stmt):
    out = set()
    for n in ast.walk(stmt):
        if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store):
            out.add(n.id)
    return out


def target_statements():
    """`masked_logits_fw = ...` through `target = ...` of the `with T.no_grad():` block of `local_learn`, compiled as they
    stand."""
    tree = ast.parse(open(AGENT, encoding="utf-8").read(), filename=AGENT)
    learn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "local_learn")
    block = next(s for s in learn.body if isinstance(s, ast.With) and "masked_logits_fw" in _stores(s)).body
    first = next(k for k, s in enumerate(block) if isinstance(s, ast.Assign) and "masked_logits_fw" in _stores(s))
    last = max(k for k, s in enumerate(block) if isinstance(s, ast.Assign) and "target" in _stores(s))
    stmts = block[first:last + 1]
    names = set().union(*(_stores(s) for s in stmts))
    assert first < last and {"idx", "next_intent_onehot", "q1_next", "q2_next", "min_q_next", "target"} <= names, \
        "the target statements changed in the reference"
    return compile(ast.Module(body=stmts, type_ignores=[]), AGENT, "exec")


TARGET = target_statements()


def quantise_(w):
    """Round a Linear weight to LEVELS levels across its initialisation range +-1 / sqrt(fan_in), in place."""
    r = w.shape[1] ** -0.5
    k = torch.clamp(torch.floor((w / r + 1.0) * (LEVELS / 2)), 0, LEVELS - 1)
    w.copy_(((2 * k + 1) / LEVELS - 1.0) * r)


def capture(V, fc1, fc2, fc3, B, seed, chkpt_dir):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    S, A = 5, V + 2
    obs_ = rng.uniform(0.0, 1.2, (B, V, S)).astype(np.float32)
    heads = np.zeros((V, B, 4 + V), np.float32)                # what the policy's forward returned: mu, log_std, logits
    heads[:, :, 0:2] = rng.normal(0.0, 0.5, (V, B, 2))
    heads[:, :, 2:4] = rng.uniform(-2.0, 0.5, (V, B, 2))
    heads[:, :, 4:] = rng.normal(0.0, 1.5, (V, B, V))
    own = rng.uniform(size=(V, B)) < 1 / 3
    for j in range(V):
        heads[j, own[j], 4 + j] = heads[j, own[j], 4:].max(-1) + 1.0
    power = np.tanh(rng.normal(0.0, 1.0, (B, V, 2))).astype(np.float32)
    logp_power = rng.uniform(-8.0, 4.0, (B, V)).astype(np.float32)
    logp_intent = rng.uniform(-np.log(V) - 2.0, 0.0, (B, V)).astype(np.float32)
    reward_l = rng.uniform(-6.0, 1.0, (B, V)).astype(np.float32)
    done = np.zeros(B, bool)
    done[rng.permutation(B)[:round(B / 4)]] = True
    gamma = 0.99
    coef = np.array([np.exp(-0.7) * 0.5, np.exp(-2.1) * 0.5], np.float32)     # alpha_c, alpha_d times the entropy scale
    out = {k: np.zeros((V, B), np.float32) for k in ("q1", "q2", "target")}
    idx_all = np.zeros((V, B), np.int64)
    weights, first_min = {}, []
    for j in range(V):
        nets = [REFNET.CriticNetwork(1e-3, S, fc1, fc2, fc3, V, action_dim=A, name="target_q%d" % c, agent_label=j,
                                     chkpt_dir=chkpt_dir) for c in (1, 2)]
        for net in nets:
            net.to("cpu")
            net.eval()
            assert net.fc1.in_features == S + A
            with torch.no_grad():
                net.q.weight.uniform_(-0.4, 0.4)
                net.q.bias.uniform_(-0.4, 0.4)
                quantise_(net.fc2.weight)
                quantise_(net.fc3.weight)
        agent = types.SimpleNamespace(agent_name=j, number_agents=V, target_q1=nets[0], target_q2=nets[1], gamma=gamma)

        def run():
            ns = dict(self=agent, T=torch, F=torch.nn.functional, intent_logits_fw=torch.from_numpy(heads[j, :, 4:].copy()),
                      next_power_actions=torch.from_numpy(power[:, j].copy()), states_=torch.from_numpy(obs_[:, j].copy()),
                      entropy_coeff_power=float(coef[0]), entropy_coeff_intent=float(coef[1]),
                      next_logp_power=torch.from_numpy(logp_power[:, j:j + 1].copy()),
                      next_logp_intent=torch.from_numpy(logp_intent[:, j:j + 1].copy()),
                      rewards=torch.from_numpy(reward_l[:, j:j + 1].copy()), done=torch.from_numpy(done))
            with torch.no_grad():
                exec(TARGET, ns)
            return ns
        with torch.no_grad():
            ns = run()
            nets[1].q.bias += (ns["q1_next"] - ns["q2_next"]).view(-1).median()      # the median of q1 - q2 becomes 0
            ns = run()
        q1, q2, target = ns["q1_next"], ns["q2_next"], ns["target"]
        assert tuple(target.shape) == (B, 1) and tuple(q1.shape) == (B, 1)
        first = float((q1 < q2).float().mean())
        assert 0.4 <= first <= 0.6 and 0.4 <= float((q2 < q1).float().mean()) <= 0.6, "one critic is the minimum almost everywhere"
        assert float(q1.abs().max()) > 0.1 and float(q2.abs().max()) > 0.1, "q does not leave the neighbourhood of zero"
        assert torch.equal(target.view(-1)[ns["done"]], ns["rewards"].view(-1)[ns["done"]])
        idx = ns["idx"].numpy()
        others = heads[j, :, 4:].copy()
        others[:, j] = -np.inf
        assert (idx != j).all() and np.array_equal(idx, others.argmax(-1))
        first_min.append(first)
        out["q1"][j], out["q2"][j], out["target"][j] = q1.view(-1).numpy(), q2.view(-1).numpy(), target.view(-1).numpy()
        idx_all[j] = idx
        for c, net in enumerate(nets):
            for k, v in net.state_dict().items():
                weights["a%d.n%d.%s" % (j, c + 1, k)] = v.numpy().copy()
    path = os.path.join(OUT_DIR, "local_critic_%d.npz" % V)
    np.savez_compressed(path, V=V, S=S, A=A, fc1=fc1, fc2=fc2, fc3=fc3, B=B, obs_=obs_, heads=heads, power=power,
                        logp_power=logp_power, logp_intent=logp_intent, reward_l=reward_l, done=done, gamma=np.float64(gamma),
                        coef=coef, idx=idx_all.astype(np.int8), **out, **weights)
    print("local_critic_%d: %d agents x 2 nets %d + %d -> %d -> %d -> %d -> 1, batch %d (%d done), own logit largest on %.0f %%, "
          "net 1 is the minimum on %.0f-%.0f %%, %d bytes"
          % (V, V, S, A, fc1, fc2, fc3, B, int(done.sum()), 100 * own.mean(), 100 * min(first_min), 100 * max(first_min),
             os.path.getsize(path)))


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        capture(8, 32, 128, 128, 33, 61, os.path.join(tmp, "chkpt"))
        capture(4, 32, 128, 128, 33, 62, os.path.join(tmp, "chkpt"))
