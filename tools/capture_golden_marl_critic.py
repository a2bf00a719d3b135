#!/usr/bin/env python3
"""Capture golden vectors for the SAC twin global critic and its TD target (`BatchedTwinCritic`) from the REFERENCE.

    python tools/capture_golden_marl_critic.py <path to the reference checkout>      (or RISVEC_REFERENCE)

Imports the reference's own `Simulation-MARL-BCD/networks.CriticNetwork` (CPU torch) read-only and builds two of them
at reduced hidden sizes (the architecture is size-agnostic; small sizes keep the fixtures small).  The class creates its
checkpoint directory at construction, so an absolute temporary `chkpt_dir` is passed: nothing is written into the
checkout.  The statements of `Global_SAC_Critic.global_learn` that compute the target (`global_sac_critic.py`: from
`q1_next = ...` through the last assignment of `target`) are taken from the script's syntax tree and executed as they
stand on recorded inputs, once for the single-alpha and once for the separate-alpha branch -- the module itself is not
imported (it pulls in the driver's buffer).

With the reference's initialisation one critic is the minimum on 97-100 % of the rows (the q biases decide it), which
would leave `min` untested: both q layers are widened to +-0.4, net 2's q bias is then set so that the median of
q1 - q2 over the recorded rows is 0, and each net is asserted to be the minimum on 40-60 % of the rows.  Action rows are
shaped like the learner's `next_actions` (:326-333): per agent a one-hot of width V, then two powers in (0, 1).  A
quarter of the rows have `done` set.  Fixtures hold weights, inputs and outputs only.
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
    sys.exit("capture_golden_marl_critic: give the reference checkout (argument or RISVEC_REFERENCE)")
sys.dont_write_bytecode = True
sys.path.insert(0, REF_DIR)
import torch  # noqa: E402
import networks as REFNET  # noqa: E402  (the reference itself)

LEARNER = os.path.join(REF_DIR, "global_sac_critic.py")


def _stores(stmt):
    out = set()
    for n in ast.walk(stmt):
        if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store):
            out.add(n.id)
    return out


def target_statements():
    """`q1_next = ...` (inside its `with T.no_grad():`) through the last assignment of `target` in `global_learn`,
    compiled as they stand."""
    tree = ast.parse(open(LEARNER, encoding="utf-8").read(), filename=LEARNER)
    learn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "global_learn")
    body = learn.body
    first = next(k for k, s in enumerate(body) if isinstance(s, ast.With) and "q1_next" in _stores(s))
    last = max(k for k, s in enumerate(body) if isinstance(s, ast.Assign) and "target" in _stores(s))
    block = body[first:last + 1]
    inner = block[0].body
    assert isinstance(inner[0], ast.Assign) and "q1_next" in _stores(inner[0]), "the target statements changed in the reference"
    assert first < last and any(isinstance(s, ast.Assign) and isinstance(s.targets[0], ast.Subscript) for s in block), \
        "the target statements changed in the reference"
    return compile(ast.Module(body=block, type_ignores=[]), LEARNER, "exec")


TARGET = target_statements()


def capture(V, fc1, fc2, fc3, B, seed, chkpt_dir):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    n_states, n_actions = 5, V + 2                            # per agent
    S, A = V * n_states, V * n_actions
    nets = [REFNET.CriticNetwork(1e-3, n_states, fc1, fc2, fc3, V, A, name="global_target_critic%d" % c, agent_label="g",
                                 chkpt_dir=chkpt_dir) for c in (1, 2)]
    for net in nets:
        net.to("cpu")
        net.eval()
        with torch.no_grad():
            net.q.weight.uniform_(-0.4, 0.4)
            net.q.bias.uniform_(-0.4, 0.4)
    state_ = rng.uniform(0.0, 1.2, (B, S)).astype(np.float32)
    action_ = np.zeros((B, V, n_actions), np.float32)
    action_[np.arange(B)[:, None], np.arange(V)[None, :], rng.integers(0, V, (B, V))] = 1.0
    action_[:, :, V:] = rng.uniform(0.0, 1.0, (B, V, 2)).astype(np.float32).clip(1e-3, 1 - 1e-3)
    action_ = action_.reshape(B, A)
    logp_power = rng.uniform(-8.0, 4.0, (B, 1)).astype(np.float32)
    logp_intent = rng.uniform(-V * np.log(V), 0.0, (B, 1)).astype(np.float32)
    reward = rng.uniform(-6.0, 1.0, B).astype(np.float32)
    done = np.zeros(B, bool)
    done[rng.permutation(B)[:round(B / 4)]] = True
    gamma = 0.99
    st, ac = torch.from_numpy(state_), torch.from_numpy(action_)
    with torch.no_grad():
        diff = (nets[0].forward(st, ac) - nets[1].forward(st, ac)).view(-1)
        nets[1].q.bias += diff.median()                       # the median of q1 - q2 becomes 0
        q1, q2 = nets[0].forward(st, ac), nets[1].forward(st, ac)
    first = float((q1 < q2).float().mean())
    assert 0.4 <= first <= 0.6 and 0.4 <= float((q2 < q1).float().mean()) <= 0.6, "one critic is the minimum almost everywhere"
    assert float(q1.abs().max()) > 0.3 and float(q2.abs().max()) > 0.3, "q does not leave the neighbourhood of zero"
    log_alpha, log_alpha_c, log_alpha_d = (torch.tensor(v, dtype=torch.float32) for v in (-1.2, -0.7, -2.1))
    entropy_scale = 0.5
    out = {}
    for branch, separate in (("single", False), ("separate", True)):
        learner = types.SimpleNamespace(global_target_critic1=nets[0], global_target_critic2=nets[1], separate_alpha=separate,
                                        alpha=log_alpha.exp(), alpha_cont=log_alpha_c.exp(), alpha_disc=log_alpha_d.exp(),
                                        entropy_scale=entropy_scale, gamma=gamma)
        ns = dict(self=learner, T=torch, B=B, states_=st, next_actions=ac, next_logp_power_sum=torch.from_numpy(logp_power),
                  next_logp_int_sum=torch.from_numpy(logp_intent), rewards_g=torch.from_numpy(reward), done=torch.from_numpy(done))
        exec(TARGET, ns)
        target = ns["target"]
        assert tuple(target.shape) == (B, 1) and torch.equal(ns["q1_next"], q1) and torch.equal(ns["q2_next"], q2)
        assert torch.equal(target.view(-1)[ns["done"]], ns["rewards_g"][ns["done"]])
        out["target_" + branch] = target.detach().numpy().copy()
        a = (log_alpha.exp() * entropy_scale, log_alpha.exp() * entropy_scale) if not separate else \
            (log_alpha_c.exp() * entropy_scale, log_alpha_d.exp() * entropy_scale)
        out["coef_" + branch] = torch.stack(a).numpy().astype(np.float32)
    weights = {"n%d.%s" % (c + 1, k): v.numpy().copy() for c, net in enumerate(nets) for k, v in net.state_dict().items()}
    path = os.path.join(OUT_DIR, "marl_critic_%d.npz" % V)
    np.savez_compressed(path, V=V, S=S, A=A, fc1=fc1, fc2=fc2, fc3=fc3, B=B, state_=state_, action_=action_,
                        q1=q1.numpy(), q2=q2.numpy(), logp_power=logp_power, logp_intent=logp_intent, reward=reward, done=done,
                        gamma=np.float64(gamma), **out, **weights)
    print("marl_critic_%d: %d + %d -> %d -> %d -> %d -> 1 twice, batch %d (%d done), net 1 is the minimum on %.0f %%, %d bytes"
          % (V, S, A, fc1, fc2, fc3, B, int(done.sum()), 100 * first, os.path.getsize(path)))


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        capture(8, 64, 128, 128, 70, 41, os.path.join(tmp, "chkpt"))
        capture(4, 64, 128, 128, 33, 42, os.path.join(tmp, "chkpt"))
