#!/usr/bin/env python3
"""Capture golden vectors for the DDPG critic forward and TD target (`BatchedCritic`, `ddpg_td_target`) from the REFERENCE.

    python tools/capture_golden_critic.py <path to the reference checkout>      (or RISVEC_REFERENCE)

Imports the reference's own `Simulation-SARL/networks.CriticNetwork` / `ActorNetwork` (CPU torch) read-only and builds
them at reduced hidden sizes (the architecture is size-agnostic; small sizes keep the fixtures small).  The statements
of `Agent.learn` that compute the target (`ddpg_torch.py:80-88`: target actor, target critic, the critic's own forward,
the done mask, the target) are taken from the script's syntax tree and executed as they stand on recorded inputs --
`ddpg_torch.py` itself is not imported (it pulls in the driver's buffer and noise).  `q.weight` / `q.bias` are widened to
+-0.4 and the LayerNorm parameters drawn in [0.5, 1.5] / +-0.2: at the reference's own +-0.003 every q is about 0.03.
States are shaped like real observations (`ddpg_train.py:134-149`), half of the stored actions lie in +-0.999 (the
OU-noised, clipped actions of the buffer) and half in (0, 1) (a sigmoid head).  Fixtures hold weights, inputs and outputs
only.
"""
from __future__ import annotations

import ast
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("RISVEC_REFERENCE", "")
REF_DIR = os.path.join(REF, "Simulation-SARL")
OUT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
if not REF or not os.path.isfile(os.path.join(REF_DIR, "networks.py")):
    sys.exit("capture_golden_critic: give the reference checkout (argument or RISVEC_REFERENCE)")
sys.dont_write_bytecode = True
sys.path.insert(0, REF_DIR)
import torch  # noqa: E402
import networks as REFNET  # noqa: E402  (the reference itself)

AGENT = os.path.join(REF_DIR, "ddpg_torch.py")


def _stores(stmt):
    out = set()
    for n in ast.walk(stmt):
        if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store):
            out.add(n.id)
    return out


def target_statements():
    """`target_actions = ...` through the last assignment of `target` in `Agent.learn`, compiled as they stand."""
    tree = ast.parse(open(AGENT, encoding="utf-8").read(), filename=AGENT)
    learn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "learn")
    body = learn.body
    first = next(k for k, s in enumerate(body) if isinstance(s, ast.Assign) and "target_actions" in _stores(s))
    last = max(k for k, s in enumerate(body) if isinstance(s, ast.Assign) and "target" in _stores(s))
    block = body[first:last + 1]
    assert first < last and any(isinstance(s, ast.Assign) and isinstance(s.targets[0], ast.Subscript) for s in block), \
        "the target statements changed in the reference"
    return compile(ast.Module(body=block, type_ignores=[]), AGENT, "exec")


TARGET = target_statements()


def observations(rng, B, V, tn):
    obs = np.empty((B, V, tn + 5), np.float32)
    obs[:, :, :tn] = rng.uniform(0, 2 * np.pi, (B, V, tn))
    obs[:, :, tn:] = rng.uniform(0, 1.2, (B, V, 5))
    obs[:, :, tn + 3] = 0.0
    return obs


def capture(V, M, fc1, fc2, fc3, afc1, afc2, B, seed):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    tn, n_actions = M // V, 2 * V + M
    critic = REFNET.CriticNetwork(1e-3, tn + 5, fc1, fc2, fc3, V, n_actions, name="target_critic")
    actor = REFNET.ActorNetwork(1e-4, tn + 5, afc1, afc2, V, n_actions, name="target_actor")
    with torch.no_grad():
        critic.q.weight.uniform_(-0.4, 0.4)
        critic.q.bias.uniform_(-0.4, 0.4)
        for bn in (critic.bn1, critic.bn2, critic.bn3, actor.bn1, actor.bn2):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
        actor.mu.weight.uniform_(-0.4, 0.4)
        actor.mu.bias.uniform_(-0.4, 0.4)
    state = observations(rng, B, V, tn)
    state[0] = 0.0                                            # the observation before the first step of a fresh env
    state_ = observations(rng, B, V, tn)
    action = np.empty((B, n_actions), np.float32)
    action[:B // 2] = rng.uniform(-0.999, 0.999, (B // 2, n_actions))
    action[B // 2:] = rng.uniform(0.0, 1.0, (B - B // 2, n_actions))
    reward = rng.uniform(-6.0, 1.0, B).astype(np.float32)
    done = rng.uniform(size=B) < 0.25
    assert done.sum() >= 5 and (~done).sum() >= 5
    gamma = 0.99
    critic.eval()
    actor.eval()
    agent = types.SimpleNamespace(target_actor=actor, target_critic=critic, critic=critic, gamma=gamma, batch_size=B)
    ns = dict(self=agent, states=torch.from_numpy(state.reshape(B, -1)), actions=torch.from_numpy(action),
              states_=torch.from_numpy(state_.reshape(B, -1)), rewards=torch.from_numpy(reward), done=torch.from_numpy(done))
    with torch.no_grad():
        q_next = critic.forward(ns["states_"], actor.forward(ns["states_"])).clone()     # before the mask overwrites it
        exec(TARGET, ns)
    target, q = ns["target"], ns["critic_value"]
    assert tuple(target.shape) == (B, 1) and tuple(q.shape) == (B, 1)
    assert torch.equal(target.view(-1)[ns["done"]], ns["rewards"][ns["done"]])
    assert float(q.abs().max()) > 0.3, "q does not leave the neighbourhood of zero"
    weights = {"w." + k: v.numpy().copy() for k, v in critic.state_dict().items()}
    weights.update({"aw." + k: v.numpy().copy() for k, v in actor.state_dict().items()})
    path = os.path.join(OUT_DIR, "sarl_critic_%d_%d.npz" % (V, M))
    np.savez_compressed(path, V=V, M=M, fc1=fc1, fc2=fc2, fc3=fc3, afc1=afc1, afc2=afc2, B=B, state=state, action=action,
                        q=q.numpy(), state_=state_, target_action=ns["target_actions"].numpy(), q_next=q_next.numpy(),
                        reward=reward, done=done, gamma=np.float64(gamma), target=target.numpy(), **weights)
    print("sarl_critic_%d_%d: %d -> %d -> %d -> %d -> 1, %d actions, batch %d (%d done), %d bytes"
          % (V, M, V * (tn + 5), fc1, fc2, fc3, n_actions, B, int(done.sum()), os.path.getsize(path)))


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    capture(8, 40, 96, 128, 128, 64, 128, 70, 31)
    capture(4, 16, 64, 128, 128, 32, 128, 33, 32)
