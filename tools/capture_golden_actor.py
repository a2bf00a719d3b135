#!/usr/bin/env python3
"""Capture golden vectors for the DDPG actor forward (`BatchedActor`) from the REFERENCE.

    python tools/capture_golden_actor.py <path to the reference checkout>      (or RISVEC_REFERENCE)

Imports the reference's own `Simulation-SARL/networks.ActorNetwork` (CPU torch) read-only and builds it at reduced
hidden sizes (the architecture is size-agnostic; small sizes keep the fixtures small, as `policy_*.npz` does).  The
`mu` layer and the LayerNorm parameters are widened so that the outputs span (0, 1): at the reference's own +-0.003
head every sigmoid is 0.5.  Inputs are shaped like real observations (`ddpg_train.py:134-149`: per agent the phase
slice in [0, 2 pi), then five scalars in [0, 1.2] with element tn + 3 zero).  The pre-sigmoid values are what the
reference's own `mu` layer returned (a forward hook).  Fixtures hold weights, inputs and outputs only.
"""
from __future__ import annotations

import os
import sys

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("RISVEC_REFERENCE", "")
REF_DIR = os.path.join(REF, "Simulation-SARL")
OUT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
if not REF or not os.path.isfile(os.path.join(REF_DIR, "networks.py")):
    sys.exit("capture_golden_actor: give the reference checkout (argument or RISVEC_REFERENCE)")
sys.dont_write_bytecode = True
sys.path.insert(0, REF_DIR)
import torch  # noqa: E402
import networks as REFNET  # noqa: E402  (the reference itself)


def capture(V, M, fc1, fc2, B, seed):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    tn = M // V
    n_actions = 2 * V + M
    net = REFNET.ActorNetwork(1e-4, tn + 5, fc1, fc2, V, n_actions, name="actor")
    with torch.no_grad():
        net.mu.weight.uniform_(-0.4, 0.4)
        net.mu.bias.uniform_(-0.4, 0.4)
        net.bn1.weight.uniform_(0.5, 1.5); net.bn1.bias.uniform_(-0.2, 0.2)
        net.bn2.weight.uniform_(0.5, 1.5); net.bn2.bias.uniform_(-0.2, 0.2)
    obs = np.empty((B, V, tn + 5), np.float32)
    obs[:, :, :tn] = rng.uniform(0, 2 * np.pi, (B, V, tn))
    obs[:, :, tn:] = rng.uniform(0, 1.2, (B, V, 5))
    obs[:, :, tn + 3] = 0.0
    obs[0] = 0.0                                              # the observation before the first step of a fresh env
    state = torch.from_numpy(obs.reshape(B, -1))              # np.asarray(state_old_all).flatten(): agent-major
    seen = {}
    hook = net.mu.register_forward_hook(lambda mod, inp, out: seen.__setitem__("logits", out.detach().clone()))
    net.eval()
    with torch.no_grad():
        out = net.forward(state)
    hook.remove()
    assert torch.equal(torch.sigmoid(seen["logits"]), out)
    assert float(out.min()) < 0.1 and float(out.max()) > 0.9, "outputs do not span (0, 1)"
    weights = {"w." + k: v.numpy().copy() for k, v in net.state_dict().items()}
    path = os.path.join(OUT_DIR, "sarl_actor_%d_%d.npz" % (V, M))
    np.savez_compressed(path, V=V, M=M, fc1=fc1, fc2=fc2, B=B, obs=obs, logits=seen["logits"].numpy(), mu=out.numpy(), **weights)
    print("sarl_actor_%d_%d: %d -> %d -> %d -> %d, batch %d, %d bytes" % (V, M, V * (tn + 5), fc1, fc2, n_actions, B,
                                                                      os.path.getsize(path)))


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    capture(8, 40, 96, 128, 70, 21)
    capture(4, 16, 64, 128, 33, 22)
