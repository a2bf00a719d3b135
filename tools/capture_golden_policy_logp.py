#!/usr/bin/env python3
"""Capture golden vectors for `BatchedPolicy.sample_normal` from the REFERENCE.  Runs ONLY in the CPU build container.

As tools/capture_golden_policy.py: imports the reference's own `sac_agent.PolicyNetwork` (CPU torch), builds one network
per agent (small hidden sizes), and calls `sample_normal(state, reparameterize=False, mask)` under a fixed torch seed --
here keeping all five outputs (power, y, log_prob_power, log_prob_intent, total).  The draws it consumed are re-drawn
from the same seed and VERIFIED to reproduce the reference's power and y bit for bit before anything is saved.

The log_std head is set by hand (small weights, bias in [-2.5, -0.7]) and the mu head kept moderate, so that the tanh is
rarely saturated: where it is, log(1 - p^2 + 1e-6) of the float32 p carries a rounding floor 2^-22 / (1 - p^2 + 1e-6)
that is too loose to test a sum against.  At most 2 % of the samples may have a floor above 1e-4 (asserted here and in
tests/test_policy_sample_normal_host.py).  Fixtures hold weights, inputs, draws and outputs only; they are named
logp_policy_*.npz because tests/test_policy_oracle_golden.py counts the files matching policy_*.npz.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

REF_DIR = "/root/reference/Simulation-MARL-BCD"
OUT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
if not os.path.isfile(os.path.join(REF_DIR, "sac_agent.py")):
    sys.exit("capture_golden_policy_logp: reference not present (this tool only runs in the build container)")
sys.dont_write_bytecode = True
sys.path.insert(0, REF_DIR)
import torch  # noqa: E402
import sac_agent as REF  # noqa: E402  (the reference itself)

FLOOR_CAP, FLOOR_CAP_SHARE = 1e-4, 0.02


def capture(tag, V, fc1, fc2, B, seed):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    tmp = tempfile.mkdtemp(prefix="risvec_policy_logp_")     # the constructor creates its checkpoint dir
    names = ("state", "mask", "has_mask", "tau", "hard", "eps", "expo", "mu", "log_std", "logits", "power", "probs",
             "logp_power", "logp_intent", "logp_total")
    rec = {k: [] for k in names}
    weights = {}
    for a in range(V):
        net = REF.PolicyNetwork(3e-4, 5, fc1, fc2, 2, V, name="policy", agent_label=a, chkpt_dir=tmp)
        net = net.to("cpu")
        net.device = torch.device("cpu")
        with torch.no_grad():                                  # move the net away from its near-zero heads
            net.mu.weight.uniform_(-0.15, 0.15)
            net.intent_logits.weight.uniform_(-0.4, 0.4)
            net.log_std.weight.uniform_(-0.02, 0.02)
            net.log_std.bias.uniform_(-2.5, -0.7)
            net.bn1.weight.uniform_(0.5, 1.5); net.bn1.bias.uniform_(-0.2, 0.2)
            net.bn2.weight.uniform_(0.5, 1.5); net.bn2.bias.uniform_(-0.2, 0.2)
        tau = float(rng.choice([2.0, 1.0, 0.5]))
        net.tau.fill_(tau)
        state = torch.from_numpy(rng.uniform(0, 1.2, (B, 5)).astype(np.float32))
        has_mask = a % 3 != 2
        hard = a % 4 == 3                                       # straight-through one-hot
        net.gumbel_hard = hard
        mask = torch.from_numpy((rng.uniform(size=(B, V)) < 0.6).astype(np.float32))
        mask[0] = 0.0                                           # an all-zero row: the reference opens it up
        net.eval()
        s = seed * 100 + a
        with torch.no_grad():
            torch.manual_seed(s)
            power, y, lp_pow, lp_int, lp_tot = net.sample_normal(state, reparameterize=False, mask=mask if has_mask else None)
            mu, log_std, logits = net.forward(state)
            # re-draw what sample_normal consumed and verify
            torch.manual_seed(s)
            eps = torch.empty(B, 2).normal_()
            expo = torch.empty(B, V).exponential_()
            ml = logits
            if has_mask:
                m = mask.clone()
                m[m.sum(-1) == 0] = 1.0
                ml = logits.masked_fill(m <= 0, torch.finfo(logits.dtype).min / 2)
            y2 = ((ml + -expo.log()) / tau).softmax(-1)
            if hard:
                y_hard = torch.zeros_like(y2).scatter_(-1, y2.max(-1, keepdim=True)[1], 1.0)
                y2 = y_hard - y2 + y2
            assert torch.equal(torch.tanh(eps * log_std.exp() + mu), power), "normal draws not reproduced"
            assert torch.equal(y2, y), "gumbel draws not reproduced"
            assert torch.equal(lp_pow + lp_int, lp_tot)
        for k, v in net.state_dict().items():
            if k != "tau":
                weights["a%d.%s" % (a, k)] = v.numpy().copy()
        for k, v in dict(state=state, mask=mask, has_mask=has_mask, hard=hard, tau=tau, eps=eps, expo=expo, mu=mu,
                         log_std=log_std, logits=logits, power=power, probs=y, logp_power=lp_pow[:, 0],
                         logp_intent=lp_int[:, 0], logp_total=lp_tot[:, 0]).items():
            rec[k].append(v.numpy() if hasattr(v, "numpy") else v)
    p = np.asarray(rec["power"], np.float64)
    floor = 2.0 ** -22 / (1.0 - p * p + 1e-6)
    share = float((floor > FLOOR_CAP).mean())
    assert share <= FLOOR_CAP_SHARE, "too many saturated samples: %.3f" % share
    np.savez_compressed(os.path.join(OUT_DIR, "logp_policy_%s.npz" % tag), V=V, fc1=fc1, fc2=fc2, B=B,
                        **{k: np.asarray(v) for k, v in rec.items()}, **weights)
    print("logp_policy_%s: %d agents, batch %d, hidden %d/%d; %.2f %% of the samples with a floor above %g, largest floor %.3g"
          % (tag, V, B, fc1, fc2, 100 * share, FLOOR_CAP, floor.max()))


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    capture("8", 8, 48, 32, 96, 17)
    capture("4", 4, 40, 24, 33, 18)
