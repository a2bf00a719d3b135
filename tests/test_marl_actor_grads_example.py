"""examples/marl_actor_grads.py runs end to end on a GPU box at 64 rows, in a fresh child process under a time limit: the critic
side of the actor update through `BatchedTwinCritic.action_grad`, the two launches named, and the stand-in policy's parameter
gradients within the bar of test_marl_action_grad_hip.py -- the device form's largest difference from float64 autograd at most
max(8 x float32 autograd's, 2^-22)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_marl_actor_grads_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "marl_actor_grads.py"), "64"], cwd=ROOT,
                         capture_output=True, text=True, timeout=240)
    print(out.stdout[-2000:], out.stderr[-1500:])
    assert out.returncode == 0
    assert "batch 64 rows" in out.stdout and "actor loss" in out.stdout
    assert "critic side: k_marl_critic_action_grad_rows<4,2>x2 -> k_marl_critic_action_grad_select" in out.stdout
    m = re.search(r"against float64 autograd: largest relative difference device (\S+)  autograd float32 (\S+)", out.stdout)
    device, library = float(m.group(1)), float(m.group(2))
    assert device <= max(8 * library, 2.0 ** -22), (device, library)
    assert re.search(r"policy gradients against autograd: largest relative difference \S+", out.stdout)
