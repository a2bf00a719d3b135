"""examples/marl_critic_grads.py runs end to end on a GPU box at 64 envs, one episode and 64 rows, in a fresh child process
under a time limit: the critic update with no autograd graph, its gradients checked against autograd's inside the example, and
the nine launches between "the TD target is ready" and "the next TD target is ready" named."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_marl_critic_grads_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "marl_critic_grads.py"), "64", "1", "64"], cwd=ROOT,
                         capture_output=True, text=True, timeout=240)
    print(out.stdout[-2000:], out.stderr[-1500:])
    assert out.returncode == 0
    assert "batch 64 rows" in out.stdout and "critic loss" in out.stdout
    assert "gradients against autograd: largest relative difference" in out.stdout
    assert ("loss + gradients:  2 x [k_marl_critic_pack x2] -> k_marl_critic_grad_rows<4,2>x2 -> k_marl_critic_grad_weights"
            in out.stdout)
    assert ("launches after the td target: 2 x [k_marl_critic_pack x2] -> k_marl_critic_grad_rows<4,2>x2 -> "
            "k_marl_critic_grad_weights -> k_adam_sqsum + k_adam_step -> 2 x [k_marl_critic_pack x2] -> k_marl_critic<4,2>x2"
            in out.stdout)
