"""examples/marl_soft_update.py runs end to end on a GPU box at 64 rows, in a fresh child process under a time limit, and
names the four launches between "the optimiser stepped" and "the next TD target is ready"."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_marl_soft_update_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "marl_soft_update.py"), "64", "1", "64"], cwd=ROOT,
                         capture_output=True, text=True, timeout=240)
    print(out.stdout[-1500:], out.stderr[-1500:])
    assert out.returncode == 0
    assert "batch 64 rows" in out.stdout and "mean target" in out.stdout
    assert "k_soft_update -> 2 x [k_marl_critic_pack x2] -> k_marl_critic<4,2>x2" in out.stdout
