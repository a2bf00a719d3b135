"""The local-target example runs end to end on a GPU box (small batch)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_marl_local_targets_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "marl_local_targets.py"), "64", "1"], cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "episode 0" in out.stdout and "launches: 4" in out.stdout and "k_local_critics<4,2>x8x2" in out.stdout
    assert "fused vs library" in out.stdout
