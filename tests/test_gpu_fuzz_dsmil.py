"""Randomised cross-check of the DSMIL kernels against float64 torch on the CPU (tools/fuzz_dsmil.py): class counts 1..16, both row
types, 1..12 ragged bags sized around the tile and part boundaries, with and without dropout, forward and backward, as a list and
as a ``BagSet`` -- the fixed-seed set only."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_fuzz_dsmil_against_the_collapsed_formula_in_float64():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_dsmil.py"), "40", "28"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "fuzz dsmil ok: 40 draws from seed 28" in r.stdout
