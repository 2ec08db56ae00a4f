"""The overlay's face table and output map at mid size against the exact numpy forms of the helper: the child process
tests/overlay_midsize_check.py (4.4 M x 4.9 M edges: the second trip of the kernels' wave loops, the third level of the
64-ary record search)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_midsize_tables_and_maps_equal_the_numpy_helper_exactly():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "overlay_midsize_check.py")], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.returncode, r.stderr[-3000:])
    out = json.loads(lines[-1])
    print(out)
    assert out["map0_edges"] > 2097152 and out["map1_edges"] > 2097152 and out["intersections"] > 262144
    assert out["bad"] == [] and out["ok"] and r.returncode == 0, (out["bad"], r.stderr[-3000:])
    assert len(out["cases"]) == 6 and all(c["rows"] >= 1000 for c in out["cases"].values())
