"""RJ_OVM_MERGE_PIECES at mid size against the numpy form of the definition, exactly: the child process
tests/overlay_merge_midsize_check.py (the 4.4 M x 4.9 M edge pair of tests/overlay_midsize_check.py; clip and
(union, pair), both drop settings)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_midsize_merged_maps_equal_the_numpy_definition_exactly():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "overlay_merge_midsize_check.py")], capture_output=True, text=True,
                       timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.returncode, r.stderr[-3000:])
    out = json.loads(lines[-1])
    print(out)
    assert out["map0_edges"] > 2097152 and out["map1_edges"] > 2097152 and out["intersections"] > 262144
    assert out["bad"] == [] and out["ok"] and r.returncode == 0, (out["bad"], r.stderr[-3000:])
    assert sorted(out["cases"]) == ["intersection/map0", "union/pair"]
    clip = out["cases"]["intersection/map0"]
    for drop in ("drop0", "drop1"):  # the clip is what the merge is for: far fewer chains, a point less per chain gone
        un, me = clip[drop]["unmerged"], clip[drop]["merged"]
        assert me[0] < un[0] and un[0] - me[0] == un[1] - me[1]
