"""k_pip_walk2_prepared -- k_pip_walk2's body over the query map's prepared points -- takes k_pip_walk2's place in the
shared schedule of a step, so it is held to the same budget (tests/test_register_budgets.py): 56 VGPRs, 96 SGPRs, no
scratch.  Its name must not be mistaken for k_pip_walk2's by whoever looks that kernel up in the resource report."""
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPORT = os.path.join(os.path.dirname(HERE), "rayjoin_amd", "csrc", "resource_usage.txt")


def _kernels():
    if not os.path.exists(REPORT):
        pytest.skip("no resource report: build the library first (__graft_entry__.build)")
    out, name = {}, None
    for line in open(REPORT):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def test_the_prepared_walk_keeps_the_walks_budget():
    k = _kernels()
    hits = [n for n in k if "k_pip_walk2_preparedE" in n]
    assert len(hits) == 1, hits
    assert "k_pip_walk2E" not in hits[0]
    r, walk2 = k[hits[0]], [v for n, v in k.items() if "k_pip_walk2E" in n]
    assert len(walk2) == 1
    assert r["VGPRs"] <= 56 and r["ScratchSize"] == 0 and r["TotalSGPRs"] <= 96, r
    assert r["VGPRs"] <= walk2[0]["VGPRs"]  # (pip_walk2_blocks_beside sizes the shared grid by k_pip_walk2's registers)
    assert r["Occupancy"] >= walk2[0]["Occupancy"]
