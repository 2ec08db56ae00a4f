"""k_pip_walk3_prepared -- the walk's body with three 64-position sets per wave over the query map's prepared points --
takes k_pip_walk2's place beside k_lsi2 in the shared schedule of a step, so it is held to k_pip_walk2's budget
(tests/test_register_budgets.py): 56 VGPRs, 96 SGPRs, no scratch, and to the byte the LDS of a k_pip_walk2 block, so
that six of its blocks fit beside two of k_lsi2's exactly as measured."""
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rayjoin_amd", "csrc")
REPORT = os.path.join(CSRC, "resource_usage.txt")


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


def test_three_sets_keep_the_walks_registers():
    k = _kernels()
    hits = [n for n in k if "k_pip_walk3_preparedE" in n]
    assert len(hits) == 1, hits
    r, walk2 = k[hits[0]], [v for n, v in k.items() if "k_pip_walk2E" in n]
    assert len(walk2) == 1
    assert r["VGPRs"] <= 56 and r["VGPRs"] <= walk2[0]["VGPRs"], r  # (pip_walk2_blocks_beside sizes the shared grid by k_pip_walk2's)
    assert r["ScratchSize"] == 0 and r["TotalSGPRs"] <= 96, r
    assert r["Occupancy"] >= walk2[0]["Occupancy"]


def _const(src, name):
    m = re.search(r"constexpr int %s = (\d+);" % name, src)
    assert m, name
    return int(m.group(1))


def test_three_sets_take_the_lds_of_two():
    src = open(os.path.join(CSRC, "rj_kernels.hip")).read()
    m = re.search(r"#define RJ_WALK_LIST (\d+)", open(os.path.join(CSRC, "rj_device.h")).read())
    wlist, wstack = int(m.group(1)), _const(src, "kWalkStack")
    list3, stack3 = _const(src, "kWalk3List"), _const(src, "kWalk3Stack")
    # per wave: a 16-byte entry per stack slot + 256 bytes (64 lanes x 4) per list slot and set; four waves a block
    two = 4 * (16 * wstack + 2 * wlist * 256)
    three = 4 * (16 * stack3 + 3 * list3 * 256)
    assert three == two == 20224
    assert list3 <= wlist  # (a todo record has kWalkList slots: k_pip_exact reads the same records from either walk)
    # the kernel is the body instantiated with exactly these
    assert re.search(r"void k_pip_walk3_prepared\(PipArgs A\) \{ pip_walk_many<false, 3, true, kWalk3List, kWalk3Stack>\(A\); \}", src)
    assert re.search(r"walk2_wave_lds\(top, 3, kWalk3List, kWalk3Stack\)", src)
