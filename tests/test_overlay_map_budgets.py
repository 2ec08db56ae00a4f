"""Register budgets of the output map's kernels, in the style of tests/test_register_budgets.py: the emit pass runs a lane
per edge over both maps twice, and what hides its dependent loads is waves in flight -- at most 64 VGPRs keeps 8 waves per
SIMD, and nothing may spill.  Pinned against the resource report of the build (`make` writes
rayjoin_amd/csrc/resource_usage_overlay_map.txt: -Rpass-analysis=kernel-resource-usage)."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPORT = os.path.join(os.path.dirname(HERE), "rayjoin_amd", "csrc", "resource_usage_overlay_map.txt")


def _kernels():
    assert os.path.exists(REPORT), "no resource report: build the library first (__graft_entry__.build)"
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


def test_output_map_kernels_keep_eight_waves_and_do_not_spill():
    k = _kernels()
    for frag in ("k_ovm_emitILb0", "k_ovm_emitILb1", "k_ovm_label", "k_ovm_keep", "k_ovm_compact_points", "k_map_check"):
        hits = [v for name, v in k.items() if frag in name]
        assert len(hits) == 1, (frag, [n for n in k if "k_ovm" in n or "k_map" in n])
        assert hits[0]["VGPRs"] <= 64 and hits[0]["ScratchSize"] == 0, (frag, hits[0])
