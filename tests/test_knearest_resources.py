"""k_knearest, the traversal of rj_knearest_query, keeps its lists in global memory and beside them only the number held and
the worst candidate's slot, double and bound per lane: no scratch memory, no spill, and no more than the 128 VGPRs that let
a SIMD hold four waves -- the bar of tests/test_nearest_resources.py for the same walk -- in either instantiation.  Read
from the resource report of the build (`make` writes rayjoin_amd/csrc/resource_usage_knearest.txt:
-Rpass-analysis=kernel-resource-usage), on any machine."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resource_report  # noqa: E402

REPORT = "resource_usage_knearest.txt"


def test_the_traversal_kernel_uses_no_scratch_and_four_waves_fit():
    assert os.path.exists(resource_report.path(REPORT)), resource_report.MISSING
    hits = {k: v for k, v in resource_report.kernels(REPORT).items() if "k_knearest" in k}
    assert len(hits) == 2, sorted(hits)  # the plain and the instrumented kernel
    for name, r in hits.items():
        print("%s: %d VGPRs, %d bytes of LDS" % (name, r["VGPRs"], r["LDS Size"]))
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, "%s: %d VGPRs, %s" % (name, r["VGPRs"], r)
        assert 0 < r["VGPRs"] <= 128, "%s: %d VGPRs (above 128 a SIMD holds fewer than four waves)" % (name, r["VGPRs"])
        assert r["LDS Size"] <= 32768, "%s: %d VGPRs, %d bytes of LDS" % (name, r["VGPRs"], r["LDS Size"])
