"""k_window, the traversal of rj_window_query, keeps a window, a segment and two 128-bit products at most in registers: no
scratch memory, no spills and at most 128 VGPRs, in either instantiation; its stack and staging buffer stay within 32 KiB of
LDS per block.  Read from the resource report of the build (`make` writes rayjoin_amd/csrc/resource_usage_window.txt:
-Rpass-analysis=kernel-resource-usage)."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resource_report  # noqa: E402

REPORT = "resource_usage_window.txt"


def kernels():
    assert os.path.exists(resource_report.path(REPORT)), resource_report.MISSING
    return resource_report.kernels(REPORT)


def test_the_traversal_kernel_uses_no_scratch():
    hits = {k: v for k, v in kernels().items() if re.search(r"k_windowILb[01]E", k)}
    assert len(hits) == 2, sorted(kernels())  # the plain and the instrumented kernel
    for name, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, "%s: %d VGPRs, %s" % (name, r["VGPRs"], r)
        assert 0 < r["VGPRs"] <= 128, "%s: %d VGPRs (above 128 a SIMD holds fewer than four waves)" % (name, r["VGPRs"])
        assert 0 < r["LDS Size"] <= 32768, "%s: %d VGPRs, %d bytes of LDS" % (name, r["VGPRs"], r["LDS Size"])


def test_the_other_kernels_use_no_scratch():
    rest = {k: v for k, v in kernels().items() if "k_window_" in k}
    assert len(rest) == 2, sorted(kernels())  # the totals and the outputs
    for name, r in rest.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
