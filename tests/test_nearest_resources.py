"""k_nearest, the traversal of rj_nearest_query, keeps its candidate -- two 128-bit integers, a double and a 64-bit bound per
lane -- and the wide compare's limbs in registers: no scratch memory, in either instantiation.  Read from the resource
report of the build (`make` writes rayjoin_amd/csrc/resource_usage_nearest.txt: -Rpass-analysis=kernel-resource-usage)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resource_report  # noqa: E402

REPORT = "resource_usage_nearest.txt"


def kernels():
    assert os.path.exists(resource_report.path(REPORT)), resource_report.MISSING
    return resource_report.kernels(REPORT)


def test_the_traversal_kernel_uses_no_scratch():
    hits = {k: v for k, v in kernels().items() if "k_nearest" in k}
    assert len(hits) == 2, sorted(kernels())  # the plain and the instrumented kernel
    for name, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, "%s: %d VGPRs, %s" % (name, r["VGPRs"], r)
        assert 0 < r["VGPRs"] <= 128, "%s: %d VGPRs (above 128 a SIMD holds fewer than four waves)" % (name, r["VGPRs"])
        assert r["LDS Size"] <= 32768, "%s: %d VGPRs, %d bytes of LDS" % (name, r["VGPRs"], r["LDS Size"])
