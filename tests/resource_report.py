"""The compiler's resource report of a build (`make` writes rayjoin_amd/csrc/resource_usage*.txt:
-Rpass-analysis=kernel-resource-usage), read once for the tests that pin registers, scratch and LDS."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rayjoin_amd", "csrc")
MISSING = "no resource report: build the library first (__graft_entry__.build)"


def path(name):
    return os.path.join(CSRC, name)


def kernels(name):
    """the report file `name` -> {mangled kernel name: {"VGPRs": .., "ScratchSize": .., "LDS Size": .., ...}}"""
    out, kernel = {}, None
    for line in open(path(name)):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            kernel = m.group(1)
            out[kernel] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and kernel:
            out[kernel][m.group(1).strip()] = int(m.group(2))
    return out
