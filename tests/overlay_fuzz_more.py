#!/usr/bin/env python3
"""More seeds of tests/test_gpu_overlay_fuzz.py, by hand (GPU box):  python tests/overlay_fuzz_more.py [first_seed [count]]
The same draw and the same checks per pair (records and vertex faces against the oracle, face table and output map of
the drawn operations against the plain-Python helper, the cascade through InstallMap), four pairs per seed; a failure
carries (seed, pair index, kind of pair, edge counts, record source, how, by, drop).
Test infrastructure (it imports oracle/): not collected by pytest, not part of the product."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import rjoracle as oracle  # noqa: E402
from test_gpu_overlay_fuzz import check_pair  # noqa: E402

first = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
count = int(sys.argv[2]) if len(sys.argv) > 2 else 20
oracle.lib().rjo_set_num_threads(16)
kinds = {}
for seed in range(first, first + count):
    rng = np.random.default_rng(seed)
    for k in range(4):
        kind, source, cascaded = check_pair(oracle, rng, (seed, k))
        for key in (kind, source.split("-")[0], "cascade" if cascaded else "no cascade"):
            kinds[key] = kinds.get(key, 0) + 1
    print("seed %d ok (%s so far)" % (seed, kinds), flush=True)
print("all %d seeds ok" % count)
