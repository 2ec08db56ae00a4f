#!/usr/bin/env python3
"""More seeds of the randomised face-ring tests, by hand (GPU box):  python tests/rings_fuzz_more.py [first_seed [count]]
Per seed one random planar subdivision (tests/rings_planar.py's draw_planar: the device against the plain-Python
definition under flags 0 and SKIP_FACE0 | NO_POINTS, and against the faces and areas of the union-find) and one fuzzed
overlay pair (tests/test_gpu_rings.py's check_rings_of_a_fuzzed_overlay: the definition on every output map, the face
table's areas on the maps of float pairs without a mixed ring); a failure carries the seed and the flags.
Test infrastructure (it imports oracle/): not collected by pytest, not part of the product."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import rjoracle as oracle  # noqa: E402
from rayjoin_amd import _capi  # noqa: E402
import rings_planar as P  # noqa: E402
import rings_ref as D  # noqa: E402
from test_gpu_rings import NOPTS, SKIP0, check_rings_of_a_fuzzed_overlay, device_rings  # noqa: E402

first = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
count = int(sys.argv[2]) if len(sys.argv) > 2 else 20
oracle.lib().rjo_set_num_threads(16)
handle = _capi.Handle(0)
seen = {}
for seed in range(first, first + count):
    m, info = P.draw_planar(seed)
    if len(m[2]):
        for flags in (0, SKIP0 | NOPTS):
            got = device_rings(handle, m, flags)
            D.assert_same_rings(got, D.rings_ref(*m, skip_face0=bool(flags & SKIP0), points=not flags & NOPTS), (seed, flags))
            P.assert_planar_answer(got, info, skip_face0=bool(flags & SKIP0), what=(seed, flags))
        key = ("frame" if info["frame"] else "open") + (", full range" if info["full_range"] else ", sheared")
        seen[key] = seen.get(key, 0) + 1
    kind, chains, n_maps, unmixed = check_rings_of_a_fuzzed_overlay(oracle, seed)
    seen[kind] = seen.get(kind, 0) + 1
    seen[kind + " maps without a mixed ring"] = seen.get(kind + " maps without a mixed ring", 0) + unmixed
    print("seed %d ok (%d chains in its output maps; %s so far)" % (seed, chains, seen), flush=True)
handle.close()
print("all %d seeds ok" % count)
