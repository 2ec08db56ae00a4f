#!/usr/bin/env python3
"""More seeds of the raw ring soups of tests/polygons_soups.py, by hand:  python tests/polygons_fuzz_more.py [first_seed [count]]
Per seed one sliver soup (heights p.y + t / d at 2^45: candidate(), floor_div() and the fractional step of lower()) and one
slope fan (equal heights: the slope step and the slot step): the plain-Python definition (tests/polygons_ref.py) against
the host twin, and against the device where there is one (no device: the twin alone, and the last line says so); a failure
carries the seed.  Test infrastructure: not collected by pytest, not part of the product."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rayjoin_amd import _capi  # noqa: E402
import polygons_ref as PR  # noqa: E402
import polygons_soups as PS  # noqa: E402
from test_polygons import twin_lib, twin_polygons  # noqa: E402

first = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
count = int(sys.argv[2]) if len(sys.argv) > 2 else 20
twin = twin_lib()
try:
    handle = _capi.Handle(0)
except _capi.RayJoinError as e:
    handle = None
    print("no device (%s): the twin alone" % e)
if handle is not None:
    from test_gpu_polygons import device_polygons  # noqa: E402
for seed in range(first, first + count):
    for kind, make in (("sliver", PS.sliver_ceilings), ("fan", PS.slope_fan)):
        rings, row, xy, info = make(seed)
        want = PR.polygons_ref(rings, row, xy)
        rc, got, _ = twin_polygons(twin, rings, row, xy)
        assert rc == 0, (kind, seed)
        PR.assert_same_polygons(got, want, (kind, seed, "twin"))
        if handle is not None:
            PR.assert_same_polygons(device_polygons(handle, rings, row, xy), want, (kind, seed, "device"))
        if kind == "fan":
            assert all(int(want["parent"][g["hole"]]) == g["above"] for g in info["groups"]), seed
    print("seed %d ok (%d polygons, %d holes, %d orphans in its fan)" % (seed, want["counts"]["n_polygons"], want["counts"]["n_holes"],
                                                                         want["counts"]["n_orphans"]), flush=True)
if handle is not None:
    handle.close()
print("all %d seeds ok, %s" % (count, "twin and device" if handle is not None else "twin only"))
