#!/usr/bin/env python3
"""RJ_OVM_MERGE_PIECES at FULL size (BASELINE config 4, USCounty x Zipcode stand-ins), not collected by pytest, in the
protocol of tests/overlay_ops_fullsize_check.py: in ONE process, on the same records, the variants alternating over
--rounds rounds, best of --reps wall times each, of rj_overlay_map_op for clip and for (union, pair) and of
rj_overlay_map (the plain intersection) with flags 0, RJ_OVM_DROP_DEGENERATE, RJ_OVM_MERGE_PIECES and both; chains and
points before and after the merge; and the check that costs little at this size: every merged array equals the numpy form
of the definition (tests/overlay_merge_ref.py) applied to the same call's unmerged arrays.
RAYJOIN_AMD_LIB=<the parent revision's library> measures that revision's calls with flags 0 and
RJ_OVM_DROP_DEGENERATE alone (the flag is RJ_E_INVALID there): the baseline of the comparison, by the same script on the
same machine."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rayjoin_amd import _capi, maps, synth  # noqa: E402
import overlay_merge_ref as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--m0", default="USCounty")
ap.add_argument("--m1", default="Zipcode")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-check", action="store_true", help="times only (for a run under a profiler)")
a = ap.parse_args()
ctx = maps.Context([synth.standin(a.m0, a.scale), synth.standin(a.m1, a.scale)]).load()
m = ctx.maps
h = _capi.Handle(0)
for im in range(2):
    h.upload_map(im, m[im].pts, m[im].row_index, m[im].left, m[im].right)
h.build_lbvh(0)
h.build_lbvh(1)
cap = int(0.2 * (m[0].n_edges + m[1].n_edges))
pairs = h.alloc(8 * cap)
n = h.lsi_query(1, 0, 0, m[0].n_edges, cap, pairs)
fc = [h.alloc(4 * m[i].n_points) for i in range(2)]
cl = [h.alloc(4 * m[i].n_points) for i in range(2)]
for im in range(2):
    h.pip_query(1 - im, im, None, 0, m[im].n_points, cl[im], fc[im])
xs = [h.alloc(48 * max(1, n)) for _ in range(2)]
for im in range(2):
    h.overlay_edge_xsects(im, pairs, n, xs[im])
h.sync()
args = (xs[0], xs[1], n, fc[0], fc[1])
MERGE = getattr(_capi, "RJ_OVM_MERGE_PIECES", 2)
try:  # does this library know the flag?
    h.overlay_map(*args, MERGE, (0, 0, 0), None, None, None, None, None, None)
    has_merge = True
except _capi.MapOverflow:
    has_merge = True
except _capi.RayJoinError:
    has_merge = False
OPS = {"clip": (_capi.RJ_OV_INTERSECTION, _capi.RJ_OV_BY_MAP0), "union": (_capi.RJ_OV_UNION, _capi.RJ_OV_BY_PAIR), "plain": None}
FLAGS = [("flags0", 0), ("drop", 1)] + ([("merge", MERGE), ("drop_merge", 1 | MERGE)] if has_merge else [])


def kw(op):
    return {} if op is None else {"op": op}


# capacities for the largest output: the union without a flag
try:
    h.overlay_map(*args, 0, (0, 0, 0), None, None, None, None, None, None, op=OPS["union"])
    cc, pc, fcap = 0, 0, 0
except _capi.MapOverflow as e:
    cc, pc, fcap = e.counts
bufs = [h.alloc(16 * max(1, pc)), h.alloc(4 * (cc + 1)), h.alloc(4 * max(1, cc)), h.alloc(4 * max(1, cc)), h.alloc(8 * max(1, fcap)),
        h.alloc(4 * max(1, cc))]


def read_map(k, p, f):
    return dict(xy=bufs[0].to_host(np.int64, 2 * p).reshape(-1, 2), row_index=bufs[1].to_host(np.uint32, k + 1),
                left=bufs[2].to_host(np.int32, k), right=bufs[3].to_host(np.int32, k),
                face_pairs=bufs[4].to_host(np.int32, 2 * f).reshape(-1, 2), origin=bufs[5].to_host(np.uint32, k))


def timed(fn):
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return r, [round(v, 3) for v in ms]


out = {"lib": os.path.basename(os.path.dirname(os.path.abspath(_capi.LIB_PATH))) + "/" + os.path.basename(_capi.LIB_PATH),
       "has_merge": has_merge, "map0_edges": m[0].n_edges, "map1_edges": m[1].n_edges, "intersections": int(n)}
times, counts = {}, {}
# the variants alternate over the rounds, so that a drift of the machine falls on all of them alike
for rnd in range(a.rounds):
    for tag, op in OPS.items():
        for ftag, flags in FLAGS:
            c3, ms = timed(lambda: h.overlay_map(*args, flags, (cc, pc, fcap), *bufs, **kw(op)))
            times.setdefault("%s_%s" % (tag, ftag), []).append(ms)
            counts["%s_%s" % (tag, ftag)] = [int(v) for v in c3]
out["ms_best"] = {k: min(min(r) for r in v) for k, v in times.items()}
out["ms_best_per_round"] = {k: [min(r) for r in v] for k, v in times.items()}
out["counts"] = counts  # (chains, points, faces) of every variant: before and after the merge
ok = True
if has_merge and not a.no_check:
    same = {}
    for tag, op in OPS.items():
        for drop in (0, 1):
            unmerged = read_map(*h.overlay_map(*args, drop, (cc, pc, fcap), *bufs, **kw(op)))
            want = G.merged_map(unmerged, np_form=True)
            got = read_map(*h.overlay_map(*args, drop | MERGE, (cc, pc, fcap), *bufs, **kw(op)))
            same["%s_drop%d" % (tag, drop)] = bool(all(got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in want))
    out["merged_equals_definition"] = same
    ok = all(same.values())
h.close()
out["ok"] = bool(ok)
print(json.dumps(out))
sys.exit(0 if ok else 1)
