#!/usr/bin/env python3
"""The overlay operations at FULL size (BASELINE config 4, USCounty x Zipcode stand-ins), not collected by pytest, in the
pattern of tests/overlay_map_fullsize_check.py: in ONE process, on the same records, best of --reps wall times of
  rj_overlay_faces / rj_overlay_map                     (the intersection's own kernels),
  rj_overlay_faces_op / rj_overlay_map_op (intersection, pair)   -- the same passes with the operation as an argument,
  rj_overlay_faces_op / rj_overlay_map_op (union, pair)          -- the largest output,
and the checks that cost nothing at this size: (intersection, pair) through the _op calls equals the calls without _op,
array by array and row by row; the union's rows are the intersection's and the symmetric difference's, disjoint.
RAYJOIN_AMD_LIB=<another revision's library> measures that revision's calls without _op alone (no _op symbols there)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rayjoin_amd import _capi, maps, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--m0", default="USCounty")
ap.add_argument("--m1", default="Zipcode")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
ctx = maps.Context([synth.standin(a.m0, a.scale), synth.standin(a.m1, a.scale)]).load()
m = ctx.maps
h = _capi.Handle(0)
has_op = hasattr(_capi.load(), "rj_overlay_faces_op")
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
UNION, INTER, SYM = (_capi.RJ_OV_UNION, 0), (_capi.RJ_OV_INTERSECTION, 0), (_capi.RJ_OV_SYMDIFF, 0)
variants = [("old", None)] + ([("op_intersection", INTER), ("op_union", UNION)] if has_op else [])


def kw(op):
    return {} if op is None else {"op": op}


def timed(fn):
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return r, [round(v, 3) for v in ms]


# capacities for the largest output
rcap = 4 * n + 2 * (m[0].n_chains + m[1].n_chains) + 1024
rows = h.alloc(_capi.FACE_DTYPE.itemsize * rcap)
try:
    h.overlay_map(*args, 0, (0, 0, 0), None, None, None, None, None, None, **kw(UNION if has_op else None))
    counts = (0, 0, 0)
except _capi.MapOverflow as e:
    counts = e.counts
cc, pc, fcap = counts
bufs = [h.alloc(16 * max(1, pc)), h.alloc(4 * (cc + 1)), h.alloc(4 * max(1, cc)), h.alloc(4 * max(1, cc)), h.alloc(8 * max(1, fcap)),
        h.alloc(4 * max(1, cc))]


def read_map(k, p, f):
    return dict(xy=bufs[0].to_host(np.int64, 2 * p), row_index=bufs[1].to_host(np.uint32, k + 1), left=bufs[2].to_host(np.int32, k),
                right=bufs[3].to_host(np.int32, k), face_pairs=bufs[4].to_host(np.int32, 2 * f), origin=bufs[5].to_host(np.uint32, k))


out = {"lib": os.path.basename(_capi.LIB_PATH), "map0_edges": m[0].n_edges, "map1_edges": m[1].n_edges, "intersections": n}
got_rows, got_maps = {}, {}
# the variants alternate over the rounds, so that a drift of the machine falls on all of them alike
for rnd in range(a.rounds):
    for tag, op in variants:
        nrows, ms = timed(lambda: h.overlay_faces(*args, rcap, rows, **kw(op)))
        out.setdefault("faces_%s_ms" % tag, []).append(ms)
        got_rows[tag] = rows.to_host(_capi.FACE_DTYPE, nrows)
        for drop in (0, 1):
            c3, ms = timed(lambda: h.overlay_map(*args, drop, (cc, pc, fcap), *bufs, **kw(op)))
            out.setdefault("map_%s_%s_ms" % (tag, "drop" if drop else "flags0"), []).append(ms)
            if not drop:
                got_maps[tag] = read_map(*c3)
                out["map_%s_counts" % tag] = [int(v) for v in c3]
for key in [k for k in out if k.endswith("_ms")]:
    out[key + "_best"] = min(min(r) for r in out[key])
    out[key + "_best_per_round"] = [min(r) for r in out[key]]
    del out[key]
ok = True
if has_op:
    same = {name: bool(np.array_equal(got_maps["old"][name], got_maps["op_intersection"][name])) for name in got_maps["old"]}
    out["op_intersection_map_equals_old"] = same
    out["op_intersection_rows_equal_old"] = bool(np.array_equal(got_rows["old"], got_rows["op_intersection"]))
    nsym = h.overlay_faces(*args, rcap, rows, op=SYM)
    sym = rows.to_host(_capi.FACE_DTYPE, nsym)
    both = np.concatenate([got_rows["old"], sym])
    order = np.argsort((both["face"][:, 0].astype(np.int64) << 32) | both["face"][:, 1].astype(np.int64), kind="stable")
    out["union_rows"] = len(got_rows["op_union"])
    out["union_is_intersection_plus_symdiff"] = bool(np.array_equal(both[order], got_rows["op_union"]))
    ok = all(same.values()) and out["op_intersection_rows_equal_old"] and out["union_is_intersection_plus_symdiff"]
out["rows_old"] = len(got_rows["old"])
h.close()
out["ok"] = bool(ok)
print(json.dumps(out))
sys.exit(0 if ok else 1)
