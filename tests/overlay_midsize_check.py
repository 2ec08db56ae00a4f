#!/usr/bin/env python3
"""The overlay's face table and output map at MID size, exactly (test infrastructure: run as a child process by
tests/test_gpu_overlay_midsize.py so that its maps are freed before the next test): lattice_map(330, 20) x
lattice_map(700, 5), 4.4 M and 4.9 M edges, about half a million intersections.  Both maps hold more than 8192 * 256 =
2 097 152 edges, so the wave loops of k_ovf_contrib* / k_ovm_emit* take a second trip, and more than 64^3 = 262 144
records, so wave_first_record's 64-ary search takes its third level: the two inequalities are asserted first, they are
the point of the check.  Then, on the device's OWN records and vertex faces (tests/overlay_fullsize_check.py holds them
to the oracle at this scale), every row of rj_overlay_faces / rj_overlay_faces_op and the counts and every array of
rj_overlay_map / rj_overlay_map_op against the numpy forms of the plain-Python helper (tests/overlay_ops_ref.py:
face_rows_np, output_maps_np), bit for bit."""
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
import overlay_ops_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--g0", type=int, default=330)
ap.add_argument("--k0", type=int, default=20)
ap.add_argument("--g1", type=int, default=700)
ap.add_argument("--k1", type=int, default=5)
ap.add_argument("--seeds", type=int, nargs=2, default=(31, 32))
ap.add_argument("--small", action="store_true", help="do not require the two sizes (a trial of the script itself)")
a = ap.parse_args()
t_start = time.perf_counter()
ctx = maps.Context([synth.lattice_map(a.g0, a.k0, a.seeds[0]), synth.lattice_map(a.g1, a.k1, a.seeds[1])]).load()
m = ctx.maps
h = _capi.Handle(0)
for im in range(2):
    h.upload_map(im, m[im].pts, m[im].row_index, m[im].left, m[im].right)
h.build_lbvh(0)
h.build_lbvh(1)
cap = int(0.2 * (m[0].n_edges + m[1].n_edges))
pairs = h.alloc(8 * cap)
n = h.lsi_query(1, 0, 0, m[0].n_edges, cap, pairs)
out = {"map0_edges": m[0].n_edges, "map1_edges": m[1].n_edges, "intersections": int(n)}
if not a.small:
    assert m[0].n_edges > 2097152 and m[1].n_edges > 2097152, out  # a second trip of the wave loops, in both maps
    assert n > 262144, out                                             # the third level of the 64-ary record search
fc = [h.alloc(4 * m[i].n_points) for i in range(2)]
cl = [h.alloc(4 * m[i].n_points) for i in range(2)]
for im in range(2):
    h.pip_query(1 - im, im, None, 0, m[im].n_points, cl[im], fc[im])
xs = [h.alloc(48 * max(1, n)) for _ in range(2)]
for im in range(2):
    h.overlay_edge_xsects(im, pairs, n, xs[im])
h.sync()
for b in cl + [pairs]:
    b.free()
recs = [xs[im].to_host(_capi.XSECT_DTYPE, n) for im in range(2)]
faces = [fc[im].to_host(np.int32, m[im].n_points) for im in range(2)]
for im in range(2):  # what the numpy forms rely on: records ordered by eid[im], labels that are faces
    e = recs[im]["eid"][:, im]
    assert np.all(e[1:] >= e[:-1]) and np.all(faces[im] >= 0)
    same = e[1:] == e[:-1]
    assert np.all(recs[im]["mid_point_polygon_id"][:-1][same] >= 0)

walk = R.walk_np(m, recs, faces)
sums = [R.piece_cross_sums_np(w) for w in walk]
out["pieces"] = [len(s) for s in sums]
out["setup_s"] = round(time.perf_counter() - t_start, 2)

rcap = 4 * n + 2 * (m[0].n_chains + m[1].n_chains) + 1024
rows = h.alloc(_capi.FACE_DTYPE.itemsize * rcap)
args = (xs[0], xs[1], n, fc[0], fc[1])
# (intersection, pair) through both entry points: None = the calls without _op
CASES = [("intersection", "pair", None), ("intersection", "pair", "op"), ("union", "pair", "op"), ("difference", "pair", "op"),
         ("intersection", "map0", "op"), ("identity", "map1", "op")]
bad = []
out["cases"] = {}
expected = {}  # (how, by) -> (rows, maps): both entry points of (intersection, pair) are held to the same arrays
for how, by, entry in CASES:
    tag = "%s/%s%s" % (how, by, "" if entry else " (without _op)")
    op = (_capi.OVERLAY_HOW[how], _capi.OVERLAY_BY[by]) if entry else None
    t0 = time.perf_counter()
    if (how, by) not in expected:
        expected[how, by] = (R.face_rows_np(m, recs, faces, how, by, walk=walk, sums=sums, arrays=True),
                             R.output_maps_np(m, recs, faces, how, by, walk=walk))
    want, want_maps = expected[how, by]
    nrows = h.overlay_faces(*args, rcap, rows, op=op)
    got = rows.to_host(_capi.FACE_DTYPE, nrows)
    ok = (nrows == len(want[0]) and np.array_equal(got["face"][:, 0], want[0]) and np.array_equal(got["face"][:, 1], want[1])
          and np.array_equal(got["area2_lo"], want[2]) and np.array_equal(got["area2_hi"], want[3]))
    if not ok:
        bad.append((tag, "face rows", int(nrows), len(want[0])))
    info = {"rows": int(nrows)}
    for drop in (0, 1):
        w = want_maps[drop]
        true = (len(w["left"]), len(w["xy"]), len(w["face_pairs"]))
        try:
            h.overlay_map(*args, drop, (0, 0, 0), None, None, None, None, None, None, op=op)
            counts = (0, 0, 0)
        except _capi.MapOverflow as e:
            counts = tuple(int(v) for v in e.counts)
        info["counts_drop%d" % drop] = list(counts)
        if counts != true:
            bad.append((tag, "drop=%d" % drop, "counts", counts, true))
            continue
        cc, pc, fcap = counts
        bufs = [h.alloc(16 * max(1, pc)), h.alloc(4 * (cc + 1)), h.alloc(4 * max(1, cc)), h.alloc(4 * max(1, cc)), h.alloc(8 * max(1, fcap)),
                h.alloc(4 * max(1, cc))]
        c3 = tuple(int(v) for v in h.overlay_map(*args, drop, counts, *bufs, op=op))
        g = dict(xy=bufs[0].to_host(np.int64, 2 * pc).reshape(-1, 2), row_index=bufs[1].to_host(np.uint32, cc + 1),
                 left=bufs[2].to_host(np.int32, cc), right=bufs[3].to_host(np.int32, cc),
                 face_pairs=bufs[4].to_host(np.int32, 2 * fcap).reshape(-1, 2), origin=bufs[5].to_host(np.uint32, cc))
        for b in bufs:
            b.free()
        if c3 != true:
            bad.append((tag, "drop=%d" % drop, "counts of the filling call", c3, true))
        for name in g:
            if g[name].shape != w[name].shape or not np.array_equal(g[name], w[name]):
                bad.append((tag, "drop=%d" % drop, name))
        if not np.array_equal(g["face_pairs"], got["face"]):
            bad.append((tag, "drop=%d" % drop, "face_pairs are not the table's rows"))
    info["s"] = round(time.perf_counter() - t0, 2)
    out["cases"][tag] = info
h.close()
out["one_point_pieces"] = int(want_maps[0]["n_one_point"])
out["bad"] = bad
out["ok"] = not bad
out["total_s"] = round(time.perf_counter() - t_start, 2)
print(json.dumps(out))
sys.exit(0 if out["ok"] else 1)
