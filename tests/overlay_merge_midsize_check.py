#!/usr/bin/env python3
"""RJ_OVM_MERGE_PIECES at MID size, exactly (test infrastructure: run as a child process by
tests/test_gpu_overlay_merge_midsize.py so that its maps are freed before the next test): the pair of
tests/overlay_midsize_check.py, lattice_map(330, 20) x lattice_map(700, 5), 4.4 M and 4.9 M edges -- more staged pieces
than one trip of the grid-stride loops of k_ovm_join / k_ovm_merge_points covers.  On the device's own records and vertex
faces: every array and the counts of rj_overlay_map_op with the flag, for clip and (union, pair) and both drop settings,
against the numpy form of the definition (tests/overlay_merge_ref.py: merge_np) applied to the numpy form of the helper's
unmerged map (tests/overlay_ops_ref.py: output_maps_np), bit for bit."""
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
import overlay_ops_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--g0", type=int, default=330)
ap.add_argument("--k0", type=int, default=20)
ap.add_argument("--g1", type=int, default=700)
ap.add_argument("--k1", type=int, default=5)
ap.add_argument("--seeds", type=int, nargs=2, default=(31, 32))
ap.add_argument("--small", action="store_true", help="do not require the sizes (a trial of the script itself)")
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
    assert m[0].n_edges > 2097152 and m[1].n_edges > 2097152 and n > 262144, out
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
walk = R.walk_np(m, recs, faces)
out["setup_s"] = round(time.perf_counter() - t_start, 2)

args = (xs[0], xs[1], n, fc[0], fc[1])
bad = []
out["cases"] = {}
for how, by in (("intersection", "map0"), ("union", "pair")):
    tag = "%s/%s" % (how, by)
    op = (_capi.OVERLAY_HOW[how], _capi.OVERLAY_BY[by])
    t0 = time.perf_counter()
    unmerged = R.output_maps_np(m, recs, faces, how, by, walk=walk)
    info = {}
    for drop in (0, 1):
        w = G.merged_map(unmerged[drop], np_form=True)
        true = (len(w["left"]), len(w["xy"]), len(w["face_pairs"]))
        flags = drop | _capi.RJ_OVM_MERGE_PIECES
        try:
            h.overlay_map(*args, flags, (0, 0, 0), None, None, None, None, None, None, op=op)
            counts = (0, 0, 0)
        except _capi.MapOverflow as e:
            counts = tuple(int(v) for v in e.counts)
        info["drop%d" % drop] = {"unmerged": [len(unmerged[drop]["left"]), len(unmerged[drop]["xy"])], "merged": list(counts[:2])}
        if counts != true:
            bad.append((tag, "drop=%d" % drop, "counts", counts, true))
            continue
        cc, pc, fcap = counts
        bufs = [h.alloc(16 * max(1, pc)), h.alloc(4 * (cc + 1)), h.alloc(4 * max(1, cc)), h.alloc(4 * max(1, cc)), h.alloc(8 * max(1, fcap)),
                h.alloc(4 * max(1, cc))]
        c3 = tuple(int(v) for v in h.overlay_map(*args, flags, counts, *bufs, op=op))
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
        if drop and cc and int(np.diff(g["row_index"].astype(np.int64)).min()) < 2:
            bad.append((tag, "a chain of fewer than two points with both flags"))
    info["s"] = round(time.perf_counter() - t0, 2)
    out["cases"][tag] = info
h.close()
out["bad"] = bad
out["ok"] = not bad
out["total_s"] = round(time.perf_counter() - t_start, 2)
print(json.dumps(out))
sys.exit(0 if out["ok"] else 1)
