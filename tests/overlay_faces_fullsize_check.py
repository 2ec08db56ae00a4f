#!/usr/bin/env python3
"""The overlay's face table at FULL size (BASELINE config 4, USCounty x Zipcode stand-ins), checked by geometry (test
infrastructure: run as a child process by tests/test_gpu_overlay_faces.py so that its 30 M-segment maps are freed before
the next test).  Every face of map 0 not on the map's border lies inside map 1 (a finer lattice over the same box): its
rows sum to its own shoelace area.  Areas are compared as exact integers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rayjoin_amd import _capi, maps, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--m0", default="USCounty")
ap.add_argument("--m1", default="Zipcode")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=5)
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
rcap = 4 * n + m[0].n_chains + m[1].n_chains + 1024
out = h.alloc(_capi.FACE_DTYPE.itemsize * rcap)
ms = []
for _ in range(a.reps):
    t0 = time.perf_counter()
    nrows = h.overlay_faces(xs[0], xs[1], n, fc[0], fc[1], rcap, out)
    ms.append((time.perf_counter() - t0) * 1e3)
raw = out.to_host(_capi.FACE_DTYPE, nrows)
h.close()

# exact table sums per face of map 0 (Python ints), and exact shoelace areas per face (object arrays)
a2 = [(int(hi) << 64) | int(lo) for lo, hi in zip(raw["area2_lo"].tolist(), raw["area2_hi"].tolist())]
per0 = {}
for f0, v in zip(raw["face"][:, 0].tolist(), a2):
    per0[f0] = per0.get(f0, 0) + v
g = m[0]
p1 = g.edge_p1().astype(np.int64)
counts = np.diff(g.row_index.astype(np.int64)) - 1
chain = np.repeat(np.arange(g.n_chains), counts)
x0, y0 = g.pts[p1, 0].astype(object), g.pts[p1, 1].astype(object)
x1, y1 = g.pts[p1 + 1, 0].astype(object), g.pts[p1 + 1, 1].astype(object)
cr = x0 * y1 - x1 * y0
starts = np.r_[0, np.cumsum(counts)[:-1]]
per_chain = np.add.reduceat(cr, starts)
shoe = {}
border = set()
for c, v in enumerate(per_chain.tolist()):
    lf, rf = int(g.left[c]), int(g.right[c])
    if lf:
        shoe[lf] = shoe.get(lf, 0) + v
    if rf:
        shoe[rf] = shoe.get(rf, 0) - v
    if lf == 0 or rf == 0:
        border.add(lf or rf)
checked = off = over = 0
for f, s in shoe.items():
    got = per0.get(f, 0)
    if f in border:
        over += got > s + s // 10**9
    else:
        checked += 1
        off += abs(got - s) > s // 10**9
print(json.dumps({"map0_edges": g.n_edges, "map1_edges": m[1].n_edges, "intersections": n, "rows": int(nrows),
                  "face_table_ms": [round(v, 3) for v in ms], "face_table_ms_best": round(min(ms), 3),
                  "negative_rows": sum(v <= 0 for v in a2), "interior_faces_checked": checked,
                  "interior_faces_off": off, "border_faces_over": over}))
