#!/usr/bin/env python3
"""rj_map_node at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/crossings_fullsize_check.py; profiles/node_fullsize.txt holds its output): a brick wall of COLS x ROWS rectangles
of 10 x 6 units, the odd rows moved by 5 -- every brick misses the corners of the bricks above and below it.  At the
default 1000 x 1000 that is 1 M rings, 5 M points as closed chains.  rj_map_crossings and rj_map_node are each timed once
warm (the second of two equal calls), HIP events round every stage; the noded rings then go through rj_rings_map and
rj_map_crossings again.

Asserted: the number of cuts, 2 COLS (ROWS - 1) -- every row boundary carries COLS brick corners from below inside the
bottom edges above it and COLS from above inside the top edges below it; the definition (tests/node_ref.py) confirms
this closed form on three small walls first --, no proper crossing, and no crossing and no conflict in the chain map of
the noded rings.

  --long N   instead: one edge with N T-junctions in scrambled order (NC.long_edge), every seventh twice -- n_cuts ==
             n_max_cuts == N is asserted; the stage times show that no stage is serial in the cuts of one edge."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crossings_ref as CR  # noqa: E402
import node_cases as NC  # noqa: E402
import node_ref as NR  # noqa: E402
from rayjoin_amd import _capi, maps, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cols", type=int, default=1000)
ap.add_argument("--rows", type=int, default=1000)
ap.add_argument("--long", type=int, default=0)
ap.add_argument("--out", help="also write the report to this file")
a = ap.parse_args()
W, H, SHIFT, UNIT = 10, 6, 5, 1 << 16
CROSS_STAGES = ("edges+sums", "registrations+sort", "runs+items", "pairs", "hits", "all")
NODE_STAGES = ("check", "candidates", "sort+kept", "per edge+scan", "scatters", "all")


def closed_form(cols, rows):
    return 2 * cols * (rows - 1)


for cols, rows in ((5, 4), (4, 3), (3, 5)):  # the closed form against the definition
    m = NC.wall_map((cols, rows, W, H, SHIFT))
    assert NR.node_ref(m[0], m[1], CR.map_crossings_ref(*m)[0])[3]["n_cuts"] == closed_form(cols, rows), (cols, rows)


def wall(cols, rows):
    """NC.brick_rings, vectorised"""
    r, c = np.divmod(np.arange(cols * rows, dtype=np.int64), cols)
    x0, y0 = c * W + (r % 2) * SHIFT, r * H
    xy = np.stack([np.stack([x0, y0], 1), np.stack([x0 + W, y0], 1), np.stack([x0 + W, y0 + H], 1), np.stack([x0, y0 + H], 1)], 1).reshape(-1, 2) * UNIT
    return np.arange(0, 4 * cols * rows + 1, 4, dtype=np.uint32), xy, np.arange(1, cols * rows + 1, dtype=np.int32)


ring_row, ring_xy, ring_face = wall(a.cols, a.rows)
if a.cols * a.rows <= 64:
    small = NC.brick_rings(a.cols, a.rows, W, H, SHIFT, unit=UNIT)
    assert all(np.array_equal(x, y) for x, y in zip(small, (ring_row, ring_xy, ring_face)))
row, xy = maps.closed_chains_of_rings(ring_row, ring_xy)
FLAGS = _capi.RJ_NODE_DROP_LAST
if a.long:
    (xy, row), _ = NC.long_edge(a.long)
    FLAGS = 0
np_, nc = len(xy), len(row) - 1
h = _capi.Handle(0)
d_xy, d_row = h.alloc(16 * np_).from_host(xy), h.alloc(4 * (nc + 1)).from_host(row)
try:
    found = h.map_crossings(d_xy, np_, d_row, nc, 0, None)["n_found"]
except _capi.CrossingsOverflow as e:
    found = e.counts["n_found"]
d_rec = h.alloc(16 * max(1, found))
for _ in range(2):
    cross = h.map_crossings(d_xy, np_, d_row, nc, found, d_rec)
cross_ms = [h.get_option("cross_last_us%d" % k) / 1000.0 for k in range(6)]
try:
    n_out = h.map_node(d_xy, np_, d_row, nc, d_rec, found, FLAGS, 0, None, None)["n_points"]
except _capi.NodeOverflow as e:
    n_out = e.counts["n_points"]
o_xy, o_row, o_origin = h.alloc(16 * n_out), h.alloc(4 * (nc + 1)), h.alloc(4 * n_out)
for _ in range(2):
    node = h.map_node(d_xy, np_, d_row, nc, d_rec, found, FLAGS, n_out, o_xy, o_row, o_origin)
node_ms = [h.get_option("node_last_us%d" % k) / 1000.0 for k in range(6)]
if a.long:
    assert node["n_cuts"] == node["n_max_cuts"] == a.long and node["n_cut_edges"] == 1 and node["n_points"] == np_ + a.long, node
    first = o_xy.to_host(np.int64, 2 * (a.long + 2)).reshape(-1, 2)
    assert np.array_equal(first[:, 0], np.arange(a.long + 1, -1, -1)) and not first[:, 1].any()
else:
    assert node["n_cuts"] == closed_form(a.cols, a.rows) and node["n_proper"] == 0 and node["n_points"] == 4 * nc + node["n_cuts"], node
    d_face = h.alloc(4 * nc).from_host(ring_face)
    dm = ops.rings_map(h, o_row, o_xy, n_out, d_face, nc)
    _, after = dm.Crossings(h)
    assert after["n_found"] == 0 and dm.counts["n_conflicts"] == 0, (after, dm.counts)

lines = ["one edge with %d T-junctions: %d chains, %d points, %d edges" % (a.long, nc, np_, np_ - nc) if a.long else
         "brick wall %d x %d: %d rings, %d points as closed chains, %d edges" % (a.cols, a.rows, nc, np_, np_ - nc),
         "rj_map_crossings: %s" % {k: cross[k] for k in ("n_found", "n_touch", "n_overlap", "n_equal", "n_proper")},
         "  ms  " + "  ".join("%s %.3f" % (n, v) for n, v in zip(CROSS_STAGES, cross_ms)),
         "rj_map_node (%sedge_origin): %s" % ("RJ_NODE_DROP_LAST, " if FLAGS else "", node),
         "  ms  " + "  ".join("%s %.3f" % (n, v) for n, v in zip(NODE_STAGES, node_ms)),
         "node / crossings: %.3f" % (node_ms[5] / cross_ms[5]),
         "largest node stage: %s, %.0f %% of the call" % (NODE_STAGES[int(np.argmax(node_ms[:5]))], 100.0 * max(node_ms[:5]) / node_ms[5]),
         ]
if not a.long:
    lines.append("rj_rings_map of the noded rings: %s; its crossings: %d" % (dm.counts, after["n_found"]))
print("\n".join(lines))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
h.close()
