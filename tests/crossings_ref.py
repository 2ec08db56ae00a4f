"""The crossings inside one chain map, by definition: plain Python integers, every pair of edges, no grid, nothing shared
with rayjoin_amd/csrc/rj_crossings.h.  Where the header decides from four orientation signs, this solves the two
segments' parametric equations a + t r = c + u s in exact integers (t = tn / den, u = un / den, never divided out) and
reads the relation off t and u.

map_crossings_ref(xy, row_index) -> (records, counts): records a list of (eid0, eid1, kind) with eid0 < eid1, ascending;
counts a dict with the names of rj_crossings_counts."""
import numpy as np

PROPER, TOUCH, OVERLAP, EQUAL = 1, 2, 3, 4
COUNTS = ("n_found", "n_proper", "n_touch", "n_overlap", "n_equal", "n_edges", "n_zero_edges")
KIND_NAME = {PROPER: "n_proper", TOUCH: "n_touch", OVERLAP: "n_overlap", EQUAL: "n_equal"}


def relation(e, f):
    """e, f = (ax, ay, bx, by) in Python ints, both of non-zero length -> 0 or the kind"""
    ax, ay, bx, by = e
    cx, cy, dx, dy = f
    rx, ry, sx, sy = bx - ax, by - ay, dx - cx, dy - cy
    qx, qy = cx - ax, cy - ay
    den = rx * sy - ry * sx
    if den != 0:  # the lines meet in one point: a + t r = c + u s
        tn, un = qx * sy - qy * sx, qx * ry - qy * rx
        if den < 0:
            den, tn, un = -den, -tn, -un
        if not (0 <= tn <= den and 0 <= un <= den):
            return 0
        t_end, u_end = tn in (0, den), un in (0, den)
        if t_end and u_end:
            return 0  # a shared vertex
        return TOUCH if t_end or u_end else PROPER
    if qx * ry - qy * rx != 0:
        return 0  # parallel, two lines
    e0, e1 = sorted([(ax, ay), (bx, by)])
    f0, f1 = sorted([(cx, cy), (dx, dy)])
    lo, hi = max(e0, f0), min(e1, f1)
    if lo >= hi:
        return 0  # apart, or end to end
    return EQUAL if (e0, e1) == (f0, f1) else OVERLAP


def edges_of(xy, row_index):
    """edge e = p - c of point p (not the last) of chain c -> [ne, 4] int64"""
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    row = np.asarray(row_index, np.int64)
    out = [np.concatenate([xy[b:e - 1], xy[b + 1:e]], axis=1) for b, e in zip(row[:-1], row[1:]) if e - b >= 2]
    return np.concatenate(out) if out else np.zeros((0, 4), np.int64)


def map_crossings_ref(xy, row_index):
    E = edges_of(xy, row_index)
    ne = len(E)
    live = (E[:, 0] != E[:, 2]) | (E[:, 1] != E[:, 3])
    x0, x1 = np.minimum(E[:, 0], E[:, 2]), np.maximum(E[:, 0], E[:, 2])
    y0, y1 = np.minimum(E[:, 1], E[:, 3]), np.maximum(E[:, 1], E[:, 3])
    rows = E.tolist()
    records = []
    counts = dict.fromkeys(COUNTS, 0)
    counts["n_edges"], counts["n_zero_edges"] = ne, int(ne - live.sum())
    for e in range(ne):
        if not live[e]:
            continue
        # every later edge; the ones whose closed boxes miss this edge's box have no point in common with it
        near = live[e + 1:] & (x0[e + 1:] <= x1[e]) & (x1[e + 1:] >= x0[e]) & (y0[e + 1:] <= y1[e]) & (y1[e + 1:] >= y0[e])
        for f in (np.nonzero(near)[0] + e + 1).tolist():
            k = relation(rows[e], rows[f])
            if k:
                records.append((e, f, k))
                counts[KIND_NAME[k]] += 1
    counts["n_found"] = len(records)
    return records, counts
