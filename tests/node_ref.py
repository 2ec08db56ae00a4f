"""Noding a chain map, by definition: plain Python integers, dicts and sorted, nothing shared with
rayjoin_amd/csrc/rj_node.h.  Where the header tests a point with an orientation sign, a box and two comparisons and orders
the cuts of an edge by one coordinate difference, this reads both off the point's parameter on the edge's line:
q = a + t (b - a) with t = (q - a) . (b - a) / |b - a|^2, never divided out -- q is inside iff the cross product is zero
and 0 < t < 1, and the cuts ascend by t.

node_ref(xy, row_index, records, drop_last=False) -> (out_xy [n, 2] int64, out_row uint32, origin uint32, counts) or
raises Invalid; records a list of (eid0, eid1, kind).  counts a dict with the names of rj_node_counts."""
import numpy as np

PROPER, TOUCH, OVERLAP, EQUAL = 1, 2, 3, 4
COUNTS = ("n_points", "n_edges", "n_cuts", "n_cut_edges", "n_max_cuts", "n_used", "n_proper", "n_equal")
L = 1 << 46


class Invalid(ValueError):
    pass


def param(a, b, q):
    """-> the numerator of q's parameter on a -> b when q lies strictly inside that segment, else None"""
    dx, dy = b[0] - a[0], b[1] - a[1]
    if dx == 0 and dy == 0:
        return None
    if dx * (q[1] - a[1]) - dy * (q[0] - a[0]) != 0:
        return None
    t, full = (q[0] - a[0]) * dx + (q[1] - a[1]) * dy, dx * dx + dy * dy
    return t if 0 < t < full else None


def node_ref(xy, row_index, records, drop_last=False):
    pts = [(int(x), int(y)) for x, y in np.asarray(xy, np.int64).reshape(-1, 2).tolist()]
    row = [int(v) for v in np.asarray(row_index).tolist()]
    nc = max(0, len(row) - 1)
    if nc == 0:
        if pts or records:
            raise Invalid("points or records without chains")
        return np.zeros((0, 2), np.int64), np.zeros(1, np.uint32), np.zeros(0, np.uint32), dict.fromkeys(COUNTS, 0)
    if row[0] != 0 or row[-1] != len(pts) or any(b >= e for b, e in zip(row, row[1:])):
        raise Invalid("row_index")
    if any(not -L <= v < L for p in pts for v in p):
        raise Invalid("coordinate")
    if drop_last and any(e - b < 2 or pts[b] != pts[e - 1] for b, e in zip(row, row[1:])):
        raise Invalid("a chain is not closed")
    first_point = [p for c in range(nc) for p in range(row[c], row[c + 1] - 1)]  # of every edge
    chain = [c for c in range(nc) for _ in range(row[c], row[c + 1] - 1)]
    ne = len(first_point)
    last = None
    for e, f, k in records:
        if not (0 <= e < f < ne and k in (PROPER, TOUCH, OVERLAP, EQUAL)):
            raise Invalid("record")
        if last is not None and (e, f) <= last:
            raise Invalid("order")
        last = (e, f)
        if pts[first_point[e]] == pts[first_point[e] + 1] or pts[first_point[f]] == pts[first_point[f] + 1]:
            raise Invalid("zero-length edge")
    cut_sets = {}  # edge -> {point: parameter}
    counts = dict.fromkeys(COUNTS, 0)
    for e, f, k in records:
        if k == PROPER:
            counts["n_proper"] += 1
        if k == EQUAL:
            counts["n_equal"] += 1
        if k not in (TOUCH, OVERLAP):
            continue
        counts["n_used"] += 1
        for host, other in ((e, f), (f, e)):
            a, b = pts[first_point[host]], pts[first_point[host] + 1]
            for q in (pts[first_point[other]], pts[first_point[other] + 1]):
                t = param(a, b, q)
                if t is not None:
                    cut_sets.setdefault(host, {})[q] = t
    out, out_row, origin = [], [0], []
    e = 0
    for c in range(nc):
        for p in range(row[c], row[c + 1]):
            is_last = p == row[c + 1] - 1
            if is_last and drop_last:
                continue
            out.append(pts[p])
            if is_last:
                continue
            inserted = [q for q, _ in sorted(cut_sets.get(e, {}).items(), key=lambda item: item[1])]
            out.extend(inserted)
            origin.extend([e] * (1 + len(inserted)))
            e += 1
        out_row.append(len(out))
    sizes = [len(v) for v in cut_sets.values()]
    counts.update(n_points=len(out), n_edges=len(origin), n_cuts=sum(sizes), n_cut_edges=len(sizes), n_max_cuts=max(sizes, default=0))
    return np.array(out, np.int64).reshape(-1, 2), np.array(out_row, np.uint32), np.array(origin, np.uint32), counts
