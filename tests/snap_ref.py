"""Cutting a chain map at its touches, overlaps and rounded proper crossings, by definition: plain Python integers and
Fractions, dicts and sorted, nothing shared with rayjoin_amd/csrc/rj_snap.h.  Where the header divides in two 26-step
partial divisions and orders the cuts of an edge by (major offset, minor offset), this solves the two lines with Fraction,
rounds with floor(v + 1/2) on the exact coordinate, and orders the cuts of an edge a -> b by (q - a) . (b - a): for points
on the segment that is their parameter, and for rounded crossing points it ascends with both offsets (both are monotone
along the edge and the major one has a nonzero weight), so it is the same order.

snap_ref(xy, row_index, records, drop_last=False) -> (out_xy [n, 2] int64, out_row uint32, origin uint32, counts) or
raises Invalid; records a list of (eid0, eid1, kind); counts a dict with the names of rj_snap_counts.
snap_rounds_ref(xy, row_index, max_rounds=8, drop_last=False) -> (out_xy, out_row, rounds, clean, remaining): what
ops.map_snap_rounds does, with tests/crossings_ref.py as the check."""
import math
from fractions import Fraction

import numpy as np

import crossings_ref as CR
from node_ref import EQUAL, OVERLAP, PROPER, TOUCH, Invalid, param

COUNTS = ("n_points", "n_edges", "n_cuts", "n_cut_edges", "n_max_cuts", "n_used", "n_proper", "n_equal", "n_exact", "n_at_end", "n_stale")
L = 1 << 46


def rnd(v):
    return math.floor(v + Fraction(1, 2))


def crossing_point(a, b, c, d):
    """-> None where the open segments a-b and c-d do not cross in one point, else (the rounded point, was it exact)"""
    r, s = (b[0] - a[0], b[1] - a[1]), (d[0] - c[0], d[1] - c[1])
    den = r[0] * s[1] - r[1] * s[0]
    if den == 0:
        return None
    w = (c[0] - a[0], c[1] - a[1])
    t, u = Fraction(w[0] * s[1] - w[1] * s[0], den), Fraction(w[0] * r[1] - w[1] * r[0], den)
    if not (0 < t < 1 and 0 < u < 1):
        return None
    x, y = a[0] + r[0] * t, a[1] + r[1] * t
    return (rnd(x), rnd(y)), x.denominator == 1 and y.denominator == 1


def snap_ref(xy, row_index, records, drop_last=False):
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
    ne = len(first_point)
    ends = lambda e: (pts[first_point[e]], pts[first_point[e] + 1])  # noqa: E731
    last = None
    for e, f, k in records:
        if not (0 <= e < f < ne and k in (PROPER, TOUCH, OVERLAP, EQUAL)):
            raise Invalid("record")
        if last is not None and (e, f) <= last:
            raise Invalid("order")
        last = (e, f)
        if ends(e)[0] == ends(e)[1] or ends(f)[0] == ends(f)[1]:
            raise Invalid("zero-length edge")
    cut_sets = {}  # edge -> set of points
    counts = dict.fromkeys(COUNTS, 0)
    for e, f, k in records:
        if k == EQUAL:
            counts["n_equal"] += 1
        elif k == PROPER:
            counts["n_proper"] += 1
            hit = crossing_point(*ends(e), *ends(f))
            if hit is None:
                counts["n_stale"] += 1
                continue
            q, exact = hit
            counts["n_exact"] += exact
            for host in (e, f):
                if q in ends(host):
                    counts["n_at_end"] += 1
                else:
                    cut_sets.setdefault(host, set()).add(q)
        else:
            counts["n_used"] += 1
            for host, other in ((e, f), (f, e)):
                for q in ends(other):
                    if param(*ends(host), q) is not None:
                        cut_sets.setdefault(host, set()).add(q)
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
            a, b = ends(e)
            inserted = sorted(cut_sets.get(e, ()), key=lambda q: (q[0] - a[0]) * (b[0] - a[0]) + (q[1] - a[1]) * (b[1] - a[1]))
            out.extend(inserted)
            origin.extend([e] * (1 + len(inserted)))
            e += 1
        out_row.append(len(out))
    sizes = [len(v) for v in cut_sets.values()]
    counts.update(n_points=len(out), n_edges=len(origin), n_cuts=sum(sizes), n_cut_edges=len(sizes), n_max_cuts=max(sizes, default=0))
    return np.array(out, np.int64).reshape(-1, 2), np.array(out_row, np.uint32), np.array(origin, np.uint32), counts


def dirty(counts):
    """what a cutting round is for: the crossings of the kinds that cut"""
    return counts["n_proper"] + counts["n_touch"] + counts["n_overlap"]


def snap_rounds_ref(xy, row_index, max_rounds=8, drop_last=False):
    xy, row = np.asarray(xy, np.int64).reshape(-1, 2), np.asarray(row_index, np.uint32)
    rounds = []
    while True:
        records, c = CR.map_crossings_ref(xy, row)
        if dirty(c) == 0 or len(rounds) >= max_rounds:
            break
        xy, row, _, sc = snap_ref(xy, row, records)
        rounds.append(dict(crossings=c, snap=sc))
    if drop_last:
        xy, row, _, _ = snap_ref(xy, row, [], True)
    return xy, row, rounds, dirty(c) == 0, c
